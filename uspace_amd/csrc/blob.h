// One layout for every model's packed weights and workspaces (host side only): the aligned arena, the parameter table and
// the loop that packs fp32 checkpoint tensors into a device blob.  Every model describes its parameters with a ParamTable and serves
// num_params / param_numel / weight_bytes / pack_weights from it: uvit.hip, vae.hip (both halves), clip.hip, clip_vision.hip and dino.hip
// (their layers through vit_encoder.h, the patch weight through vit_embed.h), and the fp32 convolution towers inception.hip, lpips.hip,
// idnet.hip and resnet.hip, whose convolutions and batch norms are P_OWNER entries that conv_f32.h's pack step writes.
#pragma once
#include <vector>

#include "common.h"

constexpr size_t US_BLOB_ALIGN = 256;   // every piece of a blob or a workspace starts on a multiple of this
inline size_t us_align_up(size_t v) { return (v + US_BLOB_ALIGN - 1) / US_BLOB_ALIGN * US_BLOB_ALIGN; }

struct Arena {
    size_t off = 0;   // bytes handed out so far = the size to allocate
    size_t align = US_BLOB_ALIGN;   // inception.hip and lpips.hip place their pieces 64 bytes apart
    size_t take(size_t bytes) {
        const size_t o = off;
        off = (off + bytes + align - 1) / align * align;
        return o;
    }
};

// how a fp32 checkpoint tensor is stored in the blob
enum PKind {
    P_F32 = 0,          // copied
    P_BF16 = 1,         // cast (GEMM weights in nn.Linear [N][K] layout, 1x1 convolutions)
    P_CONV3_BF16 = 2,   // 3x3 convolution [Co][Ci][3][3] -> bf16 [Co][9][Ci]
    P_CONV3_F32T = 3,   // ... -> fp32 [Co][9][Ci]
    P_OWNER = 4,        // counted and sized here, stored by the model's own pack step (or folded into another tensor): no space
};

struct PDesc {
    long numel;
    PKind kind;
    int co, ci;             // the conv kinds' channel counts
    size_t offset, bytes;   // in the blob
};

// The entries of one blob.  The first n_params are the caller's parameters, in the order pack_weights receives them; entries
// added after `derived` is set are tensors the model computes at pack time and only take space.
struct ParamTable {
    std::vector<PDesc> p;
    Arena arena;
    int n_params = 0;
    bool derived = false;

    static size_t bytes_of(long numel, PKind k) { return (size_t)numel * ((k == P_BF16 || k == P_CONV3_BF16) ? 2 : 4); }
    int add(long numel, PKind k, int co = 0, int ci = 0) {
        return add_at(k == P_OWNER ? 0 : arena.take(bytes_of(numel, k)), numel, k, co, ci);
    }
    // at `offset` inside space the caller took from the arena itself (several parameters packed into one region)
    int add_at(size_t offset, long numel, PKind k, int co = 0, int ci = 0) {
        p.push_back(PDesc{numel, k, co, ci, offset, bytes_of(numel, k)});
        if (!derived) n_params = (int)p.size();
        return (int)p.size() - 1;
    }
    size_t at(int i) const { return p[i].offset; }
    size_t put(long numel, PKind k) { return at(add(numel, k)); }   // add, and the offset it got
    size_t bytes() const { return arena.off; }
    long numel(int i) const { return (i < 0 || i >= n_params) ? (long)USPACE_ERR_ARG : p[i].numel; }
};

// the two conv kinds' repack launch (vae.hip owns the kernels)
int us_repack_conv3(const float* src, void* dst, int co, int ci, bool to_bf16, hipStream_t s);

// params: HOST array of n_params DEVICE pointers in table order -> blob
inline int us_pack_table(const ParamTable& t, const float* const* params, int n_params, void* blob, size_t blob_bytes,
                         uspace_stream_t stream) {
    if (!params || !blob || n_params != t.n_params) return USPACE_ERR_ARG;
    if (blob_bytes < t.bytes()) return USPACE_ERR_WORKSPACE;
    for (int i = 0; i < n_params; ++i)
        if (!params[i]) return USPACE_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    for (int i = 0; i < n_params; ++i) {
        const PDesc& d = t.p[i];
        char* dst = (char*)blob + d.offset;
        switch (d.kind) {
            case P_F32:
                if (hipMemcpyAsync(dst, params[i], d.bytes, hipMemcpyDeviceToDevice, s) != hipSuccess) return USPACE_ERR_LAUNCH;
                break;
            case P_BF16:
                US_TRY(uspace_cast_f32_bf16(params[i], (uint16_t*)dst, d.numel, stream));
                break;
            case P_CONV3_BF16:
            case P_CONV3_F32T:
                US_TRY(us_repack_conv3(params[i], dst, d.co, d.ci, d.kind == P_CONV3_BF16, s));
                break;
            case P_OWNER:
                break;
        }
    }
    return USPACE_OK;
}
