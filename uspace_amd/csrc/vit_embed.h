// The front of a ViT image tower, shared by clip_vision.hip and dino.hip: patch rows for the patch-embedding GEMM, the padded patch
// weight, class token + position table, and the gather of one token row; behind the kernels the host side of the front: the patch
// arithmetic and its validity, the padded patch weight in a ParamTable and its pack step, the workspace pieces, the embed sequence and
// the class token through a LayerNorm.  The layers between are vit_encoder.h.
#pragma once
#include "vit_encoder.h"

namespace {

// rows[b * N + gy * G + gx][k], k = (c, py, px) -> pixel_values[b, c, gy p + py, gx p + px] as bf16; columns K .. Kp - 1 are zero.
// One block per patch row.
__global__ __launch_bounds__(256) void patch_rows_kernel(const float* __restrict__ pv, bf16_t* __restrict__ rows, int S, int p, int G,
                                                         int K, int Kp) {
    const int row = blockIdx.x;
    const int N = G * G, b = row / N, i = row - b * N, gy = i / G, gx = i - gy * G;
    const int pp = p * p;
    bf16_t* dst = rows + (size_t)row * Kp;
    for (int k = threadIdx.x; k < Kp; k += 256) {
        float v = 0.0f;
        if (k < K) {
            const int c = k / pp, r = k - c * pp, py = r / p, px = r - py * p;
            v = pv[((size_t)(b * 3 + c) * S + gy * p + py) * S + gx * p + px];
        }
        dst[k] = f2bf(v);
    }
}

// x[b, 0] = cls + pos[0];  x[b, 1 + i] = patch[b, i] + pos[1 + i]  (HF CLIPVisionEmbeddings); one block per token row, fp32
__global__ __launch_bounds__(256) void assemble_tokens_kernel(const float* __restrict__ patch, const float* __restrict__ cls,
                                                              const float* __restrict__ pos, float* __restrict__ x, int T, int D) {
    const int row = blockIdx.x, b = row / T, t = row - b * T;
    const float* a = t == 0 ? cls : patch + ((size_t)b * (T - 1) + (t - 1)) * D;
    const float* pr = pos + (size_t)t * D;
    for (int d = threadIdx.x * 4; d < D; d += 1024) *(f32x4*)(x + (size_t)row * D + d) = *(const f32x4*)(a + d) + *(const f32x4*)(pr + d);
}

// out[b, :] = x[b, idx[b], :] of x [B, L, D]; idx == NULL: row 0 (the class token).  One block per sample; an index outside
// [0, L) is clamped (validated on the host).
__global__ __launch_bounds__(256) void gather_rows_kernel(const float* __restrict__ x, const int* __restrict__ idx, float* __restrict__ out,
                                                          int L, int D) {
    const int b = blockIdx.x;
    int r = idx ? idx[b] : 0;
    r = r < 0 ? 0 : (r >= L ? L - 1 : r);
    const float* src = x + ((size_t)b * L + r) * D;
    for (int d = threadIdx.x; d < D; d += 256) out[(size_t)b * D + d] = src[d];
}

// bf16 [D, K] dense (the staging area behind the table) -> [D, Kp] with zero pad columns (the table's region); one block per row
__global__ __launch_bounds__(256) void pad_patch_rows_kernel(const bf16_t* __restrict__ dense, bf16_t* __restrict__ padded, int K, int Kp) {
    const int d = blockIdx.x;
    for (int k = threadIdx.x; k < Kp; k += 256) padded[(size_t)d * Kp + k] = k < K ? dense[(size_t)d * K + k] : (bf16_t)0;
}

// ------------------------------------------------------------------------------------------------------------- host side
bool vit_patch_valid(int image, int patch) { return image > 0 && patch > 0 && image % patch == 0 && image <= 4096 && patch <= 256; }

// the patch grid of a tower's config (its fields image, patch, dim)
struct VitPatch {
    int image, patch, dim;
    int k() const { return 3 * patch * patch; }      // a patch row: (c, py, px)
    int kp() const { return (k() + 63) / 64 * 64; }   // ... padded to whole 64-value k steps of the GEMM
    int grid() const { return image / patch; }
    int n() const { return grid() * grid(); }
    int tokens() const { return n() + 1; }
};
template <class Config>
VitPatch vit_patch(const Config& c) { return VitPatch{c.image, c.patch, c.dim}; }

// patch weight [D, K] fp32 -> bf16 [D, Kp]: the table's cast is dense, so the pack step sends it to a staging area behind the table (one
// bf16 [D, K] copy: what a tower's weight_bytes adds to its table) and spreads it to the Kp-wide region with zero pad columns
struct VitPatchWeight {
    size_t offset;
    int index;
};
VitPatchWeight vit_patch_add_weight(ParamTable& t, const VitPatch& g) {
    const size_t offset = t.arena.take((size_t)g.dim * g.kp() * 2);
    return VitPatchWeight{offset, t.add_at(offset, (long)g.dim * g.k(), P_BF16)};
}
size_t vit_patch_stage_bytes(const VitPatch& g) { return us_align_up((size_t)g.dim * g.k() * 2); }
int vit_pack_table(ParamTable& t, const VitPatch& g, const VitPatchWeight& pw, const float* const* params, int n_params, void* blob,
                   size_t blob_bytes, uspace_stream_t stream) {
    const size_t stage = t.bytes();
    if (blob && blob_bytes < stage + vit_patch_stage_bytes(g)) return USPACE_ERR_WORKSPACE;
    t.p[pw.index].offset = stage;
    US_TRY(us_pack_table(t, params, n_params, blob, blob_bytes, stream));
    hipLaunchKernelGGL(pad_patch_rows_kernel, dim3(g.dim), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)((char*)blob + stage),
                       (bf16_t*)((char*)blob + pw.offset), g.k(), g.kp());
    US_CHECK_LAUNCH();
    return USPACE_OK;
}

// a tower's workspace behind its residual stream: fp32 patch embeddings, bf16 patch rows, the encoder's activations, the class-token row
struct VitTowerWs {
    size_t pe, rows;
    VitEncWs enc;
    size_t tok0;
};
VitTowerWs vit_tower_take_ws(Arena& a, const VitPatch& g, size_t B, size_t F) {
    const size_t N = g.n(), D = g.dim;   // braces: taken left to right
    return VitTowerWs{a.take(B * N * D * 4), a.take(B * N * g.kp() * 2), vit_enc_take_ws(a, B * (N + 1), D, F), a.take(B * D * 4)};
}

// pixel_values -> x [B, tokens, D] fp32 in three launches: patch rows, patch GEMM (patch_b NULL: no bias), class token + position table
int vit_embed(const VitPatch& g, const uint16_t* patch_w, const float* patch_b, const float* cls, const float* pos, void* workspace,
              const VitTowerWs& w, const float* pixel_values, float* x, int B, uspace_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    const int D = g.dim, N = g.n(), K = g.k(), Kp = g.kp();
    float* pe = (float*)((char*)workspace + w.pe);
    uint16_t* rows = (uint16_t*)((char*)workspace + w.rows);
    hipLaunchKernelGGL(patch_rows_kernel, dim3(B * N), dim3(256), 0, s, pixel_values, rows, g.image, g.patch, g.grid(), K, Kp);
    US_CHECK_LAUNCH();
    US_TRY(uspace_gemm_bf16(rows, Kp, nullptr, 0, Kp, patch_w, Kp, B * N, D, Kp, (patch_b ? USPACE_EPI_BIAS : 0) | USPACE_EPI_OUT_F32,
                            patch_b, nullptr, 0, pe, D, nullptr, 0, stream));
    hipLaunchKernelGGL(assemble_tokens_kernel, dim3(B * (N + 1)), dim3(256), 0, s, pe, cls, pos, x, N + 1, D);
    US_CHECK_LAUNCH();
    return USPACE_OK;
}

// out [B, D] = LayerNorm(x[:, 0]) of x [B, T, D]: the class token through a tower's last norm
int vit_class_token_norm(const float* x, void* workspace, const VitTowerWs& w, const float* gamma, const float* beta, float* out, int B,
                         int T, int D, float eps, uspace_stream_t stream) {
    float* tok0 = (float*)((char*)workspace + w.tok0);
    hipLaunchKernelGGL(gather_rows_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, x, (const int*)nullptr, tok0, T, D);
    US_CHECK_LAUNCH();
    return uspace_layernorm_f32(tok0, gamma, beta, out, B, D, eps, stream);
}

}  // namespace
