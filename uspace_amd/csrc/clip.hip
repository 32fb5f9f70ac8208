// CLIP text transformer (the encoder behind the reference's FrozenCLIPEmbedder, libs/clip.py:40-91: HF
// CLIPTextModel(input_ids).last_hidden_state) on the kernels of this library: token + position table lookup,
// the pre-LN blocks of vit_encoder.h (shared with clip_vision.hip and dino.hip) with CAUSAL attention, final LayerNorm.
// One-off per prompt on the sampling path; kept resident so repeated prompts cost one launch
// sequence instead of re-instantiating the encoder (tools/utils_t2i.py:25-39 does that on every call).
#include <vector>

#include "vit_encoder.h"

namespace {

// the table is the one statement of the parameter shapes and order; the offsets beside it are what the forward reads
struct ClipModel {
    ParamTable t;
    size_t tok, pos, fg, fb;
    std::vector<VitEncLayer> layers;
};

bool valid_clip(const uspace_clip_config* c) {
    if (!c || !vit_enc_valid(c->dim, c->heads, c->layers, c->ffn)) return false;
    return c->vocab > 0 && c->max_pos > 0 && c->max_pos <= 160;   // causal kernel: <= 10 key tiles
}

// HF state_dict order: embeddings.{token,position}_embedding.weight; the layers (vit_encoder.h); final_layer_norm.*
ClipModel build_clip(const uspace_clip_config& c) {
    ClipModel m;
    ParamTable& t = m.t;
    const long D = c.dim;
    m.tok = t.put((long)c.vocab * D, P_F32);
    m.pos = t.put((long)c.max_pos * D, P_F32);
    for (int i = 0; i < c.layers; ++i) m.layers.push_back(vit_enc_add_layer(t, D, c.ffn, VIT_ORDER_CLIP, false));
    m.fg = t.put(D, P_F32);
    m.fb = t.put(D, P_F32);
    return m;
}

struct ClipWs {
    size_t x;
    VitEncWs enc;
    size_t total;
};
ClipWs plan_clip_ws(const uspace_clip_config& c, int B) {
    ClipWs w;
    Arena a;
    const size_t M = (size_t)B * c.max_pos, D = c.dim;
    w.x = a.take(M * D * 4);
    w.enc = vit_enc_take_ws(a, M, D, (size_t)c.ffn);
    w.total = a.off;
    return w;
}

}  // namespace

extern "C" int uspace_clip_num_params(const uspace_clip_config* cfg) {
    return valid_clip(cfg) ? build_clip(*cfg).t.n_params : USPACE_ERR_ARG;
}

extern "C" long uspace_clip_param_numel(const uspace_clip_config* cfg, int index) {
    return valid_clip(cfg) ? build_clip(*cfg).t.numel(index) : (long)USPACE_ERR_ARG;
}

extern "C" size_t uspace_clip_weight_bytes(const uspace_clip_config* cfg) { return valid_clip(cfg) ? build_clip(*cfg).t.bytes() : 0; }

extern "C" size_t uspace_clip_workspace_bytes(const uspace_clip_config* cfg, int B) {
    return (valid_clip(cfg) && B > 0) ? plan_clip_ws(*cfg, B).total : 0;
}

extern "C" int uspace_clip_pack_weights(const uspace_clip_config* cfg, const float* const* params, int n_params, void* blob,
                                        size_t blob_bytes, uspace_stream_t stream) {
    if (!valid_clip(cfg)) return USPACE_ERR_ARG;
    return us_pack_table(build_clip(*cfg).t, params, n_params, blob, blob_bytes, stream);
}

extern "C" int uspace_clip_text_forward(const uspace_clip_config* cfg, const void* blob, void* workspace, size_t workspace_bytes,
                                        const int* ids, float* out, int B, int L, int stop_after_layer, uspace_stream_t stream) {
    if (!valid_clip(cfg) || !blob || !workspace || !ids || !out || B <= 0 || L <= 0 || L > cfg->max_pos) return USPACE_ERR_ARG;
    const ClipModel m = build_clip(*cfg);
    const ClipWs w = plan_clip_ws(*cfg, B);
    if (workspace_bytes < w.total) return USPACE_ERR_ARG;     // (the vision forward answers USPACE_ERR_WORKSPACE here)
    const char* wb = (const char*)blob;
    const int D = cfg->dim, M = B * L;
    float* x = (float*)((char*)workspace + w.x);
    auto PF = [&](size_t off) { return (const float*)(wb + off); };
    US_TRY(uspace_table_embed(ids, PF(m.tok), PF(m.pos), x, B, L, D, cfg->vocab, stream));
    // stop_after_layer: -1 = whole model incl. final norm; k >= 0: hidden state after k layers (0 = embeddings), no final norm
    const VitEncRun run = {D, cfg->ffn, cfg->heads, cfg->eps, /*causal=*/true, /*erf_gelu=*/false};
    const int n = stop_after_layer < 0 ? cfg->layers : stop_after_layer;
    US_TRY(vit_enc_layers(m.layers, n, run, blob, workspace, w.enc, x, B, L, -1, nullptr, stream));
    if (stop_after_layer >= 0) {
        if (hipMemcpyAsync(out, x, (size_t)M * D * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess) return USPACE_ERR_LAUNCH;
        return USPACE_OK;
    }
    return uspace_layernorm_f32(x, PF(m.fg), PF(m.fb), out, M, D, cfg->eps, stream);
}
