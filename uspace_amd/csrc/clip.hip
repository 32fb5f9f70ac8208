// CLIP text transformer (the encoder behind the reference's FrozenCLIPEmbedder, libs/clip.py:40-91: HF
// CLIPTextModel(input_ids).last_hidden_state) on the kernels of this library: token + position table lookup,
// pre-LN blocks with CAUSAL attention (packed q|k|v projection, head_dim 64) and a quick-GELU MLP, final LayerNorm.
// One-off per prompt on the sampling path; kept resident so repeated prompts cost one launch
// sequence instead of re-instantiating the encoder (tools/utils_t2i.py:25-39 does that on every call).
#include <vector>

#include "blob.h"

namespace {

struct ClipLayer {
    size_t wqkv, bqkv, wo, bo, ln1g, ln1b, w1, b1, w2, b2, ln2g, ln2b;
};
// the table is the one statement of the parameter shapes and order; the offsets beside it are what the forward reads
struct ClipModel {
    ParamTable t;
    size_t tok, pos, fg, fb;
    std::vector<ClipLayer> layers;
};

bool valid_clip(const uspace_clip_config* c) {
    if (!c || c->vocab <= 0 || c->dim <= 0 || c->heads <= 0 || c->layers < 0 || c->ffn <= 0 || c->max_pos <= 0) return false;
    if (c->dim != c->heads * 64 || (c->dim & 63) || (c->ffn & 63) || c->dim > 4096) return false;   // head_dim 64, K % 64
    if (c->max_pos > 160) return false;                                                              // causal kernel: <= 10 key tiles
    return true;
}

// HF state_dict order: embeddings.{token,position}_embedding.weight; per layer self_attn.{k,v,q,out}_proj.{weight,bias},
// layer_norm1.{weight,bias}, mlp.fc1.{weight,bias}, mlp.fc2.{weight,bias}, layer_norm2.{weight,bias}; final_layer_norm.*
ClipModel build_clip(const uspace_clip_config& c) {
    ClipModel m;
    ParamTable& t = m.t;
    auto put = [&t](long numel, PKind k) { return t.at(t.add(numel, k)); };
    const long D = c.dim, F = c.ffn;
    m.tok = put((long)c.vocab * D, P_F32);
    m.pos = put((long)c.max_pos * D, P_F32);
    for (int i = 0; i < c.layers; ++i) {
        ClipLayer l;
        // packed projection rows: q | k | v (the attention kernel's layout); HF lists k, v, q
        l.wqkv = t.arena.take(3 * D * D * 2);
        l.bqkv = t.arena.take(3 * D * 4);
        for (const int slot : {1, 2, 0}) {
            t.add_at(l.wqkv + slot * D * D * 2, D * D, P_BF16);
            t.add_at(l.bqkv + slot * D * 4, D, P_F32);
        }
        l.wo = put(D * D, P_BF16);
        l.bo = put(D, P_F32);
        l.ln1g = put(D, P_F32);
        l.ln1b = put(D, P_F32);
        l.w1 = put(F * D, P_BF16);
        l.b1 = put(F, P_F32);
        l.w2 = put(D * F, P_BF16);
        l.b2 = put(D, P_F32);
        l.ln2g = put(D, P_F32);
        l.ln2b = put(D, P_F32);
        m.layers.push_back(l);
    }
    m.fg = put(D, P_F32);
    m.fb = put(D, P_F32);
    return m;
}

struct ClipWs {
    size_t x, h, qkv, att, f, total;
};
ClipWs plan_clip_ws(const uspace_clip_config& c, int B) {
    ClipWs w;
    Arena a;
    const size_t M = (size_t)B * c.max_pos, D = c.dim;
    w.x = a.take(M * D * 4);
    w.h = a.take(M * D * 2);
    w.qkv = a.take(M * 3 * D * 2);
    w.att = a.take(M * D * 2);
    w.f = a.take(M * (size_t)c.ffn * 2);
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
    if (workspace_bytes < w.total) return USPACE_ERR_ARG;
    const char* wb = (const char*)blob;
    char* ws = (char*)workspace;
    const int D = cfg->dim, F = cfg->ffn, H = cfg->heads, M = B * L;
    float* x = (float*)(ws + w.x);
    uint16_t* h = (uint16_t*)(ws + w.h);
    uint16_t* qkv = (uint16_t*)(ws + w.qkv);
    uint16_t* att = (uint16_t*)(ws + w.att);
    uint16_t* f = (uint16_t*)(ws + w.f);
    auto PF = [&](size_t off) { return (const float*)(wb + off); };
    auto PH = [&](size_t off) { return (const uint16_t*)(wb + off); };
    constexpr int B_ = USPACE_EPI_BIAS, R_ = USPACE_EPI_RESIDUAL, F_ = USPACE_EPI_OUT_F32, H_ = USPACE_EPI_OUT_BF16;
    US_TRY(uspace_table_embed(ids, PF(m.tok), PF(m.pos), x, B, L, D, cfg->vocab, stream));
    // stop_after_layer: -1 = whole model incl. final norm; k >= 0: hidden state after k layers (0 = embeddings), no final norm
    const int n_layers = stop_after_layer < 0 ? cfg->layers : (stop_after_layer < cfg->layers ? stop_after_layer : cfg->layers);
    for (int i = 0; i < n_layers; ++i) {
        const ClipLayer& l = m.layers[i];
        US_TRY(uspace_layernorm_f32_bf16(x, PF(l.ln1g), PF(l.ln1b), h, M, D, cfg->eps, stream));
        US_TRY(uspace_gemm_bf16(h, D, nullptr, 0, D, PH(l.wqkv), D, M, 3 * D, D, B_ | H_, PF(l.bqkv), nullptr, 0, nullptr, 0, qkv,
                                3 * D, stream));
        US_TRY(uspace_attention_causal_bf16(qkv, att, B, L, H, stream));
        US_TRY(uspace_gemm_bf16(att, D, nullptr, 0, D, PH(l.wo), D, M, D, D, B_ | R_ | F_, PF(l.bo), x, D, x, D, nullptr, 0, stream));
        US_TRY(uspace_layernorm_f32_bf16(x, PF(l.ln2g), PF(l.ln2b), h, M, D, cfg->eps, stream));
        US_TRY(uspace_gemm_bf16(h, D, nullptr, 0, D, PH(l.w1), D, M, F, D, B_ | H_, PF(l.b1), nullptr, 0, nullptr, 0, f, F, stream));
        US_TRY(uspace_quick_gelu_bf16(f, (long)M * F, stream));
        US_TRY(uspace_gemm_bf16(f, F, nullptr, 0, F, PH(l.w2), F, M, D, F, B_ | R_ | F_, PF(l.b2), x, D, x, D, nullptr, 0, stream));
    }
    if (stop_after_layer >= 0) {
        if (hipMemcpyAsync(out, x, (size_t)M * D * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess) return USPACE_ERR_LAUNCH;
        return USPACE_OK;
    }
    return uspace_layernorm_f32(x, PF(m.fg), PF(m.fb), out, M, D, cfg->eps, stream);
}
