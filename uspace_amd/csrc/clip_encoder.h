// The transformer encoder of both CLIP towers (HF CLIPEncoder: pre-LN blocks, packed q|k|v projection with head_dim 64, quick-GELU
// MLP), host side only: a layer's offsets in the blob, its entries in a ParamTable, the four activation buffers of a workspace and the
// launch sequence of the layers.  clip.hip runs it causally over the L tokens of a prompt, clip_vision.hip non-causally over patches + 1;
// embeddings, taps, final norm, pooling and projection stay with the towers.
#pragma once
#include <vector>

#include "blob.h"

struct ClipEncLayer {
    size_t wqkv, bqkv, wo, bo, ln1g, ln1b, w1, b1, w2, b2, ln2g, ln2b;
};

// One layer's parameters in HF state_dict order: self_attn.{k,v,q,out}_proj.{weight,bias}, layer_norm1.{weight,bias},
// mlp.fc1.{weight,bias}, mlp.fc2.{weight,bias}, layer_norm2.{weight,bias}
inline ClipEncLayer clip_enc_add_layer(ParamTable& t, long D, long F) {
    auto put = [&t](long numel, PKind k) { return t.at(t.add(numel, k)); };
    ClipEncLayer l;
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
    return l;
}

// the activations of a layer over M token rows, all bf16: LayerNorm output, q|k|v, attention output, fc1 output
struct ClipEncWs {
    size_t h, qkv, att, f;
};
inline ClipEncWs clip_enc_take_ws(Arena& a, size_t M, size_t D, size_t F) {
    ClipEncWs w;
    w.h = a.take(M * D * 2);
    w.qkv = a.take(M * 3 * D * 2);
    w.att = a.take(M * D * 2);
    w.f = a.take(M * F * 2);
    return w;
}

// Layers [0, n) over the fp32 residual stream x [B * L, D], in place.  stop_after_layer < 0: n = every layer; k >= 0: n = k, at most
// every layer (the towers' taps).  Eight launches per layer.
inline int clip_enc_layers(const std::vector<ClipEncLayer>& layers, int stop_after_layer, const void* blob, void* workspace,
                           const ClipEncWs& w, float* x, int B, int L, int D, int F, int H, float eps, bool causal,
                           uspace_stream_t stream) {
    const char* wb = (const char*)blob;
    char* ws = (char*)workspace;
    const int M = B * L, all = (int)layers.size();
    uint16_t* h = (uint16_t*)(ws + w.h);
    uint16_t* qkv = (uint16_t*)(ws + w.qkv);
    uint16_t* att = (uint16_t*)(ws + w.att);
    uint16_t* f = (uint16_t*)(ws + w.f);
    auto PF = [&](size_t off) { return (const float*)(wb + off); };
    auto PH = [&](size_t off) { return (const uint16_t*)(wb + off); };
    constexpr int B_ = USPACE_EPI_BIAS, R_ = USPACE_EPI_RESIDUAL, F_ = USPACE_EPI_OUT_F32, H_ = USPACE_EPI_OUT_BF16;
    const int n_layers = stop_after_layer < 0 ? all : (stop_after_layer < all ? stop_after_layer : all);
    for (int i = 0; i < n_layers; ++i) {
        const ClipEncLayer& l = layers[i];
        US_TRY(uspace_layernorm_f32_bf16(x, PF(l.ln1g), PF(l.ln1b), h, M, D, eps, stream));
        US_TRY(uspace_gemm_bf16(h, D, nullptr, 0, D, PH(l.wqkv), D, M, 3 * D, D, B_ | H_, PF(l.bqkv), nullptr, 0, nullptr, 0, qkv,
                                3 * D, stream));
        US_TRY(causal ? uspace_attention_causal_bf16(qkv, att, B, L, H, stream) : us_attention_any(qkv, nullptr, att, B, L, H, stream));
        US_TRY(uspace_gemm_bf16(att, D, nullptr, 0, D, PH(l.wo), D, M, D, D, B_ | R_ | F_, PF(l.bo), x, D, x, D, nullptr, 0, stream));
        US_TRY(uspace_layernorm_f32_bf16(x, PF(l.ln2g), PF(l.ln2b), h, M, D, eps, stream));
        US_TRY(uspace_gemm_bf16(h, D, nullptr, 0, D, PH(l.w1), D, M, F, D, B_ | H_, PF(l.b1), nullptr, 0, nullptr, 0, f, F, stream));
        US_TRY(uspace_quick_gelu_bf16(f, (long)M * F, stream));
        US_TRY(uspace_gemm_bf16(f, F, nullptr, 0, F, PH(l.w2), F, M, D, F, B_ | R_ | F_, PF(l.b2), x, D, x, D, nullptr, 0, stream));
    }
    return USPACE_OK;
}
