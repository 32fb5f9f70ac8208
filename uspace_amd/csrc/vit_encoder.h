// The transformer encoder of the three ViT towers outside U-ViT (pre-LN blocks, packed q|k|v projection with head_dim 64, GELU MLP),
// host side only: the shape constraints, a layer's offsets in the blob, its entries in a ParamTable in either published state_dict
// order, the four activation buffers of a workspace and the launch sequence of the layers.  clip.hip runs it causally over a prompt's
// L tokens, clip_vision.hip non-causally over patches + 1, both with quick-GELU; dino.hip non-causally with the erf-GELU and, on
// request, a copy of one layer's keys.  Embeddings, taps, final norm, pooling and projection stay with the towers (vit_embed.h).
#pragma once
#include <vector>

#include "blob.h"

// head_dim 64, K of every GEMM in 64s, the row kernels' width
inline bool vit_enc_valid(int dim, int heads, int layers, int ffn) {
    return dim > 0 && heads > 0 && layers >= 0 && ffn > 0 && dim == heads * 64 && !(dim & 63) && !(ffn & 63) && dim <= 4096;
}

struct VitEncLayer {
    size_t wqkv, bqkv, wo, bo, ln1g, ln1b, w1, b1, w2, b2, ln2g, ln2b;
    int i_wo, i_bo, i_ls1, i_w2, i_b2, i_ls2;   // parameter indices of the LayerScale fold (i_ls* = -1 without LayerScale)
};

// One layer's parameters (every linear and norm as weight, bias) in the order of a published state_dict:
//   VIT_ORDER_CLIP    HF CLIPEncoderLayer: self_attn.{k,v,q,out}_proj, layer_norm1, mlp.fc1, mlp.fc2, layer_norm2
//   VIT_ORDER_DINOV2  HF Dinov2Layer: norm1, attention.attention.{query,key,value}, attention.output.dense, [layer_scale1.lambda1],
//                     norm2, mlp.fc1, mlp.fc2, [layer_scale2.lambda1]; the lambdas are plain fp32 entries the forward never reads
enum VitOrder { VIT_ORDER_CLIP, VIT_ORDER_DINOV2 };
inline VitEncLayer vit_enc_add_layer(ParamTable& t, long D, long F, VitOrder order, bool layerscale) {
    const bool clip = order == VIT_ORDER_CLIP;
    VitEncLayer l;
    auto put_i = [&t](int& index, long numel, PKind k) { return t.at(index = t.add(numel, k)); };
    auto norm = [&](size_t& g, size_t& b) { g = t.put(D, P_F32); b = t.put(D, P_F32); };
    if (!clip) norm(l.ln1g, l.ln1b);
    // packed projection rows: q | k | v (the attention kernel's layout), HF Dinov2's order; HF CLIP lists k, v, q
    l.wqkv = t.arena.take(3 * D * D * 2);
    l.bqkv = t.arena.take(3 * D * 4);
    for (int j = 0; j < 3; ++j) {
        const int slot = clip ? (j + 1) % 3 : j;
        t.add_at(l.wqkv + slot * D * D * 2, D * D, P_BF16);
        t.add_at(l.bqkv + slot * D * 4, D, P_F32);
    }
    l.wo = put_i(l.i_wo, D * D, P_BF16);
    l.bo = put_i(l.i_bo, D, P_F32);
    l.i_ls1 = layerscale ? t.add(D, P_F32) : -1;
    norm(clip ? l.ln1g : l.ln2g, clip ? l.ln1b : l.ln2b);
    l.w1 = t.put(F * D, P_BF16);
    l.b1 = t.put(F, P_F32);
    l.w2 = put_i(l.i_w2, D * F, P_BF16);
    l.b2 = put_i(l.i_b2, D, P_F32);
    l.i_ls2 = layerscale ? t.add(D, P_F32) : -1;
    if (clip) norm(l.ln2g, l.ln2b);
    return l;
}

// the activations of a layer over M token rows, all bf16: LayerNorm output, q|k|v, attention output, fc1 output
struct VitEncWs {
    size_t h, qkv, att, f;
};
inline VitEncWs vit_enc_take_ws(Arena& a, size_t M, size_t D, size_t F) {
    return VitEncWs{a.take(M * D * 2), a.take(M * 3 * D * 2), a.take(M * D * 2), a.take(M * F * 2)};   // braces: taken left to right
}

// how a tower runs the layers: attention kind; quick-GELU as a launch of its own or the erf-GELU in fc1's epilogue
struct VitEncRun {
    int D, F, H;
    float eps;
    bool causal, erf_gelu;
};

// Layers [0, n) (at most every layer) over the fp32 residual stream x [B * L, D], in place: eight launches per layer with quick-GELU,
// seven with the erf-GELU.  key_layer in [0, n): the keys of that layer, as its q|k|v GEMM stored them, go to keys_out [B * L, D]
// between that GEMM and the attention.
inline int vit_enc_layers(const std::vector<VitEncLayer>& layers, int n, const VitEncRun& r, const void* blob, void* workspace,
                          const VitEncWs& w, float* x, int B, int L, int key_layer, uint16_t* keys_out, uspace_stream_t stream) {
    const char* wb = (const char*)blob;
    char* ws = (char*)workspace;
    const int D = r.D, F = r.F, M = B * L, all = (int)layers.size();
    uint16_t* h = (uint16_t*)(ws + w.h);
    uint16_t* qkv = (uint16_t*)(ws + w.qkv);
    uint16_t* att = (uint16_t*)(ws + w.att);
    uint16_t* f = (uint16_t*)(ws + w.f);
    auto PF = [&](size_t off) { return (const float*)(wb + off); };
    auto PH = [&](size_t off) { return (const uint16_t*)(wb + off); };
    constexpr int B_ = USPACE_EPI_BIAS, R_ = USPACE_EPI_RESIDUAL, F_ = USPACE_EPI_OUT_F32, H_ = USPACE_EPI_OUT_BF16;
    const int fc1_epi = B_ | H_ | (r.erf_gelu ? USPACE_EPI_GELU : 0);
    for (int i = 0; i < (n < all ? n : all); ++i) {
        const VitEncLayer& l = layers[i];
        US_TRY(uspace_layernorm_f32_bf16(x, PF(l.ln1g), PF(l.ln1b), h, M, D, r.eps, stream));
        US_TRY(uspace_gemm_bf16(h, D, nullptr, 0, D, PH(l.wqkv), D, M, 3 * D, D, B_ | H_, PF(l.bqkv), nullptr, 0, nullptr, 0, qkv,
                                3 * D, stream));
        if (i == key_layer && hipMemcpy2DAsync(keys_out, (size_t)D * 2, qkv + D, (size_t)3 * D * 2, (size_t)D * 2, M,
                                               hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess)
            return USPACE_ERR_LAUNCH;
        US_TRY(r.causal ? uspace_attention_causal_bf16(qkv, att, B, L, r.H, stream) : us_attention_any(qkv, nullptr, att, B, L, r.H, stream));
        US_TRY(uspace_gemm_bf16(att, D, nullptr, 0, D, PH(l.wo), D, M, D, D, B_ | R_ | F_, PF(l.bo), x, D, x, D, nullptr, 0, stream));
        US_TRY(uspace_layernorm_f32_bf16(x, PF(l.ln2g), PF(l.ln2b), h, M, D, r.eps, stream));
        US_TRY(uspace_gemm_bf16(h, D, nullptr, 0, D, PH(l.w1), D, M, F, D, fc1_epi, PF(l.b1), nullptr, 0, nullptr, 0, f, F, stream));
        if (!r.erf_gelu) US_TRY(uspace_quick_gelu_bf16(f, (long)M * F, stream));
        US_TRY(uspace_gemm_bf16(f, F, nullptr, 0, F, PH(l.w2), F, M, D, F, B_ | R_ | F_, PF(l.b2), x, D, x, D, nullptr, 0, stream));
    }
    return USPACE_OK;
}
