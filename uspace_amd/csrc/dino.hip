// The DINO image towers (HF Dinov2Model; with layerscale = 0 a plain pre-LN ViT such as HF ViTModel / DINO v1) and the structure
// distance of an edit.  The tower runs through the two headers it shares with the CLIP towers: the front of vit_embed.h (patch rows ->
// the patch GEMM with the patch bias, class token + position table; the padded patch weight; the final LayerNorm of the class token)
// and the layers of vit_encoder.h (LN1 -> q|k|v -> non-causal attention -> out projection (+ residual) -> LN2 -> fc1 with the erf-GELU
// epilogue -> fc2 (+ residual): seven launches, and the copy of one layer's keys).  LayerScale is folded into the out projection and
// fc2 when the blob is packed: W' = bf16(lambda[n] W[n, k]) from the fp32 checkpoint values (one rounding), b' = lambda[n] b[n]; the
// forward never sees lambda.  The position table arrives already interpolated to image / patch (the host does that once, in torch).
// The structure distance compares the cosine self-similarity matrices of two key sets tile by tile on the bf16 matrix cores; neither
// T x T matrix is stored, and every sum has one fixed order (no atomics).
#include <vector>

#include "vit_embed.h"
#include "vit_encoder.h"

namespace {

// ------------------------------------------------------------------------------------------------------------- the model
struct DModel {
    ParamTable t;
    size_t cls, pos, patchb, ng, nb;
    VitPatchWeight patch;
    std::vector<VitEncLayer> layers;
};

bool valid_dino(const uspace_dino_config* c) {
    if (!c || !vit_enc_valid(c->dim, c->heads, c->layers, c->ffn) || !vit_patch_valid(c->image, c->patch)) return false;
    return c->layerscale == 0 || c->layerscale == 1;
}

// HF Dinov2Model.state_dict() order without mask_token (see the header)
DModel build_dino(const uspace_dino_config& c) {
    DModel m;
    ParamTable& t = m.t;
    const VitPatch g = vit_patch(c);
    const long D = c.dim;
    m.cls = t.put(D, P_F32);
    m.pos = t.put((long)g.tokens() * D, P_F32);
    m.patch = vit_patch_add_weight(t, g);
    m.patchb = t.put(D, P_F32);
    for (int i = 0; i < c.layers; ++i) m.layers.push_back(vit_enc_add_layer(t, D, c.ffn, VIT_ORDER_DINOV2, c.layerscale != 0));
    m.ng = t.put(D, P_F32);
    m.nb = t.put(D, P_F32);
    return m;
}

// LayerScale folded into a branch's last linear: Wd[n, k] = bf16(lam[n] W[n, k]), bd[n] = lam[n] b[n]; one block per output row
__global__ __launch_bounds__(256) void fold_layerscale_kernel(const float* __restrict__ W, const float* __restrict__ b,
                                                              const float* __restrict__ lam, bf16_t* __restrict__ Wd,
                                                              float* __restrict__ bd, int K) {
    const int n = blockIdx.x;
    const float l = lam[n];
    for (int k = threadIdx.x; k < K; k += 256) Wd[(size_t)n * K + k] = f2bf(l * W[(size_t)n * K + k]);
    if (threadIdx.x == 0) bd[n] = l * b[n];
}

struct DWs {
    size_t x;
    VitTowerWs vit;
    size_t total;
};
DWs plan_dino_ws(const uspace_dino_config& c, int B) {
    DWs w;
    Arena a;
    const VitPatch g = vit_patch(c);
    w.x = a.take((size_t)B * g.tokens() * c.dim * 4);
    w.vit = vit_tower_take_ws(a, g, (size_t)B, (size_t)c.ffn);
    w.total = a.off;
    return w;
}

// ------------------------------------------------------------------------------------------------------------- structure distance
// norms[(p * 2 + which) * T + t] = |k_t| of member `which` (0: a, 1: b) of pair p: fp32 sum of squares of the stored bf16 keys, one
// wave per row, lanes over 8-value pieces, then the wave's fixed reduction
__global__ __launch_bounds__(256) void key_norms_kernel(const bf16_t* __restrict__ ka, const bf16_t* __restrict__ kb,
                                                        float* __restrict__ norms, int T, int D, long ld, long pair_stride) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= T) return;
    const int which = blockIdx.y, p = blockIdx.z;
    const bf16_t* src = (which ? kb : ka) + (size_t)p * pair_stride + (size_t)row * ld;
    float acc = 0.0f;
    for (int d = lane * 8; d < D; d += 512) {
        const bf16x8 v = *(const bf16x8*)(src + d);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc = fmaf((float)v[j], (float)v[j], acc);
    }
    acc = wave_sum(acc);
    if (lane == 0) norms[((size_t)p * 2 + which) * T + row] = sqrtf(acc);
}

// One wave per 16 x 16 tile (ti, tj) of a pair: both Gram tiles by v_mfma_f32_16x16x32_bf16 straight from global memory (the
// fragment layout of attention_map.hip: a lane holds 8 consecutive k of row lane & 15 for each operand and, of the result, rows
// 4 (lane >> 4) + 0..3 of column lane & 15), the cosine normalisation after the product, the squared difference summed over the
// lane's four values and then over the wave.  Rows beyond T read row T - 1 again and count as 0.
__global__ __launch_bounds__(256) void self_sim_tiles_kernel(const bf16_t* __restrict__ ka, const bf16_t* __restrict__ kb,
                                                             const float* __restrict__ norms, float* __restrict__ partial, int T,
                                                             int D, long ld, long pair_stride, int nt) {
    const int lane = threadIdx.x & 63, fr = lane & 15, fq = lane >> 4;
    const int tile = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile >= nt * nt) return;
    const int ti = tile / nt, tj = tile - ti * nt, p = blockIdx.y;
    const int ri = min(ti * 16 + fr, T - 1), rj = min(tj * 16 + fr, T - 1);
    const bf16_t* a0 = ka + (size_t)p * pair_stride;
    const bf16_t* b0 = kb + (size_t)p * pair_stride;
    const bf16_t* ai = a0 + (size_t)ri * ld + fq * 8;
    const bf16_t* aj = a0 + (size_t)rj * ld + fq * 8;
    const bf16_t* bi = b0 + (size_t)ri * ld + fq * 8;
    const bf16_t* bj = b0 + (size_t)rj * ld + fq * 8;
    f32x4 sa = (f32x4){0.f, 0.f, 0.f, 0.f}, sb = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < D; k += 32) {
        sa = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8*)(ai + k), *(const bf16x8*)(aj + k), sa, 0, 0, 0);
        sb = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8*)(bi + k), *(const bf16x8*)(bj + k), sb, 0, 0, 0);
    }
    const float* na = norms + (size_t)p * 2 * T;
    const float* nb = na + T;
    const int col = tj * 16 + fr;
    const float naj = na[rj], nbj = nb[rj];
    float sum = 0.0f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = ti * 16 + fq * 4 + r, rc = min(row, T - 1);
        const float d = sa[r] / fmaxf(na[rc] * naj, 1e-8f) - sb[r] / fmaxf(nb[rc] * nbj, 1e-8f);
        if (row < T && col < T) sum = fmaf(d, d, sum);
    }
    sum = wave_sum(sum);
    if (lane == 0) partial[(size_t)p * nt * nt + tile] = sum;
}

// out[p] = (sum of the pair's n tile sums) / T^2 in fp64: thread t adds tiles t, t + 256, ... in order, then a fixed tree
__global__ __launch_bounds__(256) void self_sim_finish_kernel(const float* __restrict__ partial, double* __restrict__ out, int n,
                                                              double tt) {
    __shared__ double red[256];
    const int p = blockIdx.x, tid = threadIdx.x;
    const float* src = partial + (size_t)p * n;
    double acc = 0.0;
    for (int i = tid; i < n; i += 256) acc += (double)src[i];
    red[tid] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid == 0) out[p] = red[0] / tt;
}

constexpr int SS_MAX_T = 16384;   // 1024 x 1024 tiles per pair

struct SsWs {
    size_t norms, partial, total;
};
SsWs plan_ss_ws(int P, int T) {
    SsWs w;
    Arena a;
    const size_t nt = (T + 15) / 16;
    w.norms = a.take((size_t)P * 2 * T * 4);
    w.partial = a.take((size_t)P * nt * nt * 4);
    w.total = a.off;
    return w;
}

}  // namespace

extern "C" int uspace_dino_num_params(const uspace_dino_config* cfg) {
    return valid_dino(cfg) ? build_dino(*cfg).t.n_params : USPACE_ERR_ARG;
}

extern "C" long uspace_dino_param_numel(const uspace_dino_config* cfg, int index) {
    return valid_dino(cfg) ? build_dino(*cfg).t.numel(index) : (long)USPACE_ERR_ARG;
}

extern "C" size_t uspace_dino_weight_bytes(const uspace_dino_config* cfg) {
    // + the staging area of the patch weight's pad step behind the table
    return valid_dino(cfg) ? build_dino(*cfg).t.bytes() + vit_patch_stage_bytes(vit_patch(*cfg)) : 0;
}

extern "C" size_t uspace_dino_workspace_bytes(const uspace_dino_config* cfg, int B) {
    return (valid_dino(cfg) && B > 0) ? plan_dino_ws(*cfg, B).total : 0;
}

extern "C" int uspace_dino_pack_weights(const uspace_dino_config* cfg, const float* const* params, int n_params, void* blob,
                                        size_t blob_bytes, uspace_stream_t stream) {
    if (!valid_dino(cfg)) return USPACE_ERR_ARG;
    DModel m = build_dino(*cfg);
    hipStream_t s = (hipStream_t)stream;
    const int D = cfg->dim, F = cfg->ffn;
    US_TRY(vit_pack_table(m.t, vit_patch(*cfg), m.patch, params, n_params, blob, blob_bytes, stream));
    char* wb = (char*)blob;
    if (cfg->layerscale) {
        // over the plain casts the table loop just made: the branch's last linear with lambda folded in, from the fp32 values
        for (const VitEncLayer& l : m.layers) {
            hipLaunchKernelGGL(fold_layerscale_kernel, dim3(D), dim3(256), 0, s, params[l.i_wo], params[l.i_bo], params[l.i_ls1],
                               (bf16_t*)(wb + l.wo), (float*)(wb + l.bo), D);
            US_CHECK_LAUNCH();
            hipLaunchKernelGGL(fold_layerscale_kernel, dim3(D), dim3(256), 0, s, params[l.i_w2], params[l.i_b2], params[l.i_ls2],
                               (bf16_t*)(wb + l.w2), (float*)(wb + l.b2), F);
            US_CHECK_LAUNCH();
        }
    }
    return USPACE_OK;
}

extern "C" int uspace_dino_forward(const uspace_dino_config* cfg, const void* blob, void* workspace, size_t workspace_bytes,
                                   const float* pixel_values, float* pooler_output, int B, int stop_after_layer, float* tap_out,
                                   int key_layer, uint16_t* keys_out, uspace_stream_t stream) {
    if (!valid_dino(cfg) || !blob || !workspace || !pixel_values || B <= 0) return USPACE_ERR_ARG;
    const bool stopped = stop_after_layer != -1;
    if (stop_after_layer < -2) return USPACE_ERR_ARG;
    const int n_run = stop_after_layer == -1 ? cfg->layers : (stop_after_layer == -2 ? 0 : min(stop_after_layer, cfg->layers));
    const bool want_keys = key_layer >= 0;
    if (want_keys && (!keys_out || key_layer >= n_run)) return USPACE_ERR_ARG;
    if (key_layer < -1) return USPACE_ERR_ARG;
    // something must come out: the pooled class token of the whole model, a tap of a stopped run, or keys
    if (stopped ? (!tap_out && !want_keys) : (!pooler_output && !want_keys)) return USPACE_ERR_ARG;
    const DModel m = build_dino(*cfg);
    const DWs w = plan_dino_ws(*cfg, B);
    if (workspace_bytes < w.total) return USPACE_ERR_WORKSPACE;
    const char* wb = (const char*)blob;
    const VitPatch g = vit_patch(*cfg);
    const int D = cfg->dim, T = g.tokens();
    float* x = (float*)((char*)workspace + w.x);
    auto PF = [&](size_t off) { return (const float*)(wb + off); };

    US_TRY(vit_embed(g, (const uint16_t*)(wb + m.patch.offset), PF(m.patchb), PF(m.cls), PF(m.pos), workspace, w.vit, pixel_values, x, B,
                     stream));
    const VitEncRun run = {D, cfg->ffn, cfg->heads, cfg->eps, /*causal=*/false, /*erf_gelu=*/true};
    US_TRY(vit_enc_layers(m.layers, n_run, run, blob, workspace, w.vit.enc, x, B, T, key_layer, keys_out, stream));
    if (stopped) {
        if (tap_out && hipMemcpyAsync(tap_out, x, (size_t)B * T * D * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess)
            return USPACE_ERR_LAUNCH;
        return USPACE_OK;
    }
    if (!pooler_output) return USPACE_OK;
    return vit_class_token_norm(x, workspace, w.vit, PF(m.ng), PF(m.nb), pooler_output, B, T, D, cfg->eps, stream);
}

extern "C" size_t uspace_self_similarity_mse_workspace_bytes(int P, int T) {
    return (P > 0 && P <= 65535 && T > 0 && T <= SS_MAX_T) ? plan_ss_ws(P, T).total : 0;
}

extern "C" int uspace_self_similarity_mse_f64(const uint16_t* keys_a, const uint16_t* keys_b, int P, int T, int D, long row_stride,
                                              long pair_stride, void* workspace, size_t workspace_bytes, double* out,
                                              uspace_stream_t stream) {
    if (!keys_a || !keys_b || !workspace || !out || P <= 0 || P > 65535 || T <= 0 || T > SS_MAX_T) return USPACE_ERR_ARG;
    // 16-byte fragment loads: D in whole 64-value k steps, rows and pairs on 8-value boundaries
    if (D <= 0 || (D & 63) || row_stride < D || (row_stride & 7) || pair_stride < 0 || (pair_stride & 7)) return USPACE_ERR_ARG;
    if (((uintptr_t)keys_a | (uintptr_t)keys_b) & 15) return USPACE_ERR_ARG;
    const SsWs w = plan_ss_ws(P, T);
    if (workspace_bytes < w.total) return USPACE_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    float* norms = (float*)((char*)workspace + w.norms);
    float* partial = (float*)((char*)workspace + w.partial);
    const int nt = (T + 15) / 16;
    hipLaunchKernelGGL(key_norms_kernel, dim3(us_cdiv(T, 4), 2, P), dim3(256), 0, s, keys_a, keys_b, norms, T, D, row_stride,
                       pair_stride);
    US_CHECK_LAUNCH();
    hipLaunchKernelGGL(self_sim_tiles_kernel, dim3(us_cdiv(nt * nt, 4), P), dim3(256), 0, s, keys_a, keys_b, (const float*)norms, partial,
                       T, D, row_stride, pair_stride, nt);
    US_CHECK_LAUNCH();
    hipLaunchKernelGGL(self_sim_finish_kernel, dim3(P), dim3(256), 0, s, (const float*)partial, out, nt * nt, (double)T * (double)T);
    US_CHECK_LAUNCH();
    return USPACE_OK;
}
