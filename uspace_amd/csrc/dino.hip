// The DINO image towers (HF Dinov2Model; with layerscale = 0 a plain pre-LN ViT such as HF ViTModel / DINO v1) and the structure
// distance of an edit.  The tower runs on the kernels of this library: patch rows -> uspace_gemm_bf16 with the patch bias, class token
// + position table (vit_embed.h, shared with clip_vision.hip), then per layer LN1 -> q|k|v -> non-causal attention -> out projection
// (+ residual) -> LN2 -> fc1 with the erf-GELU epilogue -> fc2 (+ residual): seven launches, and the final LayerNorm of the class
// token.  LayerScale is folded into the out projection and fc2 when the blob is packed: W' = bf16(lambda[n] W[n, k]) from the fp32
// checkpoint values (one rounding), b' = lambda[n] b[n]; the forward never sees lambda.  The position table arrives already
// interpolated to image / patch (the host does that once, in torch).
// The structure distance compares the cosine self-similarity matrices of two key sets tile by tile on the bf16 matrix cores; neither
// T x T matrix is stored, and every sum has one fixed order (no atomics).
#include <vector>

#include "clip_encoder.h"
#include "vit_embed.h"

namespace {

// ------------------------------------------------------------------------------------------------------------- the model
struct DinoLayer {
    size_t ln1g, ln1b, wqkv, bqkv, wo, bo, ln2g, ln2b, w1, b1, w2, b2;
    int i_wo, i_bo, i_ls1, i_w2, i_b2, i_ls2;   // parameter indices of the LayerScale fold (i_ls* = -1 without LayerScale)
};

struct DModel {
    ParamTable t;
    size_t cls, pos, patch, patchb, ng, nb;
    int i_patch;
    std::vector<DinoLayer> layers;
};

int patch_k(const uspace_dino_config& c) { return 3 * c.patch * c.patch; }
int patch_kp(const uspace_dino_config& c) { return (patch_k(c) + 63) / 64 * 64; }
int n_patches(const uspace_dino_config& c) { return (c.image / c.patch) * (c.image / c.patch); }

bool valid_dino(const uspace_dino_config* c) {
    if (!c || c->image <= 0 || c->patch <= 0 || c->dim <= 0 || c->heads <= 0 || c->layers < 0 || c->ffn <= 0) return false;
    if (c->dim != c->heads * 64 || (c->dim & 63) || (c->ffn & 63) || c->dim > 4096) return false;
    if (c->image % c->patch || c->image > 4096 || c->patch > 256) return false;
    if (c->layerscale != 0 && c->layerscale != 1) return false;
    return true;
}

// HF Dinov2Model.state_dict() order without mask_token (see the header)
DModel build_dino(const uspace_dino_config& c) {
    DModel m;
    ParamTable& t = m.t;
    auto put = [&t](long numel, PKind k) { return t.at(t.add(numel, k)); };
    const long D = c.dim, F = c.ffn, K = patch_k(c), Kp = patch_kp(c);
    m.cls = put(D, P_F32);
    m.pos = put((long)(n_patches(c) + 1) * D, P_F32);
    // patch weight [D, K] fp32 -> bf16 [D, Kp]: the region is Kp wide, the cast fills K of every row (the pack step pads)
    m.patch = t.arena.take((size_t)D * Kp * 2);
    m.i_patch = t.add_at(m.patch, D * K, P_BF16);
    m.patchb = put(D, P_F32);
    for (int i = 0; i < c.layers; ++i) {
        DinoLayer l;
        l.ln1g = put(D, P_F32);
        l.ln1b = put(D, P_F32);
        // packed projection rows q | k | v (the attention kernel's layout), which is also HF's order here
        l.wqkv = t.arena.take(3 * D * D * 2);
        l.bqkv = t.arena.take(3 * D * 4);
        for (int slot = 0; slot < 3; ++slot) {
            t.add_at(l.wqkv + slot * D * D * 2, D * D, P_BF16);
            t.add_at(l.bqkv + slot * D * 4, D, P_F32);
        }
        l.i_wo = t.add(D * D, P_BF16);
        l.i_bo = t.add(D, P_F32);
        l.i_ls1 = c.layerscale ? t.add(D, P_F32) : -1;
        l.ln2g = put(D, P_F32);
        l.ln2b = put(D, P_F32);
        l.w1 = put(F * D, P_BF16);
        l.b1 = put(F, P_F32);
        l.i_w2 = t.add(D * F, P_BF16);
        l.i_b2 = t.add(D, P_F32);
        l.i_ls2 = c.layerscale ? t.add(D, P_F32) : -1;
        l.wo = t.at(l.i_wo);
        l.bo = t.at(l.i_bo);
        l.w2 = t.at(l.i_w2);
        l.b2 = t.at(l.i_b2);
        m.layers.push_back(l);
    }
    m.ng = put(D, P_F32);
    m.nb = put(D, P_F32);
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
    size_t x, pe, rows;
    ClipEncWs enc;
    size_t tok0, total;
};
DWs plan_dino_ws(const uspace_dino_config& c, int B) {
    DWs w;
    Arena a;
    const size_t N = n_patches(c), M = (size_t)B * (N + 1), D = c.dim;
    w.x = a.take(M * D * 4);
    w.pe = a.take((size_t)B * N * D * 4);
    w.rows = a.take((size_t)B * N * patch_kp(c) * 2);
    w.enc = clip_enc_take_ws(a, M, D, (size_t)c.ffn);
    w.tok0 = a.take((size_t)B * D * 4);
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
    // + one dense bf16 copy of the patch weight behind the table: the staging area of the pad step
    return valid_dino(cfg) ? build_dino(*cfg).t.bytes() + us_align_up((size_t)cfg->dim * patch_k(*cfg) * 2) : 0;
}

extern "C" size_t uspace_dino_workspace_bytes(const uspace_dino_config* cfg, int B) {
    return (valid_dino(cfg) && B > 0) ? plan_dino_ws(*cfg, B).total : 0;
}

extern "C" int uspace_dino_pack_weights(const uspace_dino_config* cfg, const float* const* params, int n_params, void* blob,
                                        size_t blob_bytes, uspace_stream_t stream) {
    if (!valid_dino(cfg)) return USPACE_ERR_ARG;
    if (blob && blob_bytes < uspace_dino_weight_bytes(cfg)) return USPACE_ERR_WORKSPACE;
    DModel m = build_dino(*cfg);
    hipStream_t s = (hipStream_t)stream;
    const int K = patch_k(*cfg), Kp = patch_kp(*cfg), D = cfg->dim, F = cfg->ffn;
    const size_t stage = m.t.bytes();
    m.t.p[m.i_patch].offset = stage;
    US_TRY(us_pack_table(m.t, params, n_params, blob, blob_bytes, stream));
    char* wb = (char*)blob;
    hipLaunchKernelGGL(pad_patch_rows_kernel, dim3(D), dim3(256), 0, s, (const bf16_t*)(wb + stage), (bf16_t*)(wb + m.patch), K, Kp);
    US_CHECK_LAUNCH();
    if (cfg->layerscale) {
        // over the plain casts the table loop just made: the branch's last linear with lambda folded in, from the fp32 values
        for (const DinoLayer& l : m.layers) {
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
    char* ws = (char*)workspace;
    hipStream_t s = (hipStream_t)stream;
    const int D = cfg->dim, F = cfg->ffn, G = cfg->image / cfg->patch, N = G * G, T = N + 1, M = B * T;
    const int K = patch_k(*cfg), Kp = patch_kp(*cfg);
    float* x = (float*)(ws + w.x);
    float* pe = (float*)(ws + w.pe);
    uint16_t* rows = (uint16_t*)(ws + w.rows);
    uint16_t* h = (uint16_t*)(ws + w.enc.h);
    uint16_t* qkv = (uint16_t*)(ws + w.enc.qkv);
    uint16_t* att = (uint16_t*)(ws + w.enc.att);
    uint16_t* f = (uint16_t*)(ws + w.enc.f);
    float* tok0 = (float*)(ws + w.tok0);
    auto PF = [&](size_t off) { return (const float*)(wb + off); };
    auto PH = [&](size_t off) { return (const uint16_t*)(wb + off); };
    constexpr int B_ = USPACE_EPI_BIAS, G_ = USPACE_EPI_GELU, R_ = USPACE_EPI_RESIDUAL, F_ = USPACE_EPI_OUT_F32,
                  H_ = USPACE_EPI_OUT_BF16;

    hipLaunchKernelGGL(patch_rows_kernel, dim3(B * N), dim3(256), 0, s, pixel_values, rows, cfg->image, cfg->patch, G, K, Kp);
    US_CHECK_LAUNCH();
    US_TRY(uspace_gemm_bf16(rows, Kp, nullptr, 0, Kp, PH(m.patch), Kp, B * N, D, Kp, B_ | F_, PF(m.patchb), nullptr, 0, pe, D, nullptr,
                            0, stream));
    hipLaunchKernelGGL(assemble_tokens_kernel, dim3(M), dim3(256), 0, s, pe, PF(m.cls), PF(m.pos), x, T, D);
    US_CHECK_LAUNCH();
    for (int i = 0; i < n_run; ++i) {
        const DinoLayer& l = m.layers[i];
        US_TRY(uspace_layernorm_f32_bf16(x, PF(l.ln1g), PF(l.ln1b), h, M, D, cfg->eps, stream));
        US_TRY(uspace_gemm_bf16(h, D, nullptr, 0, D, PH(l.wqkv), D, M, 3 * D, D, B_ | H_, PF(l.bqkv), nullptr, 0, nullptr, 0, qkv, 3 * D,
                                stream));
        if (i == key_layer &&
            hipMemcpy2DAsync(keys_out, (size_t)D * 2, qkv + D, (size_t)3 * D * 2, (size_t)D * 2, M, hipMemcpyDeviceToDevice, s) != hipSuccess)
            return USPACE_ERR_LAUNCH;
        US_TRY(us_attention_any(qkv, nullptr, att, B, T, cfg->heads, stream));
        US_TRY(uspace_gemm_bf16(att, D, nullptr, 0, D, PH(l.wo), D, M, D, D, B_ | R_ | F_, PF(l.bo), x, D, x, D, nullptr, 0, stream));
        US_TRY(uspace_layernorm_f32_bf16(x, PF(l.ln2g), PF(l.ln2b), h, M, D, cfg->eps, stream));
        US_TRY(uspace_gemm_bf16(h, D, nullptr, 0, D, PH(l.w1), D, M, F, D, B_ | G_ | H_, PF(l.b1), nullptr, 0, nullptr, 0, f, F, stream));
        US_TRY(uspace_gemm_bf16(f, F, nullptr, 0, F, PH(l.w2), F, M, D, F, B_ | R_ | F_, PF(l.b2), x, D, x, D, nullptr, 0, stream));
    }
    if (stopped) {
        if (tap_out && hipMemcpyAsync(tap_out, x, (size_t)M * D * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) return USPACE_ERR_LAUNCH;
        return USPACE_OK;
    }
    if (!pooler_output) return USPACE_OK;
    hipLaunchKernelGGL(gather_rows_kernel, dim3(B), dim3(256), 0, s, x, (const int*)nullptr, tok0, T, D);
    US_CHECK_LAUNCH();
    return uspace_layernorm_f32(tok0, PF(m.ng), PF(m.nb), pooler_output, B, D, cfg->eps, stream);
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
