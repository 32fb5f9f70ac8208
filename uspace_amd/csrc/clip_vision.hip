// CLIP's image side and the CLIP score (HF CLIPVisionModelWithProjection + the cosine of CLIPModel): image preprocessing
// (save_image quantisation, antialiased bicubic resize, mean / std), the vision tower on the kernels of this library -- patch rows ->
// uspace_gemm_bf16, class token + position table (the front of vit_embed.h, shared with dino.hip), pre_layrnorm, the pre-LN blocks of
// vit_encoder.h (shared with clip.hip and dino.hip) with NON-causal attention, post_layernorm of token 0, visual_projection -- and the
// small fp32 pieces of the metric: a no-bias fp32 linear for the two projections, a row gather for the text pooling, the cosine and
// the normalised difference of the directional (editing) similarity.
// Every reduction runs in a fixed order inside one wave or one block: no atomics, run-to-run bit-equal.
#include <vector>

#include "vit_embed.h"
#include "vit_encoder.h"

namespace {

// ------------------------------------------------------------------------------------------------------------- preprocessing
// Keys cubic convolution kernel, a = -0.5 (the filter of torch's antialiased bicubic and of PIL's BICUBIC)
__device__ __forceinline__ float keys_cubic(float x) {
    x = fabsf(x);
    if (x < 1.0f) return (1.5f * x - 2.5f) * x * x + 1.0f;
    if (x < 2.0f) return ((-0.5f * x + 2.5f) * x - 4.0f) * x + 2.0f;
    return 0.0f;
}

// the window of output index o: input pixels lo .. lo + n - 1 (clipped to the image), centre (o + 0.5) scale, support 2 max(scale, 1)
__device__ __forceinline__ void resize_window(int o, float scale, float support, int H, float* center, int* lo, int* n) {
    const float c = scale * ((float)o + 0.5f);
    int a = (int)(c - support + 0.5f);
    a = a < 0 ? 0 : a;
    int b = (int)(c + support + 0.5f);
    b = b > H ? H : b;
    *center = c;
    *lo = a;
    *n = b - a;
}

constexpr int RS_MAX_H = 4096;    // input side the row buffer holds
constexpr int RS_MAX_TAPS = 256;  // window length: 4 max(H / S, 1) + 2 at most

// One block per output row (b, c, oy): the vertical pass over every input column into LDS, then the horizontal pass of each
// output pixel; both with the window weights renormalised to sum 1.  out = (clamp(v, 0, 255) / 255 - mean[c]) / std[c].
__global__ __launch_bounds__(256) void clip_preprocess_kernel(const float* __restrict__ img, float* __restrict__ out, int H, int S,
                                                              int quantize, float m0, float m1, float m2, float s0, float s1,
                                                              float s2) {
    __shared__ float col[RS_MAX_H];
    __shared__ float wy[RS_MAX_TAPS];
    __shared__ float wy_sum[1];
    const int oy = blockIdx.x, c = blockIdx.y, b = blockIdx.z;
    const float scale = (float)H / (float)S;
    const float support = 2.0f * fmaxf(scale, 1.0f), inv = 1.0f / fmaxf(scale, 1.0f);
    float cy;
    int y0, ny;
    resize_window(oy, scale, support, H, &cy, &y0, &ny);
    const int tid = threadIdx.x;
    // vertical weights: one wave computes them and their sum in lane order
    if (tid < 64) {
        float part = 0.0f;
        for (int j = tid; j < ny; j += 64) {
            const float w = keys_cubic(((float)(j + y0) - cy + 0.5f) * inv);
            wy[j] = w;
            part += w;
        }
        part = wave_sum(part);
        if (tid == 0) wy_sum[0] = part;
    }
    __syncthreads();
    const float ry = 1.0f / wy_sum[0];
    const float* src = img + ((size_t)(b * 3 + c) * H + y0) * H;
    for (int ix = tid; ix < H; ix += 256) {
        float acc = 0.0f;
        for (int j = 0; j < ny; ++j) {
            // two fp32 roundings, never one fused multiply-add: save_image's x.mul(255).add_(0.5) decides the ties this way
            float v = __fmul_rn(255.0f, src[(size_t)j * H + ix]);
            if (quantize) v = fminf(fmaxf(floorf(__fadd_rn(v, 0.5f)), 0.0f), 255.0f);
            acc = fmaf(wy[j], v, acc);
        }
        col[ix] = acc * ry;
    }
    __syncthreads();
    const float mean = c == 0 ? m0 : (c == 1 ? m1 : m2), sd = c == 0 ? s0 : (c == 1 ? s1 : s2);
    float* dst = out + ((size_t)(b * 3 + c) * S + oy) * S;
    for (int ox = tid; ox < S; ox += 256) {
        float cx;
        int x0, nx;
        resize_window(ox, scale, support, H, &cx, &x0, &nx);
        float acc = 0.0f, tot = 0.0f;
        for (int j = 0; j < nx; ++j) {
            const float w = keys_cubic(((float)(j + x0) - cx + 0.5f) * inv);
            acc = fmaf(w, col[x0 + j], acc);
            tot += w;
        }
        const float v = fminf(fmaxf(acc / tot, 0.0f), 255.0f) / 255.0f;
        dst[ox] = (v - mean) / sd;
    }
}

// ------------------------------------------------------------------------------------------------------------- fp32 linear
// out[b, n] = sum_k x[b, k] w[n, k]: one wave per output column n and group of LIN_ROWS batch rows; the lanes stride K in float4,
// the wave reduction has a fixed order.  K % 4 == 0.
constexpr int LIN_ROWS = 8;
__global__ __launch_bounds__(256) void linear_f32_kernel(const float* __restrict__ x, const float* __restrict__ w, float* __restrict__ out,
                                                         int B, int N, int K) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int b0 = blockIdx.y * LIN_ROWS;
    if (n >= N) return;
    float acc[LIN_ROWS];
#pragma unroll
    for (int r = 0; r < LIN_ROWS; ++r) acc[r] = 0.0f;
    const float* wr = w + (size_t)n * K;
    for (int k = lane * 4; k < K; k += 256) {
        const f32x4 wv = *(const f32x4*)(wr + k);
#pragma unroll
        for (int r = 0; r < LIN_ROWS; ++r) {
            const int b = b0 + r < B ? b0 + r : B - 1;      // rows past the batch repeat the last one and are not stored
            const f32x4 xv = *(const f32x4*)(x + (size_t)b * K + k);
            acc[r] = fmaf(wv[0], xv[0], acc[r]);
            acc[r] = fmaf(wv[1], xv[1], acc[r]);
            acc[r] = fmaf(wv[2], xv[2], acc[r]);
            acc[r] = fmaf(wv[3], xv[3], acc[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < LIN_ROWS; ++r) {
        const float v = wave_sum(acc[r]);
        if (lane == 0 && b0 + r < B) out[(size_t)(b0 + r) * N + n] = v;
    }
}

// ------------------------------------------------------------------------------------------------------------- the score
// one wave per row: out[b] = scale <a_b, c_b> / (|a_b| |c_b|), optionally max(., 0)
__global__ __launch_bounds__(256) void cosine_kernel(const float* __restrict__ a, const float* __restrict__ c, float* __restrict__ out,
                                                     int B, int D, float scale, int relu) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const float* ar = a + (size_t)b * D;
    const float* cr = c + (size_t)b * D;
    float dot = 0.0f, na = 0.0f, nc = 0.0f;
    for (int d = lane; d < D; d += 64) {
        const float u = ar[d], v = cr[d];
        dot = fmaf(u, v, dot);
        na = fmaf(u, u, na);
        nc = fmaf(v, v, nc);
    }
    dot = wave_sum(dot);
    na = wave_sum(na);
    nc = wave_sum(nc);
    float v = scale * (dot / (sqrtf(na) * sqrtf(nc)));
    if (relu) v = fmaxf(v, 0.0f);
    if (lane == 0) out[b] = v;
}

// one wave per row: out[b] = a_b / |a_b| - c_b / |c_b|  (the step of an embedding under an edit, on the unit sphere)
__global__ __launch_bounds__(256) void normalized_diff_kernel(const float* __restrict__ a, const float* __restrict__ c,
                                                              float* __restrict__ out, int B, int D) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const float* ar = a + (size_t)b * D;
    const float* cr = c + (size_t)b * D;
    float na = 0.0f, nc = 0.0f;
    for (int d = lane; d < D; d += 64) {
        na = fmaf(ar[d], ar[d], na);
        nc = fmaf(cr[d], cr[d], nc);
    }
    const float ia = 1.0f / sqrtf(wave_sum(na)), ic = 1.0f / sqrtf(wave_sum(nc));
    for (int d = lane; d < D; d += 64) out[(size_t)b * D + d] = ar[d] * ia - cr[d] * ic;
}

// ------------------------------------------------------------------------------------------------------------- the model
struct VModel {
    ParamTable t;
    size_t cls, pos, preg, preb, postg, postb, proj;
    VitPatchWeight patch;
    std::vector<VitEncLayer> layers;
};

bool valid_clipv(const uspace_clipv_config* c) {
    if (!c || !vit_enc_valid(c->dim, c->heads, c->layers, c->ffn) || !vit_patch_valid(c->image, c->patch)) return false;
    return c->proj_dim > 0 && !(c->proj_dim & 3);
}

// HF CLIPVisionModelWithProjection.state_dict() order (see the header)
VModel build_clipv(const uspace_clipv_config& c) {
    VModel m;
    ParamTable& t = m.t;
    const VitPatch g = vit_patch(c);
    const long D = c.dim;
    m.cls = t.put(D, P_F32);
    m.patch = vit_patch_add_weight(t, g);
    m.pos = t.put((long)g.tokens() * D, P_F32);
    m.preg = t.put(D, P_F32);
    m.preb = t.put(D, P_F32);
    for (int i = 0; i < c.layers; ++i) m.layers.push_back(vit_enc_add_layer(t, D, c.ffn, VIT_ORDER_CLIP, false));
    m.postg = t.put(D, P_F32);
    m.postb = t.put(D, P_F32);
    m.proj = t.put((long)c.proj_dim * D, P_F32);
    return m;
}

struct VWs {
    size_t x, e;   // the residual stream; the embeddings before pre_layrnorm (the "embeddings" tap)
    VitTowerWs vit;
    size_t pool, total;   // pooler_output when the caller takes none
};
VWs plan_clipv_ws(const uspace_clipv_config& c, int B) {
    VWs w;
    Arena a;
    const VitPatch g = vit_patch(c);
    const size_t M = (size_t)B * g.tokens(), D = c.dim;
    w.x = a.take(M * D * 4);
    w.e = a.take(M * D * 4);
    w.vit = vit_tower_take_ws(a, g, (size_t)B, (size_t)c.ffn);
    w.pool = a.take((size_t)B * D * 4);
    w.total = a.off;
    return w;
}

}  // namespace

extern "C" int uspace_clipv_num_params(const uspace_clipv_config* cfg) {
    return valid_clipv(cfg) ? build_clipv(*cfg).t.n_params : USPACE_ERR_ARG;
}

extern "C" long uspace_clipv_param_numel(const uspace_clipv_config* cfg, int index) {
    return valid_clipv(cfg) ? build_clipv(*cfg).t.numel(index) : (long)USPACE_ERR_ARG;
}

extern "C" size_t uspace_clipv_weight_bytes(const uspace_clipv_config* cfg) {
    // + the staging area of the patch weight's pad step behind the table
    return valid_clipv(cfg) ? build_clipv(*cfg).t.bytes() + vit_patch_stage_bytes(vit_patch(*cfg)) : 0;
}

extern "C" size_t uspace_clipv_workspace_bytes(const uspace_clipv_config* cfg, int B) {
    return (valid_clipv(cfg) && B > 0) ? plan_clipv_ws(*cfg, B).total : 0;
}

extern "C" int uspace_clipv_pack_weights(const uspace_clipv_config* cfg, const float* const* params, int n_params, void* blob,
                                         size_t blob_bytes, uspace_stream_t stream) {
    if (!valid_clipv(cfg)) return USPACE_ERR_ARG;
    VModel m = build_clipv(*cfg);
    return vit_pack_table(m.t, vit_patch(*cfg), m.patch, params, n_params, blob, blob_bytes, stream);
}

extern "C" int uspace_clipv_forward(const uspace_clipv_config* cfg, const void* blob, void* workspace, size_t workspace_bytes,
                                    const float* pixel_values, float* image_embeds, float* pooler_output, int B, int stop_after_layer,
                                    float* tap_out, uspace_stream_t stream) {
    if (!valid_clipv(cfg) || !blob || !workspace || !pixel_values || B <= 0) return USPACE_ERR_ARG;
    const bool tap = stop_after_layer != -1;
    if (stop_after_layer < -2 || (tap && !tap_out) || (!tap && !image_embeds)) return USPACE_ERR_ARG;
    const VModel m = build_clipv(*cfg);
    const VWs w = plan_clipv_ws(*cfg, B);
    if (workspace_bytes < w.total) return USPACE_ERR_WORKSPACE;
    const char* wb = (const char*)blob;
    char* ws = (char*)workspace;
    hipStream_t s = (hipStream_t)stream;
    const VitPatch g = vit_patch(*cfg);
    const int D = cfg->dim, T = g.tokens(), M = B * T;
    float* x = (float*)(ws + w.x);
    float* e = (float*)(ws + w.e);
    float* pool = pooler_output ? pooler_output : (float*)(ws + w.pool);
    auto PF = [&](size_t off) { return (const float*)(wb + off); };
    auto dump = [&](const float* src) {
        return hipMemcpyAsync(tap_out, src, (size_t)M * D * 4, hipMemcpyDeviceToDevice, s) == hipSuccess ? USPACE_OK : USPACE_ERR_LAUNCH;
    };

    US_TRY(vit_embed(g, (const uint16_t*)(wb + m.patch.offset), nullptr, PF(m.cls), PF(m.pos), workspace, w.vit, pixel_values, e, B,
                     stream));
    // stop_after_layer: -1 = the whole model; -2 = the embeddings before pre_layrnorm; k >= 0 = the hidden state after k layers
    if (stop_after_layer == -2) return dump(e);
    US_TRY(uspace_layernorm_f32(e, PF(m.preg), PF(m.preb), x, M, D, cfg->eps, stream));
    const VitEncRun run = {D, cfg->ffn, cfg->heads, cfg->eps, /*causal=*/false, /*erf_gelu=*/false};
    US_TRY(vit_enc_layers(m.layers, tap ? stop_after_layer : cfg->layers, run, blob, workspace, w.vit.enc, x, B, T, -1, nullptr, stream));
    if (tap) return dump(x);
    US_TRY(vit_class_token_norm(x, workspace, w.vit, PF(m.postg), PF(m.postb), pool, B, T, D, cfg->eps, stream));
    return uspace_linear_f32(pool, PF(m.proj), image_embeds, B, cfg->proj_dim, D, stream);
}

extern "C" int uspace_clip_preprocess(const float* images, float* pixel_values, int B, int H, int W, int S, int quantize,
                                      const float* mean, const float* std, uspace_stream_t stream) {
    if (!images || !pixel_values || !mean || !std || B <= 0 || H <= 0 || S <= 0 || H != W) return USPACE_ERR_ARG;
    if (H > RS_MAX_H || S > 65535 || B > 65535) return USPACE_ERR_ARG;
    const double scale = (double)H / S;
    if (4.0 * (scale > 1.0 ? scale : 1.0) + 2.0 > RS_MAX_TAPS) return USPACE_ERR_ARG;
    for (int c = 0; c < 3; ++c)
        if (!(std[c] > 0.0f)) return USPACE_ERR_ARG;
    hipLaunchKernelGGL(clip_preprocess_kernel, dim3(S, 3, B), dim3(256), 0, (hipStream_t)stream, images, pixel_values, H, S, quantize,
                       mean[0], mean[1], mean[2], std[0], std[1], std[2]);
    US_CHECK_LAUNCH();
    return USPACE_OK;
}

extern "C" int uspace_linear_f32(const float* x, const float* w, float* out, int B, int N, int K, uspace_stream_t stream) {
    if (!x || !w || !out || B <= 0 || N <= 0 || K <= 0 || (K & 3)) return USPACE_ERR_ARG;
    const int gy = us_cdiv(B, LIN_ROWS);
    if (gy > 65535) return USPACE_ERR_ARG;
    hipLaunchKernelGGL(linear_f32_kernel, dim3(us_cdiv(N, 4), gy), dim3(256), 0, (hipStream_t)stream, x, w, out, B, N, K);
    US_CHECK_LAUNCH();
    return USPACE_OK;
}

extern "C" int uspace_gather_rows_f32(const float* x, const int* idx, float* out, int B, int L, int D, uspace_stream_t stream) {
    if (!x || !idx || !out || B <= 0 || L <= 0 || D <= 0) return USPACE_ERR_ARG;
    hipLaunchKernelGGL(gather_rows_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, x, idx, out, L, D);
    US_CHECK_LAUNCH();
    return USPACE_OK;
}

extern "C" int uspace_cosine_f32(const float* a, const float* b, float* out, int B, int D, float scale, int relu,
                                 uspace_stream_t stream) {
    if (!a || !b || !out || B <= 0 || D <= 0) return USPACE_ERR_ARG;
    hipLaunchKernelGGL(cosine_kernel, dim3(us_cdiv(B, 4)), dim3(256), 0, (hipStream_t)stream, a, b, out, B, D, scale, relu);
    US_CHECK_LAUNCH();
    return USPACE_OK;
}

extern "C" int uspace_normalized_diff_f32(const float* a, const float* b, float* out, int B, int D, uspace_stream_t stream) {
    if (!a || !b || !out || B <= 0 || D <= 0) return USPACE_ERR_ARG;
    hipLaunchKernelGGL(normalized_diff_kernel, dim3(us_cdiv(B, 4)), dim3(256), 0, (hipStream_t)stream, a, b, out, B, D);
    US_CHECK_LAUNCH();
    return USPACE_OK;
}
