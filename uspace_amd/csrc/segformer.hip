// Segmentation on gfx950 (uspace_amd/libs/segformer.py, uspace_amd/tools/seg_metrics.py).  First the operators, each a public
// entry point of its own: the Mix-FFN's depthwise 3 x 3 convolution with its GELU, bilinear resampling of NHWC maps, the resampling
// fused with the argmax that makes a label map, and the two per-pair reductions of the segmentation-consistency metric.  Then the
// SegFormer tower that is built from them, uspace_attention_kv_bf16, the GEMM, the row LayerNorms and conv_f32.h (its head comment
// is further down).
//
// All five operators are memory-bound and do no matrix work; none uses a workspace.  Every output element is produced by ONE thread (or, for
// the reductions, one workgroup per pair in one fixed order), so a sample's or a pair's result is bit-identical whatever batch it
// sits in and wherever it sits in it.
//   bilinear: align_corners = False.  The source coordinate of output index d, ((2 d + 1) in - out) / (2 out) clamped at 0, is formed
//             in INTEGERS: the lower tap is its quotient and the weight of the upper tap its remainder over 2 out, one fp32 rounding.
//             So a tap index never depends on a floating-point floor, and in == out is the identity, exactly.  bilerp() below is the
//             one statement of the arithmetic; the label kernel calls it too, so labels == argmax(resampled logits) bit for bit.
//   argmax:   strict > in channel order: the lowest index on ties; a NaN logit never wins.
//   counts:   integers, accumulated with LDS integer atomics: integer adds are exact in any order, so the counts have one value.
//             (Runs of equal labels are added up in the thread first: a label map is piecewise constant, and 64 lanes adding to one
//             LDS word take 64 turns.)
//   sse:      fp64, thread t sums pixels t, t + 1024, ... in order, channels 0, 1, 2 inside a pixel; wave_sum_f64's tree; the 16 waves
//             in order.
// Thread-per-element forms, the 1024-thread workgroup per pair and the absence of LDS tiling are a first choice: no alternative
// was measured (profiles/seg_metrics.md has what these cost).
#include <math.h>

#include <algorithm>
#include <vector>

#include "blob.h"
#include "common.h"
#include "conv_f32.h"

namespace {

constexpr int kMaxSide = 16384;       // (2 d + 1) in stays below 2^30
constexpr int kMaxLabels = 256;
constexpr int kPairThreads = 1024;    // one workgroup per pair

struct Tap {
    int i0, i1;
    float l;      // weight of i1; i0 has 1 - l
};

__device__ __forceinline__ Tap source_tap(int d, int in, int out) {
    Tap t;
    const int num = (2 * d + 1) * in - out;       // source coordinate times 2 out
    if (num <= 0) {
        t.i0 = 0;
        t.l = 0.f;
    } else {
        const int den = 2 * out;
        t.i0 = num / den;
        t.l = (float)(num - t.i0 * den) / (float)den;
    }
    t.i1 = t.i0 + 1 < in ? t.i0 + 1 : in - 1;
    return t;
}

// (1 - ly) ((1 - lx) a + lx b) + ly ((1 - lx) c + lx d): a, b the upper row's left and right neighbour, c, d the lower row's
__device__ __forceinline__ float bilerp(float a, float b, float c, float d, float lx, float ly) {
    const float wx = 1.f - lx, wy = 1.f - ly;
    const float top = fmaf(lx, b, wx * a);
    const float bot = fmaf(lx, d, wx * c);
    return fmaf(ly, bot, wy * top);
}

// ---------------------------------------------------------------------------------------------- depthwise 3 x 3 + GELU
// One thread per (pixel, 8 channels): nine 16-byte loads of x, acc = bias then fma in (ty, tx) order, taps outside the map left
// out (their product is an exact zero), the GEMM epilogue's GELU, one 16-byte store.
__global__ __launch_bounds__(256) void dwconv3x3_gelu_kernel(const bf16_t* __restrict__ x, const float* __restrict__ w,
                                                             const float* __restrict__ bias, bf16_t* __restrict__ y, long total,
                                                             int H, int W, int C8) {
    const long id = (long)blockIdx.x * 256 + threadIdx.x;
    if (id >= total) return;
    const int c8 = (int)(id % C8);
    const long pix = id / C8;
    const int px = (int)(pix % W);
    const int py = (int)((pix / W) % H);
    const int C = C8 * 8, c0 = c8 * 8;
    f32x4 acc[2];
    acc[0] = *reinterpret_cast<const f32x4*>(bias + c0);
    acc[1] = *reinterpret_cast<const f32x4*>(bias + c0 + 4);
#pragma unroll
    for (int ty = 0; ty < 3; ++ty) {
        const int sy = py + ty - 1;
        if (sy < 0 || sy >= H) continue;
#pragma unroll
        for (int tx = 0; tx < 3; ++tx) {
            const int sx = px + tx - 1;
            if (sx < 0 || sx >= W) continue;
            const long src = pix + (long)(ty - 1) * W + (tx - 1);      // same image: sy, sx are inside it
            const uint4 raw = *reinterpret_cast<const uint4*>(x + src * C + c0);
            const float* wt = w + (ty * 3 + tx) * C + c0;
            const f32x4 w0 = *reinterpret_cast<const f32x4*>(wt);
            const f32x4 w1 = *reinterpret_cast<const f32x4*>(wt + 4);
            const uint32_t r[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float lo = __uint_as_float(r[j] << 16), hi = __uint_as_float(r[j] & 0xffff0000u);
                const int v = j >> 1, e = (j & 1) * 2;
                acc[v][e] = fmaf(lo, (v ? w1 : w0)[e], acc[v][e]);
                acc[v][e + 1] = fmaf(hi, (v ? w1 : w0)[e + 1], acc[v][e + 1]);
            }
        }
    }
    gelu_erf_batch<2>(acc);
    uint4 o;
    o.x = pack_bf2(acc[0][0], acc[0][1]);
    o.y = pack_bf2(acc[0][2], acc[0][3]);
    o.z = pack_bf2(acc[1][0], acc[1][1]);
    o.w = pack_bf2(acc[1][2], acc[1][3]);
    *reinterpret_cast<uint4*>(y + pix * C + c0) = o;
}

// ---------------------------------------------------------------------------------------------- bilinear resampling
// One thread per (output pixel, V channels), V = 4 where C, ldo, coff and the pointers allow 16-byte accesses, else 1.
template <int V>
__global__ __launch_bounds__(256) void bilinear_kernel(const float* __restrict__ x, float* __restrict__ y, long total, int h, int w,
                                                       int C, int Ho, int Wo, int ldo, int coff) {
    const long id = (long)blockIdx.x * 256 + threadIdx.x;
    if (id >= total) return;
    const int CV = C / V;
    const int c0 = (int)(id % CV) * V;
    const long pix = id / CV;
    const int ox = (int)(pix % Wo);
    const int oy = (int)((pix / Wo) % Ho);
    const long b = pix / ((long)Wo * Ho);
    const Tap tx = source_tap(ox, w, Wo), ty = source_tap(oy, h, Ho);
    const float* img = x + b * h * w * C + c0;
    const float* p00 = img + ((long)ty.i0 * w + tx.i0) * C;
    const float* p01 = img + ((long)ty.i0 * w + tx.i1) * C;
    const float* p10 = img + ((long)ty.i1 * w + tx.i0) * C;
    const float* p11 = img + ((long)ty.i1 * w + tx.i1) * C;
    float* q = y + pix * ldo + coff + c0;
    if constexpr (V == 4) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(p00), bq = *reinterpret_cast<const f32x4*>(p01);
        const f32x4 c = *reinterpret_cast<const f32x4*>(p10), d = *reinterpret_cast<const f32x4*>(p11);
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = bilerp(a[j], bq[j], c[j], d[j], tx.l, ty.l);
        *reinterpret_cast<f32x4*>(q) = o;
    } else {
        *q = bilerp(*p00, *p01, *p10, *p11, tx.l, ty.l);
    }
}

// ---------------------------------------------------------------------------------------------- resampling + argmax
// One thread per output pixel walks the L channels of its four neighbours: neighbouring lanes share them (the map is upsampled),
// so the loads are broadcasts out of L1 and the full-size logits exist only in a register.
__global__ __launch_bounds__(256) void seg_labels_kernel(const float* __restrict__ logits, uint8_t* __restrict__ labels, long total,
                                                         int h, int w, int L, int H, int W) {
    const long pix = (long)blockIdx.x * 256 + threadIdx.x;
    if (pix >= total) return;
    const int ox = (int)(pix % W);
    const int oy = (int)((pix / W) % H);
    const long b = pix / ((long)W * H);
    const Tap tx = source_tap(ox, w, W), ty = source_tap(oy, h, H);
    const float* img = logits + b * h * w * L;
    const float* p00 = img + ((long)ty.i0 * w + tx.i0) * L;
    const float* p01 = img + ((long)ty.i0 * w + tx.i1) * L;
    const float* p10 = img + ((long)ty.i1 * w + tx.i0) * L;
    const float* p11 = img + ((long)ty.i1 * w + tx.i1) * L;
    float best = bilerp(p00[0], p01[0], p10[0], p11[0], tx.l, ty.l);
    int arg = 0;
    for (int c = 1; c < L; ++c) {
        const float v = bilerp(p00[c], p01[c], p10[c], p11[c], tx.l, ty.l);
        if (v > best || (best != best && v == v)) {      // the second clause: a NaN in channel 0 does not keep the lead
            best = v;
            arg = c;
        }
    }
    labels[pix] = (uint8_t)arg;
}

// ---------------------------------------------------------------------------------------------- per-pair label counts
// hist[0][l]: pixels of label l in a, hist[1][l]: in b, hist[2][l]: in both (a == b == l).  Thread t owns the 16-pixel groups
// t, t + 1024, ...; a run of equal (a, b) inside a group is one add per histogram.  Labels >= L are counted nowhere.
__global__ __launch_bounds__(kPairThreads) void seg_pair_counts_kernel(const uint8_t* __restrict__ la, const uint8_t* __restrict__ lb,
                                                                       long npx, int L, int* __restrict__ counts) {
    __shared__ int hist[3 * kMaxLabels];
    const int tid = threadIdx.x;
    for (int i = tid; i < 3 * kMaxLabels; i += kPairThreads) hist[i] = 0;
    __syncthreads();
    const uint8_t* pa = la + (size_t)blockIdx.x * npx;
    const uint8_t* pb = lb + (size_t)blockIdx.x * npx;
    const long groups = (npx + 15) / 16;
    for (long g = tid; g < groups; g += kPairThreads) {
        const long p0 = g * 16;
        const int n = npx - p0 < 16 ? (int)(npx - p0) : 16;
        int ra = pa[p0], rb = pb[p0], run = 1;
        for (int j = 1; j <= n; ++j) {
            const int a = j < n ? pa[p0 + j] : -1, b = j < n ? pb[p0 + j] : -1;
            if (a == ra && b == rb) {
                ++run;
                continue;
            }
            if (ra < L) atomicAdd(&hist[ra], run);
            if (rb < L) atomicAdd(&hist[kMaxLabels + rb], run);
            if (ra == rb && ra < L) atomicAdd(&hist[2 * kMaxLabels + ra], run);
            ra = a;
            rb = b;
            run = 1;
        }
    }
    __syncthreads();
    int* out = counts + (size_t)blockIdx.x * 3 * L;
    for (int i = tid; i < 3 * L; i += kPairThreads) out[i] = hist[(i / L) * kMaxLabels + i % L];
}

// ---------------------------------------------------------------------------------------------- squared difference outside a region
// out[b] = { sum over the kept pixels and the 3 channels of (img_a - img_b)^2, the number of kept pixels }; a pixel is kept when the
// label of NEITHER map is in the set (member[l] != 0; labels >= L are in no set).  Images fp32 NCHW [B, 3, H, W].
__global__ __launch_bounds__(kPairThreads) void seg_region_sse_kernel(const float* __restrict__ img_a, const float* __restrict__ img_b,
                                                                      const uint8_t* __restrict__ la, const uint8_t* __restrict__ lb,
                                                                      const uint8_t* __restrict__ member, int L, long npx,
                                                                      double* __restrict__ out) {
    __shared__ uint8_t in_set[kMaxLabels];
    __shared__ double red[kPairThreads / 64];
    __shared__ long red_n[kPairThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < kMaxLabels; i += kPairThreads) in_set[i] = i < L ? member[i] : 0;
    __syncthreads();
    const size_t b = blockIdx.x;
    const uint8_t* pa = la + b * npx;
    const uint8_t* pb = lb + b * npx;
    const float* xa = img_a + b * 3 * npx;
    const float* xb = img_b + b * 3 * npx;
    double s = 0.0;
    long n = 0;
    for (long p = tid; p < npx; p += kPairThreads) {
        if (in_set[pa[p]] || in_set[pb[p]]) continue;
        ++n;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double d = (double)xa[c * npx + p] - (double)xb[c * npx + p];
            s = fma(d, d, s);
        }
    }
    s = wave_sum_f64(s);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if (lane == 0) {
        red[wave] = s;
        red_n[wave] = n;
    }
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        long m = 0;
        for (int i = 0; i < kPairThreads / 64; ++i) {
            t += red[i];
            m += red_n[i];
        }
        out[2 * b] = t;
        out[2 * b + 1] = (double)m;
    }
}

bool side_ok(int v) { return v >= 1 && v <= kMaxSide; }
bool grid_ok(long threads) { return threads >= 1 && (threads + 255) / 256 < (1L << 31); }
bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int uspace_dwconv3x3_gelu_bf16(const uint16_t* x, const float* w, const float* bias, uint16_t* y, int B, int H, int W, int C,
                                          uspace_stream_t stream) {
    if (!x || !w || !bias || !y || x == y || B < 1 || !side_ok(H) || !side_ok(W) || C < 8 || C % 8 != 0) return USPACE_ERR_ARG;
    if (!aligned16(x) || !aligned16(y) || !aligned16(w) || !aligned16(bias)) return USPACE_ERR_ARG;
    const long total = (long)B * H * W * (C / 8);
    if (!grid_ok(total) || 9L * C >= (1L << 31)) return USPACE_ERR_ARG;
    hipLaunchKernelGGL(dwconv3x3_gelu_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, w, bias, y,
                       total, H, W, C / 8);
    US_CHECK_LAUNCH();
    return USPACE_OK;
}

extern "C" int uspace_bilinear_nhwc_f32(const float* x, int B, int h, int w, int C, float* y, int Ho, int Wo, int ldo, int coff,
                                        uspace_stream_t stream) {
    if (!x || !y || B < 1 || !side_ok(h) || !side_ok(w) || !side_ok(Ho) || !side_ok(Wo) || C < 1) return USPACE_ERR_ARG;
    if (coff < 0 || ldo < 1 || (long)coff + C > ldo) return USPACE_ERR_ARG;
    if ((long)B * h * w * C >= (1L << 40) || (long)B * Ho * Wo * ldo >= (1L << 40)) return USPACE_ERR_ARG;
    const bool vec = C % 4 == 0 && ldo % 4 == 0 && coff % 4 == 0 && aligned16(x) && aligned16(y);
    const long total = (long)B * Ho * Wo * (vec ? C / 4 : C);
    if (!grid_ok(total)) return USPACE_ERR_ARG;
    const dim3 grid((unsigned)((total + 255) / 256));
    if (vec)
        hipLaunchKernelGGL(bilinear_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, x, y, total, h, w, C, Ho, Wo, ldo, coff);
    else
        hipLaunchKernelGGL(bilinear_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, x, y, total, h, w, C, Ho, Wo, ldo, coff);
    US_CHECK_LAUNCH();
    return USPACE_OK;
}

extern "C" int uspace_seg_labels_u8(const float* logits, int B, int h, int w, int L, uint8_t* labels, int H, int W,
                                    uspace_stream_t stream) {
    if (!logits || !labels || B < 1 || !side_ok(h) || !side_ok(w) || !side_ok(H) || !side_ok(W) || L < 1 || L > kMaxLabels)
        return USPACE_ERR_ARG;
    const long total = (long)B * H * W;
    if (!grid_ok(total) || (long)B * h * w * L >= (1L << 40)) return USPACE_ERR_ARG;
    hipLaunchKernelGGL(seg_labels_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, logits, labels,
                       total, h, w, L, H, W);
    US_CHECK_LAUNCH();
    return USPACE_OK;
}

extern "C" int uspace_seg_pair_counts(const uint8_t* la, const uint8_t* lb, int B, long npx, int L, int* counts,
                                      uspace_stream_t stream) {
    if (!la || !lb || !counts || B < 1 || B > 65535 || npx < 1 || npx >= (1L << 31) || L < 1 || L > kMaxLabels) return USPACE_ERR_ARG;
    hipLaunchKernelGGL(seg_pair_counts_kernel, dim3((unsigned)B), dim3(kPairThreads), 0, (hipStream_t)stream, la, lb, npx, L, counts);
    US_CHECK_LAUNCH();
    return USPACE_OK;
}

extern "C" int uspace_seg_region_sse_f64(const float* img_a, const float* img_b, const uint8_t* la, const uint8_t* lb,
                                         const uint8_t* member, int L, int B, int H, int W, double* out, uspace_stream_t stream) {
    if (!img_a || !img_b || !la || !lb || !member || !out || B < 1 || B > 65535 || !side_ok(H) || !side_ok(W) || L < 1 ||
        L > kMaxLabels)
        return USPACE_ERR_ARG;
    hipLaunchKernelGGL(seg_region_sse_kernel, dim3((unsigned)B), dim3(kPairThreads), 0, (hipStream_t)stream, img_a, img_b, la, lb,
                       member, L, (long)H * W, out);
    US_CHECK_LAUNCH();
    return USPACE_OK;
}

// ================================================================================================ the SegFormer tower
// Hugging Face SegformerForSemanticSegmentation in eval mode (MiT encoder, all-MLP decode head), head dim 64.
//   stage i:  overlapping patch embedding (conv 7x7 s4 p3 | 3x3 s2 p1, with bias; fp32 MFMA) -> LayerNorm -> the fp32 residual stream x
//   block:    x += o_proj(attn(LN1 x));  x += fc2(GELU(dwconv3x3(fc1(LN2 x))))
//             q = q_proj(LN1 x);  sr > 1: k | v = (k_proj | v_proj)(LN(conv_sr(LN1 x)))  (kernel = stride = sr, no padding: trailing
//             rows and columns dropped; the convolution in fp32 on the fp32 copy of LN1 x);  sr = 1: k | v from LN1 x itself.
//             The five linears are uspace_gemm_bf16 (bf16 operands, fp32 accumulation, the residual added in fp32), k | v ONE
//             GEMM of N = 2 C; the attention is uspace_attention_kv_bf16; dwconv + GELU is uspace_dwconv3x3_gelu_bf16.
//   stage end: LayerNorm -> the stage's fp32 map, which feeds the next stage and the head
//   head:     per stage Linear C_i -> D as a 1 x 1 convolution; bilinear resize to the stage-0 map, written straight into its slice
//             of the concatenation (reversed stage order: stage 3 first; stage 0 needs no resize and is written there by its
//             convolution); linear_fuse 1 x 1 (4 D -> D, no bias) with the batch norm folded at pack time (fp64, rounded once) and
//             ReLU; classifier 1 x 1 (D -> labels, with bias).  All fp32 on conv_f32_launch.
// LN1 is computed twice where sr > 1 (a bf16 copy for q_proj, an fp32 copy for the convolution): a form of the row kernel that
// writes both in one pass is not written.  The classifier's output channels are padded to a multiple of 4 (the convolution reads
// weight rows 16 bytes at a time) and the logits copied out without the padding.
// Every sum has one fixed order that neither B nor the sample's place in the batch changes.  Nothing of the workspace is read
// before it is written.
namespace {

struct SLin {
    size_t w, b;      // blob byte offsets: bf16 [n][k], fp32 [n]
    int n, k;
};
struct SNorm {
    size_t g, b;      // blob byte offsets, fp32 [C]
};
struct SConv {
    ConvSpec c;
    size_t w, b;      // blob byte offsets: fp32 [Kpad][cout], fp32 [cout]
    int i_w;          // parameter index of the weight (the bias, or the batch norm, follows it)
};
struct SBlock {
    SNorm ln1, ln2, srn;
    SLin q, kv, o, fc1, fc2;
    SConv sr;
    size_t dw_w, dw_b;
    int i_dw;
};
struct SStage {
    int C, heads, sr, hidden;
    SConv pe;
    SNorm pe_ln, out_ln;
    std::vector<SBlock> blocks;
};
struct SNet {
    SStage st[4];
    int D, L, Lp;
    SConv proj[4], fuse, cls;
    float eps_embed, eps_block, eps_sr, eps_stage;
    double eps_bn;
    ParamTable t;
};

bool eps_ok(float e) { return e > 0.f && e < 1.f; }

bool make_seg(const uspace_segformer_config* cfg, SNet* out) {
    if (!cfg) return false;
    if (cfg->decoder_dim < 4 || cfg->decoder_dim % 4 || cfg->decoder_dim > 2048) return false;
    if (cfg->num_labels < 1 || cfg->num_labels > kMaxLabels) return false;
    if (!eps_ok(cfg->eps_embed) || !eps_ok(cfg->eps_block) || !eps_ok(cfg->eps_sr) || !eps_ok(cfg->eps_stage) || !eps_ok(cfg->eps_bn))
        return false;
    for (int i = 0; i < 4; ++i) {
        const int C = cfg->hidden[i];
        if (C < 64 || C % 64 || C > 2048 || cfg->heads[i] * 64 != C) return false;      // head dim 64 only (MiT-B0 has 32)
        if (cfg->depths[i] < 1 || cfg->depths[i] > 256 || cfg->sr[i] < 1 || cfg->sr[i] > 16) return false;
        if (cfg->mlp[i] < 1 || cfg->mlp[i] > 8) return false;
    }
    SNet n;
    n.D = cfg->decoder_dim;
    n.L = cfg->num_labels;
    n.Lp = (n.L + 3) & ~3;
    n.eps_embed = cfg->eps_embed, n.eps_block = cfg->eps_block, n.eps_sr = cfg->eps_sr, n.eps_stage = cfg->eps_stage;
    n.eps_bn = (double)cfg->eps_bn;
    ParamTable& t = n.t;
    // a convolution: its packed weight and bias pieces, then its `after` parameters (1: its own bias; 4: a batch norm; 0: none)
    auto conv = [&](int cin, int cout, int cout_params, int k, int s, int p, int after) {
        SConv v;
        v.c = ConvSpec{cin, cout, k, k, s, p, p};
        v.w = t.arena.take((size_t)conv_kpad(v.c) * cout * sizeof(float));
        v.b = t.arena.take((size_t)cout * sizeof(float));
        v.i_w = t.add((long)cout_params * cin * k * k, P_OWNER);
        for (int j = 0; j < after; ++j) t.add(cout_params, P_OWNER);
        return v;
    };
    auto norm = [&](int C) {
        SNorm v;
        v.g = t.put(C, P_F32);
        v.b = t.put(C, P_F32);
        return v;
    };
    auto lin = [&](int nn, int k) {
        SLin v;
        v.n = nn, v.k = k;
        v.w = t.put((long)nn * k, P_BF16);
        v.b = t.put(nn, P_F32);
        return v;
    };
    for (int i = 0; i < 4; ++i) {
        SStage& s = n.st[i];
        s.C = cfg->hidden[i], s.heads = cfg->heads[i], s.sr = cfg->sr[i], s.hidden = cfg->hidden[i] * cfg->mlp[i];
        const int C = s.C;
        s.pe = i == 0 ? conv(3, C, C, 7, 4, 3, 1) : conv(cfg->hidden[i - 1], C, C, 3, 2, 1, 1);
        s.pe_ln = norm(C);
        for (int j = 0; j < cfg->depths[i]; ++j) {
            SBlock b{};
            b.ln1 = norm(C);
            b.q = lin(C, C);
            // k_proj and v_proj side by side: one weight [2 C][C] and one bias [2 C]; the parameters arrive k.w, k.b, v.w, v.b
            b.kv.n = 2 * C, b.kv.k = C;
            b.kv.w = t.arena.take((size_t)2 * C * C * 2);
            b.kv.b = t.arena.take((size_t)2 * C * sizeof(float));
            t.add_at(b.kv.w, (long)C * C, P_BF16);
            t.add_at(b.kv.b, C, P_F32);
            t.add_at(b.kv.w + (size_t)C * C * 2, (long)C * C, P_BF16);
            t.add_at(b.kv.b + (size_t)C * sizeof(float), C, P_F32);
            b.o = lin(C, C);
            if (s.sr > 1) {
                b.sr = conv(C, C, C, s.sr, s.sr, 0, 1);
                b.srn = norm(C);
            }
            b.ln2 = norm(C);
            b.fc1 = lin(s.hidden, C);
            b.dw_w = t.arena.take((size_t)9 * s.hidden * sizeof(float));
            b.i_dw = t.add((long)s.hidden * 9, P_OWNER);
            b.dw_b = t.put(s.hidden, P_F32);
            b.fc2 = lin(C, s.hidden);
            s.blocks.push_back(b);
        }
        s.out_ln = norm(C);
    }
    for (int i = 0; i < 4; ++i) n.proj[i] = conv(cfg->hidden[i], n.D, n.D, 1, 1, 0, 1);
    n.fuse = conv(4 * n.D, n.D, n.D, 1, 1, 0, 4);
    n.cls = conv(n.D, n.Lp, n.L, 1, 1, 0, 1);
    *out = std::move(n);
    return true;
}

// map sizes: stage 0 from the image, the others from the stage in front
struct SDims {
    int h[4], w[4], hk[4], wk[4];
};
bool seg_dims(const SNet& n, int H, int W, SDims* d) {
    if (H < 32 || W < 32 || H > kMaxSide || W > kMaxSide) return false;
    int h = H, w = W;
    for (int i = 0; i < 4; ++i) {
        const ConvSpec& c = n.st[i].pe.c;
        h = (h + 2 * c.ph - c.kh) / c.s + 1;
        w = (w + 2 * c.pw - c.kw) / c.s + 1;
        d->h[i] = h, d->w[i] = w;
        d->hk[i] = h / n.st[i].sr, d->wk[i] = w / n.st[i].sr;       // kernel = stride = sr, no padding
        if (d->hk[i] < 1 || d->wk[i] < 1 || (long)d->hk[i] * d->wk[i] > 336) return false;
    }
    return true;
}

struct SCarve {
    size_t conv, x, lnb, lnf, srb, q, kv, att, h1, h2, stage[4], proj, cat, fused, logits, bytes;
};
bool seg_plan(const SNet& n, int B, int H, int W, SDims* d, SCarve* c) {
    if (B < 1 || B > 32767 || !seg_dims(n, H, W, d)) return false;
    const size_t lim = (size_t)1 << 31;       // every tensor below 2^31 elements: the convolution and the GEMM count rows in int
    if ((size_t)B * H * W * 3 >= lim) return false;
    size_t mc = 0, mk = 0, mkv = 0, mh = 0, mproj = 0, msr = 0;
    for (int i = 0; i < 4; ++i) {
        const size_t M = (size_t)B * d->h[i] * d->w[i], Mk = (size_t)B * d->hk[i] * d->wk[i];
        mc = std::max(mc, M * n.st[i].C);
        mk = std::max(mk, Mk * n.st[i].C);
        mkv = std::max(mkv, (n.st[i].sr > 1 ? Mk : M) * 2 * n.st[i].C);
        mh = std::max(mh, M * n.st[i].hidden);
        if (n.st[i].sr > 1) msr = std::max(msr, M * n.st[i].C);
        if (i > 0) mproj = std::max(mproj, M * n.D);
    }
    const size_t M0 = (size_t)B * d->h[0] * d->w[0];
    if (mh >= lim || M0 * 4 * n.D >= lim || mkv >= lim) return false;
    Arena a;
    c->conv = a.take(std::max(mc, mk) * 4);
    c->x = a.take(mc * 4);
    c->lnb = a.take(mc * 2);
    c->lnf = a.take(msr * 4);
    c->srb = a.take(mk * 2);
    c->q = a.take(mc * 2);
    c->kv = a.take(mkv * 2);
    c->att = a.take(mc * 2);
    c->h1 = a.take(mh * 2);
    c->h2 = a.take(mh * 2);
    for (int i = 0; i < 4; ++i) c->stage[i] = a.take((size_t)B * d->h[i] * d->w[i] * n.st[i].C * 4);
    c->proj = a.take(mproj * 4);
    c->cat = a.take(M0 * 4 * n.D * 4);
    c->fused = a.take(M0 * n.D * 4);
    c->logits = a.take(M0 * n.Lp * 4);
    c->bytes = a.off;
    return true;
}

int seg_num_stages(const SNet& n) {
    int s = 3;      // the concatenation, the fused map, the logits
    for (int i = 0; i < 4; ++i) s += 2 + (int)n.st[i].blocks.size();
    return s;
}

// dwconv.weight [C][1][3][3] -> [9][C]
__global__ __launch_bounds__(256) void seg_pack_dw_kernel(const float* __restrict__ w, float* __restrict__ out, int C) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 9 * C) return;
    const int tap = i / C, c = i - tap * C;
    out[i] = w[c * 9 + tap];
}
// classifier.weight [L][D] -> W'[k][n] of Lp columns (columns >= L and rows >= D zero), then the bias [Lp]
__global__ __launch_bounds__(256) void seg_pack_cls_kernel(const float* __restrict__ w, const float* __restrict__ bias,
                                                           float* __restrict__ wout, float* __restrict__ bout, int D, int Kpad, int L, int Lp) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < Kpad * Lp) {
        const int k = i / Lp, nn = i - k * Lp;
        wout[i] = (k < D && nn < L) ? w[nn * D + k] : 0.f;
    } else if (i < Kpad * Lp + Lp) {
        const int nn = i - Kpad * Lp;
        bout[nn] = nn < L ? bias[nn] : 0.f;
    }
}
// rows of ld floats -> rows of n floats (the first n of each)
__global__ __launch_bounds__(256) void seg_take_columns_kernel(const float* __restrict__ x, float* __restrict__ y, long rows, int ld, int nn) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * nn) return;
    const long r = i / nn;
    y[i] = x[r * ld + (i - r * nn)];
}

struct SRun {
    const SNet& n;
    const char* blob;
    hipStream_t st;
    const float* f(size_t off) const { return (const float*)(blob + off); }
    const bf16_t* h(size_t off) const { return (const bf16_t*)(blob + off); }
    int ln_bf(const float* x, const SNorm& v, bf16_t* y, int M, int C, float eps) const {
        return uspace_layernorm_f32_bf16(x, f(v.g), f(v.b), y, M, C, eps, st);
    }
    int ln_f32(const float* x, const SNorm& v, float* y, int M, int C, float eps) const {
        return uspace_layernorm_f32(x, f(v.g), f(v.b), y, M, C, eps, st);
    }
    // out = A . W^T + bias (+ resid); one of of32 / obf
    int gemm(const bf16_t* A, const SLin& l, int M, const float* resid, float* of32, bf16_t* obf) const {
        const int flags = USPACE_EPI_BIAS | (resid ? USPACE_EPI_RESIDUAL : 0) | (of32 ? USPACE_EPI_OUT_F32 : 0) | (obf ? USPACE_EPI_OUT_BF16 : 0);
        return uspace_gemm_bf16(A, l.k, nullptr, 0, l.k, h(l.w), l.k, M, l.n, l.k, flags, f(l.b), resid, l.n, of32, l.n, obf, l.n, st);
    }
    template <int EPI>
    int conv(const SConv& v, const float* x, int B, int H, int W, float* y, int ldo, int coff, int* Ho, int* Wo) const {
        return conv_f32_launch<EPI>(v.c, x, B, H, W, f(v.w), f(v.b), y, ldo, coff, st, Ho, Wo);
    }
};

// dump != NULL: tap stage `last` is copied there and nothing later runs; dump == NULL: everything runs and `logits` is written.
int seg_run(const uspace_segformer_config* cfg, const void* blob, void* ws, size_t ws_bytes, const float* x_nhwc, int B, int H, int W,
            int last, float* dump, float* logits, hipStream_t st) {
    SNet n;
    if (!make_seg(cfg, &n) || !blob || !ws || !x_nhwc) return USPACE_ERR_ARG;
    const int S = seg_num_stages(n);
    if (!dump) last = S - 1;
    if (last < 0 || last >= S) return USPACE_ERR_ARG;
    SDims d;
    SCarve cv;
    if (!seg_plan(n, B, H, W, &d, &cv)) return USPACE_ERR_ARG;
    if (ws_bytes < cv.bytes) return USPACE_ERR_WORKSPACE;
    char* base = (char*)ws;
    float* convb = (float*)(base + cv.conv);
    float* x = (float*)(base + cv.x);
    bf16_t* lnb = (bf16_t*)(base + cv.lnb);
    float* lnf = (float*)(base + cv.lnf);
    bf16_t* srb = (bf16_t*)(base + cv.srb);
    bf16_t* q = (bf16_t*)(base + cv.q);
    bf16_t* kv = (bf16_t*)(base + cv.kv);
    bf16_t* att = (bf16_t*)(base + cv.att);
    bf16_t* h1 = (bf16_t*)(base + cv.h1);
    bf16_t* h2 = (bf16_t*)(base + cv.h2);
    const SRun r{n, (const char*)blob, st};
    int stage = 0;
    // the tap: true when `src` is the stage asked for and has been copied out
    auto tapped = [&](const float* src, size_t floats, int* rc) {
        if (!dump || stage++ != last) return false;
        *rc = hipMemcpyAsync(dump, src, floats * sizeof(float), hipMemcpyDeviceToDevice, st) == hipSuccess ? USPACE_OK : USPACE_ERR_LAUNCH;
        return true;
    };
    int rc = USPACE_OK, ho, wo;
    const float* in = x_nhwc;
    int hin = H, win = W;
    for (int i = 0; i < 4; ++i) {
        const SStage& s = n.st[i];
        const int C = s.C, h = d.h[i], w = d.w[i], M = B * h * w;
        US_TRY(r.conv<CONV_EPI_BIAS>(s.pe, in, B, hin, win, convb, C, 0, &ho, &wo));
        if (ho != h || wo != w) return USPACE_ERR_ARG;
        US_TRY(r.ln_f32(convb, s.pe_ln, x, M, C, n.eps_embed));
        if (tapped(x, (size_t)M * C, &rc)) return rc;
        for (const SBlock& b : s.blocks) {
            US_TRY(r.ln_bf(x, b.ln1, lnb, M, C, n.eps_block));
            US_TRY(r.gemm(lnb, b.q, M, nullptr, nullptr, q));
            int Lk = h * w;
            if (s.sr > 1) {
                US_TRY(r.ln_f32(x, b.ln1, lnf, M, C, n.eps_block));
                US_TRY(r.conv<CONV_EPI_BIAS>(b.sr, lnf, B, h, w, convb, C, 0, &ho, &wo));
                if (ho != d.hk[i] || wo != d.wk[i]) return USPACE_ERR_ARG;
                Lk = ho * wo;
                US_TRY(r.ln_bf(convb, b.srn, srb, B * Lk, C, n.eps_sr));
                US_TRY(r.gemm(srb, b.kv, B * Lk, nullptr, nullptr, kv));
            } else {
                US_TRY(r.gemm(lnb, b.kv, M, nullptr, nullptr, kv));
            }
            US_TRY(uspace_attention_kv_bf16(q, C, kv, 2 * C, att, C, B, h * w, Lk, s.heads, st));
            US_TRY(r.gemm(att, b.o, M, x, x, nullptr));
            US_TRY(r.ln_bf(x, b.ln2, lnb, M, C, n.eps_block));
            US_TRY(r.gemm(lnb, b.fc1, M, nullptr, nullptr, h1));
            US_TRY(uspace_dwconv3x3_gelu_bf16(h1, r.f(b.dw_w), r.f(b.dw_b), h2, B, h, w, s.hidden, st));
            US_TRY(r.gemm(h2, b.fc2, M, x, x, nullptr));
            if (tapped(x, (size_t)M * C, &rc)) return rc;
        }
        float* so = (float*)(base + cv.stage[i]);
        US_TRY(r.ln_f32(x, s.out_ln, so, M, C, n.eps_stage));
        if (tapped(so, (size_t)M * C, &rc)) return rc;
        in = so, hin = h, win = w;
    }
    // the head: stage i's projection lands in channels (3 - i) D .. of the concatenation
    const int D = n.D, h0 = d.h[0], w0 = d.w[0], M0 = B * h0 * w0;
    float* cat = (float*)(base + cv.cat);
    float* proj = (float*)(base + cv.proj);
    float* fused = (float*)(base + cv.fused);
    float* lp = (float*)(base + cv.logits);
    for (int i = 0; i < 4; ++i) {
        const float* so = (const float*)(base + cv.stage[i]);
        if (i == 0) {
            US_TRY(r.conv<CONV_EPI_BIAS>(n.proj[0], so, B, h0, w0, cat, 4 * D, 3 * D, &ho, &wo));
        } else {
            US_TRY(r.conv<CONV_EPI_BIAS>(n.proj[i], so, B, d.h[i], d.w[i], proj, D, 0, &ho, &wo));
            US_TRY(uspace_bilinear_nhwc_f32(proj, B, d.h[i], d.w[i], D, cat, h0, w0, 4 * D, (3 - i) * D, st));
        }
    }
    if (tapped(cat, (size_t)M0 * 4 * D, &rc)) return rc;
    US_TRY(r.conv<CONV_EPI_RELU>(n.fuse, cat, B, h0, w0, fused, D, 0, &ho, &wo));
    if (tapped(fused, (size_t)M0 * D, &rc)) return rc;
    US_TRY(r.conv<CONV_EPI_BIAS>(n.cls, fused, B, h0, w0, lp, n.Lp, 0, &ho, &wo));
    const long cnt = (long)M0 * n.L;
    hipLaunchKernelGGL(seg_take_columns_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, (const float*)lp,
                       dump ? dump : logits, (long)M0, n.Lp, n.L);
    US_CHECK_LAUNCH();
    return USPACE_OK;
}

}  // namespace

extern "C" int uspace_segformer_num_params(const uspace_segformer_config* cfg) {
    SNet n;
    return make_seg(cfg, &n) ? n.t.n_params : USPACE_ERR_ARG;
}

extern "C" long uspace_segformer_param_numel(const uspace_segformer_config* cfg, int index) {
    SNet n;
    return make_seg(cfg, &n) ? n.t.numel(index) : USPACE_ERR_ARG;
}

extern "C" size_t uspace_segformer_weight_bytes(const uspace_segformer_config* cfg) {
    SNet n;
    return make_seg(cfg, &n) ? n.t.bytes() : 0;
}

extern "C" size_t uspace_segformer_workspace_bytes(const uspace_segformer_config* cfg, int B, int H, int W) {
    SNet n;
    SDims d;
    SCarve c;
    return make_seg(cfg, &n) && seg_plan(n, B, H, W, &d, &c) ? c.bytes : 0;
}

extern "C" int uspace_segformer_num_stages(const uspace_segformer_config* cfg) {
    SNet n;
    return make_seg(cfg, &n) ? seg_num_stages(n) : USPACE_ERR_ARG;
}

extern "C" int uspace_segformer_pack_weights(const uspace_segformer_config* cfg, const float* const* params, int n_params, void* blob,
                                             size_t blob_bytes, uspace_stream_t stream) {
    SNet n;
    if (!make_seg(cfg, &n)) return USPACE_ERR_ARG;
    US_TRY(us_pack_table(n.t, params, n_params, blob, blob_bytes, stream));      // the checks; LayerNorms, linears, biases
    hipStream_t st = (hipStream_t)stream;
    char* out = (char*)blob;
    auto conv_bias = [&](const SConv& v) {
        return conv_f32_pack(v.c, params[v.i_w], ConvPackSource::with_bias(params[v.i_w + 1]), (float*)(out + v.w), (float*)(out + v.b), st);
    };
    for (int i = 0; i < 4; ++i) {
        US_TRY(conv_bias(n.st[i].pe));
        for (const SBlock& b : n.st[i].blocks) {
            if (n.st[i].sr > 1) US_TRY(conv_bias(b.sr));
            const int Ch = n.st[i].hidden;
            hipLaunchKernelGGL(seg_pack_dw_kernel, dim3((unsigned)us_cdiv(9 * Ch, 256)), dim3(256), 0, st, params[b.i_dw],
                               (float*)(out + b.dw_w), Ch);
            US_CHECK_LAUNCH();
        }
        US_TRY(conv_bias(n.proj[i]));
    }
    US_TRY(conv_f32_pack(n.fuse.c, params[n.fuse.i_w], ConvPackSource::batch_norm(params + n.fuse.i_w + 1, n.eps_bn),
                         (float*)(out + n.fuse.w), (float*)(out + n.fuse.b), st));
    const int Kpad = conv_kpad(n.cls.c), cnt = Kpad * n.Lp + n.Lp;
    hipLaunchKernelGGL(seg_pack_cls_kernel, dim3((unsigned)us_cdiv(cnt, 256)), dim3(256), 0, st, params[n.cls.i_w], params[n.cls.i_w + 1],
                       (float*)(out + n.cls.w), (float*)(out + n.cls.b), n.D, Kpad, n.L, n.Lp);
    US_CHECK_LAUNCH();
    return USPACE_OK;
}

extern "C" int uspace_segformer_forward(const uspace_segformer_config* cfg, const void* blob, void* workspace, size_t workspace_bytes,
                                        const float* x_nhwc, int B, int H, int W, float* logits, uspace_stream_t stream) {
    if (!logits) return USPACE_ERR_ARG;
    return seg_run(cfg, blob, workspace, workspace_bytes, x_nhwc, B, H, W, 0, nullptr, logits, (hipStream_t)stream);
}

extern "C" int uspace_segformer_tap(const uspace_segformer_config* cfg, const void* blob, void* workspace, size_t workspace_bytes,
                                    const float* x_nhwc, int B, int H, int W, int stage, float* dump, uspace_stream_t stream) {
    if (!dump) return USPACE_ERR_ARG;
    return seg_run(cfg, blob, workspace, workspace_bytes, x_nhwc, B, H, W, stage, dump, nullptr, (hipStream_t)stream);
}
