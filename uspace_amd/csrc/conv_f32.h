// The fp32 convolution and 3 x 3 pooling kernels over NHWC activations that the feature networks share (inception.hip,
// lpips.hip, idnet.hip, resnet.hip), with their launchers.  fp32 operands on the fp32 matrix cores (v_mfma_f32_32x32x2_f32): that instruction is
// bit-for-bit a k-ordered fp32 fma chain, so every output element is fma(..fma(a_0 b_0, 0)..) over K in the fixed (tap, channel)
// order, whatever the batch size: each image's activations are bit-identical across batch sizes.
#pragma once
#include <math.h>

#include "common.h"

namespace {

struct ConvSpec {
    int cin, cout, kh, kw, s, ph, pw;
};

inline int conv_k(const ConvSpec& c) { return c.kh * c.kw * c.cin; }
inline int conv_kpad(const ConvSpec& c) { return (conv_k(c) + 15) & ~15; }

// ---- 3 x 3 pooling over NHWC, 4 channels per thread.  MAX: max_pool2d (padding never wins: taps outside are skipped);
// AVG: avg_pool2d(count_include_pad=False), the 9 (or fewer) valid taps summed in row-major order over their count.
template <bool MAX>
__global__ __launch_bounds__(256) void pool3_kernel(const float* __restrict__ x, float* __restrict__ y, int B, int H, int W,
                                                    int C, int s, int p, int Ho, int Wo, int ldo, int coff) {
    const int C4 = C >> 2;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)B * Ho * Wo * C4) return;
    const int c = (int)(idx % C4) * 4;
    const long pix = idx / C4;
    const int b = (int)(pix / ((long)Ho * Wo));
    const int r = (int)(pix - (long)b * Ho * Wo);
    const int oy = r / Wo, ox = r - oy * Wo;
    f32x4 acc = MAX ? (f32x4){-INFINITY, -INFINITY, -INFINITY, -INFINITY} : (f32x4){0.f, 0.f, 0.f, 0.f};
    int cnt = 0;
    for (int dy = 0; dy < 3; ++dy) {
        const int iy = oy * s - p + dy;
        if (iy < 0 || iy >= H) continue;
        for (int dx = 0; dx < 3; ++dx) {
            const int ix = ox * s - p + dx;
            if (ix < 0 || ix >= W) continue;
            const f32x4 v = *(const f32x4*)(x + (((long)b * H + iy) * W + ix) * C + c);
            if (MAX) {
                acc[0] = fmaxf(acc[0], v[0]); acc[1] = fmaxf(acc[1], v[1]);
                acc[2] = fmaxf(acc[2], v[2]); acc[3] = fmaxf(acc[3], v[3]);
            } else {
                acc += v;
            }
            ++cnt;
        }
    }
    if (!MAX) acc /= (float)cnt;
    *(f32x4*)(y + pix * ldo + coff + c) = acc;
}

// ---- implicit-GEMM convolution, fp32 MFMA.  GEMM view: M = B*Ho*Wo output pixels, N = Cout, K = kh*kw*Cin ordered
// (tap, channel).  Workgroup = 128 x 64 output tile, 4 waves of 64 x 32 (two 32 x 32 accumulators sharing the B
// operand); K advances 16 at a time through LDS (A as [k][m], B as [k][n]: both MFMA operand reads are 32 consecutive
// floats), the next K slice is prefetched into registers while the current one is multiplied.  VEC: Cin % 16 == 0,
// so a K slice is 16 consecutive channels of one tap and each thread loads 8 of them as two 16-B loads; otherwise
// (Conv2d_1a, Cin = 3) the slice is gathered element by element.  Padding and rows beyond M read as zeros.
// EPI chooses the epilogue (below); only idnet.hip and resnet.hip ask for another than the default.
struct ConvArgs {
    const float* x;
    const float* w;
    const float* bias;
    float* y;
    int H, W, cin, Ho, Wo, cout, kw, s, ph, pw, K, Kpad, ldo, coff, M;
    const float* slope = nullptr;       // CONV_EPI_PRELU: per output channel
    const float* res = nullptr;         // CONV_EPI_ADD_RELU: the residual map, row m at res + m * ldr, channel n at + n
    int ldr = 0;
};

// Epilogues: bias + ReLU (the feature networks) | bias + per-channel PReLU max(v, 0) + a_n min(v, 0) | bias alone |
// the residual block's end, y = relu((acc + bias) + res[m, n]): the bias (the folded batch norm's shift) joins the accumulator
// first and the residual second, the order of the network's own `bn(conv(x)) + identity`; the order is part of the bits.
enum { CONV_EPI_RELU = 0, CONV_EPI_PRELU = 1, CONV_EPI_BIAS = 2, CONV_EPI_ADD_RELU = 3 };

constexpr int BM = 128, BN = 64, BK = 16;

template <bool VEC, int EPI = CONV_EPI_RELU>
__global__ __launch_bounds__(256) void conv_kernel(ConvArgs a) {
    __shared__ float As[BK][BM];
    __shared__ float Bs[BK][BN];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    // A loader: one output pixel, 8 consecutive k of the slice
    const int lm = tid & (BM - 1), lh = tid >> 7;
    const int m = m0 + lm;
    const bool mvalid = m < a.M;
    int b = 0, oy = 0, ox = 0;
    if (mvalid) {
        const int hw = a.Ho * a.Wo;
        b = m / hw;
        const int r = m - b * hw;
        oy = r / a.Wo;
        ox = r - oy * a.Wo;
    }
    const int iy0 = oy * a.s - a.ph, ix0 = ox * a.s - a.pw;
    const float* xb = a.x + (size_t)b * a.H * a.W * a.cin;
    // B loader: one k row, 4 consecutive n
    const int bk = tid >> 4, bn = n0 + (tid & 15) * 4;
    const bool nvalid = bn < a.cout;

    float ra[8];
    f32x4 rb;
    auto load = [&](int k0) {
        if (VEC) {
            const int tap = k0 / a.cin, c0 = k0 - tap * a.cin + lh * 8;
            const int ty = tap / a.kw, tx = tap - ty * a.kw;
            const int iy = iy0 + ty, ix = ix0 + tx;
            if (mvalid && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) {
                const float* p = xb + ((size_t)iy * a.W + ix) * a.cin + c0;
                const f32x4 v0 = *(const f32x4*)p, v1 = *(const f32x4*)(p + 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    ra[j] = v0[j];
                    ra[4 + j] = v1[j];
                }
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) ra[j] = 0.f;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = k0 + lh * 8 + j;
                float v = 0.f;
                if (mvalid && k < a.K) {
                    const int tap = k / a.cin, c = k - tap * a.cin;
                    const int ty = tap / a.kw, tx = tap - ty * a.kw;
                    const int iy = iy0 + ty, ix = ix0 + tx;
                    if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) v = xb[((size_t)iy * a.W + ix) * a.cin + c];
                }
                ra[j] = v;
            }
        }
        rb = nvalid ? *(const f32x4*)(a.w + (size_t)(k0 + bk) * a.cout + bn) : (f32x4){0.f, 0.f, 0.f, 0.f};
    };
    auto store = [&]() {
#pragma unroll
        for (int j = 0; j < 8; ++j) As[lh * 8 + j][lm] = ra[j];
        *(f32x4*)&Bs[bk][(tid & 15) * 4] = rb;
    };

    const int wm = wave >> 1, wn = wave & 1;
    const int l32 = lane & 31, kh = lane >> 5;
    f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        acc0[r] = 0.f;
        acc1[r] = 0.f;
    }
    const int nk = a.Kpad / BK;
    load(0);
    store();
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        if (kt + 1 < nk) load((kt + 1) * BK);
#pragma unroll
        for (int kk = 0; kk < BK / 2; ++kk) {
            const int kr = 2 * kk + kh;
            const float a0 = As[kr][wm * 64 + l32];
            const float a1 = As[kr][wm * 64 + 32 + l32];
            const float bv = Bs[kr][wn * 32 + l32];
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, bv, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, bv, acc1, 0, 0, 0);
        }
        __syncthreads();
        if (kt + 1 < nk) {
            store();
            __syncthreads();
        }
    }
    // C/D of the 32x32 MFMA: column = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
    const int n = n0 + wn * 32 + l32;
    if (n >= a.cout) return;
    const float bias = a.bias[n];
    float slope = 0.f;
    if constexpr (EPI == CONV_EPI_PRELU) slope = a.slope[n];
    auto act = [&](float v) {
        if constexpr (EPI == CONV_EPI_RELU) return fmaxf(v, 0.f);
        if constexpr (EPI == CONV_EPI_PRELU) return fmaxf(v, 0.f) + slope * fminf(v, 0.f);
        return v;
    };
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * kh;
        const int mA = m0 + wm * 64 + row, mB = mA + 32;
        if constexpr (EPI == CONV_EPI_ADD_RELU) {
            if (mA < a.M) a.y[(size_t)mA * a.ldo + a.coff + n] = fmaxf((acc0[r] + bias) + a.res[(size_t)mA * a.ldr + n], 0.f);
            if (mB < a.M) a.y[(size_t)mB * a.ldo + a.coff + n] = fmaxf((acc1[r] + bias) + a.res[(size_t)mB * a.ldr + n], 0.f);
        } else {
            if (mA < a.M) a.y[(size_t)mA * a.ldo + a.coff + n] = act(acc0[r] + bias);
            if (mB < a.M) a.y[(size_t)mB * a.ldo + a.coff + n] = act(acc1[r] + bias);
        }
    }
}

// ---- launcher.  w: packed W'[k = (ty * kw + tx) * Cin + c][n] with rows K .. Kpad - 1 zero, bias [Cout]; the output pixel
// rows are ldo channels apart and the result lands at channel offset coff (Cout % 4 == 0: the weight rows are read 16 bytes
// at a time).  EPI: the epilogue (CONV_EPI_*; slope [Cout] for PReLU; res with rows ldr floats apart for ADD_RELU, which y must
// not overlap); a template, so that only the translation unit that asks for an epilogue carries its kernels.  Ho / Wo receive
// the output size.
template <int EPI = CONV_EPI_RELU>
int conv_f32_launch(const ConvSpec& c, const float* x, int B, int H, int W, const float* w, const float* bias, float* y, int ldo,
                    int coff, hipStream_t st, int* Ho, int* Wo, const float* slope = nullptr, const float* res = nullptr, int ldr = 0) {
    if (EPI == CONV_EPI_PRELU && !slope) return USPACE_ERR_ARG;
    if (EPI == CONV_EPI_ADD_RELU && (!res || ldr < c.cout)) return USPACE_ERR_ARG;
    ConvArgs a;
    a.x = x;
    a.w = w;
    a.bias = bias;
    a.y = y;
    a.H = H;
    a.W = W;
    a.cin = c.cin;
    a.Ho = (H + 2 * c.ph - c.kh) / c.s + 1;
    a.Wo = (W + 2 * c.pw - c.kw) / c.s + 1;
    a.cout = c.cout;
    a.kw = c.kw;
    a.s = c.s;
    a.ph = c.ph;
    a.pw = c.pw;
    a.K = conv_k(c);
    a.Kpad = conv_kpad(c);
    a.ldo = ldo;
    a.coff = coff;
    a.M = B * a.Ho * a.Wo;
    a.slope = slope;
    a.res = res;
    a.ldr = ldr;
    const dim3 grid(us_cdiv(a.M, BM), us_cdiv(c.cout, BN));
    if (c.cin % 16 == 0)
        hipLaunchKernelGGL((conv_kernel<true, EPI>), grid, dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL((conv_kernel<false, EPI>), grid, dim3(256), 0, st, a);
    US_CHECK_LAUNCH();
    *Ho = a.Ho;
    *Wo = a.Wo;
    return USPACE_OK;
}
// every translation unit carries the default epilogue's two kernels, as it did while that launcher was not a template
template int conv_f32_launch<CONV_EPI_RELU>(const ConvSpec&, const float*, int, int, int, const float*, const float*, float*, int, int,
                                            hipStream_t, int*, int*, const float*, const float*, int);

// ---- weight packing.  Where a packed convolution's scale and bias come from: the eval-mode batch norm that follows it
// (gamma != NULL), folded in fp64 and rounded once to fp32 -- W' = w s_n, s_n = gamma_n / sqrt(var_n + eps), bias_n = beta_n - mean_n s_n;
// or its own bias, copied; or neither: the plain weights, bout untouched.
struct ConvPackSource {
    const float *gamma = nullptr, *beta = nullptr, *mean = nullptr, *var = nullptr;
    double eps = 0.0;
    const float* bias = nullptr;
    // p: the batch norm's weight, bias, running_mean, running_var (state-dict order)
    static ConvPackSource batch_norm(const float* const* p, double eps) { return {p[0], p[1], p[2], p[3], eps, nullptr}; }
    static ConvPackSource with_bias(const float* b) { return {nullptr, nullptr, nullptr, nullptr, 0.0, b}; }
};

// w [Cout][Cin][kh][kw] -> wout W'[k = (ty * kw + tx) * Cin + c][n], zero rows k >= K; then bout [Cout]
__global__ __launch_bounds__(256) void pack_conv_kernel(const float* __restrict__ w, ConvPackSource src, float* __restrict__ wout,
                                                        float* __restrict__ bout, int cin, int cout, int kh, int kw, int K,
                                                        int Kpad) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long nw = (long)Kpad * cout;
    if (idx < nw) {
        const int k = (int)(idx / cout), n = (int)(idx - (long)k * cout);
        float v = 0.f;
        if (k < K) {
            const int tap = k / cin, c = k - tap * cin, ty = tap / kw, tx = tap - ty * kw;
            v = w[(((long)n * cin + c) * kh + ty) * kw + tx];
            if (src.gamma) v = (float)((double)v * ((double)src.gamma[n] / sqrt((double)src.var[n] + src.eps)));
        }
        wout[idx] = v;
    } else if (idx < nw + cout) {
        const int n = (int)(idx - nw);
        if (src.gamma) {
            const double s = (double)src.gamma[n] / sqrt((double)src.var[n] + src.eps);
            bout[n] = (float)((double)src.beta[n] - (double)src.mean[n] * s);
        } else if (src.bias) {
            bout[n] = src.bias[n];
        }
    }
}

inline int conv_f32_pack(const ConvSpec& c, const float* w, const ConvPackSource& src, float* wout, float* bout, hipStream_t st) {
    const long n = (long)conv_kpad(c) * c.cout + c.cout;
    hipLaunchKernelGGL(pack_conv_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, w, src, wout, bout, c.cin, c.cout, c.kh,
                       c.kw, conv_k(c), conv_kpad(c));
    US_CHECK_LAUNCH();
    return USPACE_OK;
}

// 3 x 3 pool (max or average) of x [B, H, W, C] (stride s, padding p) into y at channel offset coff of rows of ldo channels
inline int pool3_launch(const float* x, int B, int H, int W, int C, bool mx, int s, int p, float* y, int ldo, int coff,
                        hipStream_t st, int* Ho_, int* Wo_) {
    const int Ho = (H + 2 * p - 3) / s + 1, Wo = (W + 2 * p - 3) / s + 1;
    const long n = (long)B * Ho * Wo * (C / 4);
    const unsigned blocks = (unsigned)((n + 255) / 256);
    if (mx)
        hipLaunchKernelGGL(pool3_kernel<true>, dim3(blocks), dim3(256), 0, st, x, y, B, H, W, C, s, p, Ho, Wo, ldo, coff);
    else
        hipLaunchKernelGGL(pool3_kernel<false>, dim3(blocks), dim3(256), 0, st, x, y, B, H, W, C, s, p, Ho, Wo, ldo, coff);
    US_CHECK_LAUNCH();
    *Ho_ = Ho;
    *Wo_ = Wo;
    return USPACE_OK;
}

}  // namespace
