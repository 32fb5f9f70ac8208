// FID feature extractor on gfx950: the FID variant of Inception-v3 (pytorch-fid's fid_inception_v3, reference
// tools/inception.py) up to the final average pool, and the fp64 running statistics of its features
// (reference tools/fid_score.py: np.mean / np.cov of the pool_3 activations).
//
// Precision: fp32 operands on the fp32 matrix cores (v_mfma_f32_32x32x2_f32).  That instruction is bit-for-bit a
// k-ordered fp32 fma chain, so every output element of a convolution is fma(..fma(a_0 b_0, 0)..) over K in the fixed
// (tap, channel) order, whatever the batch size: each image's features are bit-identical across batch sizes.
//
// Layout: activations NHWC fp32 in the caller's workspace.  Every BasicConv2d (conv(bias=False) -> BatchNorm2d(eps=1e-3)
// -> ReLU) is one launch of the implicit-GEMM kernel of conv_f32.h with BN folded into the packed weights (in fp64, rounded once)
// and the bias + ReLU in its epilogue; the epilogue stores at a channel offset and row stride of the block's output, so the
// torch.cat of every Mixed block costs nothing.
#include <math.h>

#include <vector>

#include "blob.h"
#include "common.h"
#include "conv_f32.h"

namespace {

constexpr int kIn = 299;              // resize target (pytorch-fid resizes every input to 299 x 299)
constexpr double kBnEps = 1e-3;       // BatchNorm2d(eps=0.001) of torchvision's BasicConv2d
constexpr int kNumStages = 20;        // 0 resized input .. 18 Mixed_7c, 19 global mean
// per-image buffer sizes (floats): P/Q hold block inputs and outputs (largest: Conv2d_2b_3x3, 147 x 147 x 64), T1-T3 the
// branch intermediates (largest: the pooled input of Mixed_5d, 35 x 35 x 288; the resized input, 299 x 299 x 3, lives in T1)
constexpr long kBigPer = 147L * 147 * 64;
constexpr long kTmpPer = 35L * 35 * 288;

// the 94 BasicConv2d of torchvision's Inception3 with the FID patches, in state_dict (= execution) order
const std::vector<ConvSpec>& conv_specs() {
    static const std::vector<ConvSpec> specs = [] {
        std::vector<ConvSpec> v;
        auto c = [&](int ci, int co, int kh, int kw, int s, int ph, int pw) { v.push_back({ci, co, kh, kw, s, ph, pw}); };
        c(3, 32, 3, 3, 2, 0, 0);      // Conv2d_1a_3x3
        c(32, 32, 3, 3, 1, 0, 0);     // Conv2d_2a_3x3
        c(32, 64, 3, 3, 1, 1, 1);     // Conv2d_2b_3x3
        c(64, 80, 1, 1, 1, 0, 0);     // Conv2d_3b_1x1
        c(80, 192, 3, 3, 1, 0, 0);    // Conv2d_4a_3x3
        const int a_in[3] = {192, 256, 288}, a_pool[3] = {32, 64, 64};
        for (int i = 0; i < 3; ++i) {  // Mixed_5b-5d (InceptionA)
            c(a_in[i], 64, 1, 1, 1, 0, 0);
            c(a_in[i], 48, 1, 1, 1, 0, 0);
            c(48, 64, 5, 5, 1, 2, 2);
            c(a_in[i], 64, 1, 1, 1, 0, 0);
            c(64, 96, 3, 3, 1, 1, 1);
            c(96, 96, 3, 3, 1, 1, 1);
            c(a_in[i], a_pool[i], 1, 1, 1, 0, 0);
        }
        c(288, 384, 3, 3, 2, 0, 0);    // Mixed_6a (InceptionB)
        c(288, 64, 1, 1, 1, 0, 0);
        c(64, 96, 3, 3, 1, 1, 1);
        c(96, 96, 3, 3, 2, 0, 0);
        const int c7s[4] = {128, 160, 160, 192};
        for (int i = 0; i < 4; ++i) {  // Mixed_6b-6e (InceptionC)
            const int c7 = c7s[i];
            c(768, 192, 1, 1, 1, 0, 0);
            c(768, c7, 1, 1, 1, 0, 0);
            c(c7, c7, 1, 7, 1, 0, 3);
            c(c7, 192, 7, 1, 1, 3, 0);
            c(768, c7, 1, 1, 1, 0, 0);
            c(c7, c7, 7, 1, 1, 3, 0);
            c(c7, c7, 1, 7, 1, 0, 3);
            c(c7, c7, 7, 1, 1, 3, 0);
            c(c7, 192, 1, 7, 1, 0, 3);
            c(768, 192, 1, 1, 1, 0, 0);
        }
        c(768, 192, 1, 1, 1, 0, 0);    // Mixed_7a (InceptionD)
        c(192, 320, 3, 3, 2, 0, 0);
        c(768, 192, 1, 1, 1, 0, 0);
        c(192, 192, 1, 7, 1, 0, 3);
        c(192, 192, 7, 1, 1, 3, 0);
        c(192, 192, 3, 3, 2, 0, 0);
        const int e_in[2] = {1280, 2048};
        for (int i = 0; i < 2; ++i) {  // Mixed_7b, 7c (InceptionE)
            c(e_in[i], 320, 1, 1, 1, 0, 0);
            c(e_in[i], 384, 1, 1, 1, 0, 0);
            c(384, 384, 1, 3, 1, 0, 1);
            c(384, 384, 3, 1, 1, 1, 0);
            c(e_in[i], 448, 1, 1, 1, 0, 0);
            c(448, 384, 3, 3, 1, 1, 1);
            c(384, 384, 1, 3, 1, 0, 1);
            c(384, 384, 3, 1, 1, 1, 0);
            c(e_in[i], 192, 1, 1, 1, 0, 0);
        }
        return v;
    }();
    return specs;
}

// The caller's parameters, per conv: conv.weight, then bn.weight, bn.bias, bn.running_mean, bn.running_var, all five folded into
// the conv's two pieces of the blob: W [K_pad, Cout] then bias [Cout], every piece starting at a multiple of 16 floats.
struct BlobLayout {
    ParamTable t;
    std::vector<size_t> w_off, b_off;     // floats
    std::vector<int> i_w;                 // parameter index of the weight; its batch norm is i_w + 1 .. i_w + 4
};
const BlobLayout& blob_layout() {
    static const BlobLayout L = [] {
        BlobLayout l;
        l.t.arena.align = 16 * sizeof(float);
        for (const ConvSpec& c : conv_specs()) {
            l.w_off.push_back(l.t.arena.take((size_t)conv_kpad(c) * c.cout * sizeof(float)) / sizeof(float));
            l.b_off.push_back(l.t.arena.take(c.cout * sizeof(float)) / sizeof(float));
            l.i_w.push_back(l.t.add((long)c.cout * c.cin * c.kh * c.kw, P_OWNER));
            for (int j = 0; j < 4; ++j) l.t.add(c.cout, P_OWNER);
        }
        return l;
    }();
    return L;
}

// ---- input: bilinear resize (align_corners=False) of NCHW [B,3,H,W] to 299 x 299, then 2x - 1, written NHWC
__global__ __launch_bounds__(256) void resize_input_kernel(const float* __restrict__ x, float* __restrict__ out, int B, int H,
                                                           int W) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;   // (b, oy, ox)
    if (idx >= (long)B * kIn * kIn) return;
    const int b = (int)(idx / (kIn * kIn));
    const int r = (int)(idx - (long)b * kIn * kIn);
    const int oy = r / kIn, ox = r - oy * kIn;
    const float sh = (float)H / kIn, sw = (float)W / kIn;
    const float fy = fmaxf(((float)oy + 0.5f) * sh - 0.5f, 0.f);
    const float fx = fmaxf(((float)ox + 0.5f) * sw - 0.5f, 0.f);
    const int y0 = (int)fy, x0 = (int)fx;
    const int y1 = y0 + (y0 < H - 1 ? 1 : 0), x1 = x0 + (x0 < W - 1 ? 1 : 0);
    const float ly = fy - (float)y0, lx = fx - (float)x0;
    const float hy = 1.f - ly, hx = 1.f - lx;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float* p = x + ((long)b * 3 + c) * H * W;
        const float v = hy * (hx * p[(long)y0 * W + x0] + lx * p[(long)y0 * W + x1]) +
                        ly * (hx * p[(long)y1 * W + x0] + lx * p[(long)y1 * W + x1]);
        out[idx * 3 + c] = 2.f * v - 1.f;
    }
}

// ---- global spatial mean: feat[b, c] = mean over H*W of x[b, :, :, c] (fp64 sum in pixel order, rounded once)
__global__ __launch_bounds__(256) void spatial_mean_kernel(const float* __restrict__ x, float* __restrict__ feat, int B, int HW,
                                                           int C) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)B * C) return;
    const int b = (int)(idx / C), c = (int)(idx - (long)b * C);
    const float* p = x + (long)b * HW * C + c;
    double s = 0.0;
    for (int i = 0; i < HW; ++i) s += p[(long)i * C];
    feat[idx] = (float)(s / HW);
}

// ---- channel gather: out[pix, c] = x[pix, c], c < nc, of an NHWC map with C channels (the spatial features of sFID: the
// first channels of every pixel, flattened in (h, w, c) order per image)
__global__ __launch_bounds__(256) void gather_channels_kernel(const float* __restrict__ x, float* __restrict__ out, long npix,
                                                              int C, int nc) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= npix * nc) return;
    const long pix = idx / nc;
    const int c = (int)(idx - pix * nc);
    out[idx] = x[pix * C + c];
}

// ---- fp64 statistics: S2[i, j] += sum_b (x[b,i] - c[i]) (x[b,j] - c[j]) on v_mfma_f64_16x16x4_f64.  Workgroup = one
// 64 x 64 tile of the upper triangle (4 waves of 32 x 32, 2 x 2 MFMA tiles), mirrored on store; inside a diagonal tile only
// the lanes with i <= j read-modify-write, so no element is touched by two lanes.  The MFMA's k index is the sample: lane
// l supplies sample k0 + (l >> 4) of feature (l & 15) of its sub-tile; samples beyond B contribute exact zeros.
typedef __attribute__((ext_vector_type(4))) double f64x4;

__global__ __launch_bounds__(256) void stats_s2_kernel(const float* __restrict__ x, const double* __restrict__ c,
                                                       double* __restrict__ S2, int B, int F, int tiles) {
    int ti = 0, rem = blockIdx.x;
    while (rem >= tiles - ti) {
        rem -= tiles - ti;
        ++ti;
    }
    const int tj = ti + rem;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wi = wave >> 1, wj = wave & 1;
    const int r16 = lane & 15, g = lane >> 4;
    int fa[2], fb[2];
    double ca[2], cb[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        fa[t] = min(ti * 64 + wi * 32 + t * 16 + r16, F - 1);
        fb[t] = min(tj * 64 + wj * 32 + t * 16 + r16, F - 1);
        ca[t] = c[fa[t]];
        cb[t] = c[fb[t]];
    }
    f64x4 acc[2][2];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int q = 0; q < 2; ++q) acc[p][q] = (f64x4){0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < B; k0 += 4) {
        const int bb = k0 + g;
        double va[2], vb[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            va[t] = bb < B ? (double)x[(size_t)bb * F + fa[t]] - ca[t] : 0.0;
            vb[t] = bb < B ? (double)x[(size_t)bb * F + fb[t]] - cb[t] : 0.0;
        }
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int q = 0; q < 2; ++q) acc[p][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(va[p], vb[q], acc[p][q], 0, 0, 0);
    }
    // C/D of the f64 MFMA: column = lane & 15 (operand B's row), row = (lane >> 4) + 4 * reg (operand A's row)
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = ti * 64 + wi * 32 + p * 16 + g + 4 * r;
                const int j = tj * 64 + wj * 32 + q * 16 + r16;
                if (i < F && j < F && i <= j) {
                    const double v = S2[(size_t)i * F + j] + acc[p][q][r];
                    S2[(size_t)i * F + j] = v;
                    S2[(size_t)j * F + i] = v;
                }
            }
}

// S1[f] += sum_b (x[b,f] - c[f]), in sample order
__global__ __launch_bounds__(256) void stats_s1_kernel(const float* __restrict__ x, const double* __restrict__ c,
                                                       double* __restrict__ S1, int B, int F) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    const double cf = c[f];
    double s = 0.0;
    for (int b = 0; b < B; ++b) s += (double)x[(size_t)b * F + f] - cf;
    S1[f] += s;
}

// ---- host side: the forward as a sequence of launches over the workspace
struct Act {
    float* p;
    int H, W, C;
};

struct Runner {
    const float* blob;
    hipStream_t st;
    int B;
    int conv_i = 0;

    int conv(const Act& in, float* out, int ldo, int coff, Act* res) {
        const ConvSpec& c = conv_specs()[conv_i];
        const BlobLayout& L = blob_layout();
        if (c.cin != in.C) return USPACE_ERR_ARG;
        int Ho, Wo;
        US_TRY(conv_f32_launch(c, in.p, B, in.H, in.W, blob + L.w_off[conv_i], blob + L.b_off[conv_i], out, ldo, coff, st, &Ho, &Wo));
        ++conv_i;
        if (res) *res = {out, Ho, Wo, ldo};
        return USPACE_OK;
    }
    // 3 x 3 pool of `in` (stride s, padding p) into out at channel offset coff of rows of ldo channels
    int pool(const Act& in, bool mx, int s, int p, float* out, int ldo, int coff, Act* res) {
        int Ho, Wo;
        US_TRY(pool3_launch(in.p, B, in.H, in.W, in.C, mx, s, p, out, ldo, coff, st, &Ho, &Wo));
        if (res) *res = {out, Ho, Wo, ldo};
        return USPACE_OK;
    }
};

struct Work {
    float *P, *Q, *T1, *T2, *T3;
};

size_t workspace_bytes_for(int B) { return (size_t)B * (2 * kBigPer + 3 * kTmpPer) * sizeof(float); }

Work carve(void* ws, int B) {
    float* f = (float*)ws;
    Work w;
    w.P = f;
    w.Q = w.P + (size_t)B * kBigPer;
    w.T1 = w.Q + (size_t)B * kBigPer;
    w.T2 = w.T1 + (size_t)B * kTmpPer;
    w.T3 = w.T2 + (size_t)B * kTmpPer;
    return w;
}

// InceptionA (FID): 1x1 | 1x1 -> 5x5 | 1x1 -> 3x3 -> 3x3 | avg-pool (excl. pad) -> 1x1
int block_a(Runner& R, const Act& x, float* y, const Work& w, int pool_ch, Act* out) {
    const int ld = 64 + 64 + 96 + pool_ch;
    Act t1, t2, t3;
    US_TRY(R.conv(x, y, ld, 0, nullptr));
    US_TRY(R.conv(x, w.T1, 48, 0, &t1));
    US_TRY(R.conv(t1, y, ld, 64, nullptr));
    US_TRY(R.conv(x, w.T1, 64, 0, &t1));
    US_TRY(R.conv(t1, w.T2, 96, 0, &t2));
    US_TRY(R.conv(t2, y, ld, 128, nullptr));
    US_TRY(R.pool(x, false, 1, 1, w.T3, x.C, 0, &t3));
    US_TRY(R.conv(t3, y, ld, 224, out));
    out->C = ld;
    return USPACE_OK;
}

// InceptionB: 3x3 s2 | 1x1 -> 3x3 -> 3x3 s2 | max-pool 3/2
int block_b(Runner& R, const Act& x, float* y, const Work& w, Act* out) {
    const int ld = 384 + 96 + x.C;
    Act t1, t2;
    US_TRY(R.conv(x, y, ld, 0, out));
    US_TRY(R.conv(x, w.T1, 64, 0, &t1));
    US_TRY(R.conv(t1, w.T2, 96, 0, &t2));
    US_TRY(R.conv(t2, y, ld, 384, nullptr));
    US_TRY(R.pool(x, true, 2, 0, y, ld, 480, nullptr));
    out->C = ld;
    return USPACE_OK;
}

// InceptionC (FID): 1x1 | 1x1 -> 1x7 -> 7x1 | 1x1 -> 7x1 -> 1x7 -> 7x1 -> 1x7 | avg-pool (excl. pad) -> 1x1
int block_c(Runner& R, const Act& x, float* y, const Work& w, int c7, Act* out) {
    const int ld = 768;
    Act t1, t2, t3;
    US_TRY(R.conv(x, y, ld, 0, out));
    US_TRY(R.conv(x, w.T1, c7, 0, &t1));
    US_TRY(R.conv(t1, w.T2, c7, 0, &t2));
    US_TRY(R.conv(t2, y, ld, 192, nullptr));
    US_TRY(R.conv(x, w.T1, c7, 0, &t1));
    US_TRY(R.conv(t1, w.T2, c7, 0, &t2));
    US_TRY(R.conv(t2, w.T1, c7, 0, &t1));
    US_TRY(R.conv(t1, w.T2, c7, 0, &t2));
    US_TRY(R.conv(t2, y, ld, 384, nullptr));
    US_TRY(R.pool(x, false, 1, 1, w.T3, x.C, 0, &t3));
    US_TRY(R.conv(t3, y, ld, 576, nullptr));
    out->C = ld;
    return USPACE_OK;
}

// InceptionD: 1x1 -> 3x3 s2 | 1x1 -> 1x7 -> 7x1 -> 3x3 s2 | max-pool 3/2
int block_d(Runner& R, const Act& x, float* y, const Work& w, Act* out) {
    const int ld = 320 + 192 + x.C;
    Act t1, t2;
    US_TRY(R.conv(x, w.T1, 192, 0, &t1));
    US_TRY(R.conv(t1, y, ld, 0, out));
    US_TRY(R.conv(x, w.T1, 192, 0, &t1));
    US_TRY(R.conv(t1, w.T2, 192, 0, &t2));
    US_TRY(R.conv(t2, w.T1, 192, 0, &t1));
    US_TRY(R.conv(t1, y, ld, 320, nullptr));
    US_TRY(R.pool(x, true, 2, 0, y, ld, 512, nullptr));
    out->C = ld;
    return USPACE_OK;
}

// InceptionE (FID): 1x1 | 1x1 -> [1x3, 3x1] | 1x1 -> 3x3 -> [1x3, 3x1] | pool (avg excl. pad; max in Mixed_7c) -> 1x1
int block_e(Runner& R, const Act& x, float* y, const Work& w, bool max_pool, Act* out) {
    const int ld = 2048;
    Act t1, t2, t3;
    US_TRY(R.conv(x, y, ld, 0, out));
    US_TRY(R.conv(x, w.T1, 384, 0, &t1));
    US_TRY(R.conv(t1, y, ld, 320, nullptr));
    US_TRY(R.conv(t1, y, ld, 704, nullptr));
    US_TRY(R.conv(x, w.T1, 448, 0, &t1));
    US_TRY(R.conv(t1, w.T2, 384, 0, &t2));
    US_TRY(R.conv(t2, y, ld, 1088, nullptr));
    US_TRY(R.conv(t2, y, ld, 1472, nullptr));
    US_TRY(R.pool(x, max_pool, 1, 1, w.T3, x.C, 0, &t3));
    US_TRY(R.conv(t3, y, ld, 1856, nullptr));
    out->C = ld;
    return USPACE_OK;
}

int spatial_mean(const Act& a, float* feat, int B, hipStream_t st) {
    const long n = (long)B * a.C;
    hipLaunchKernelGGL(spatial_mean_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a.p, feat, B, a.H * a.W, a.C);
    US_CHECK_LAUNCH();
    return USPACE_OK;
}

// Channels of every tap stage 0 .. 18, what the walk below produces (tests/test_eval_suite_host.py holds it against the
// Python side's STAGE_SHAPES): the gather's arguments are checked against it before anything is launched.
constexpr int kStageChannels[19] = {3, 32, 32, 64, 64, 80, 192, 192, 256, 288, 288, 768, 768, 768, 768, 768, 1280, 2048, 2048};

bool spatial_args_ok(int stage, int channels) { return stage >= 1 && stage <= 18 && channels >= 1 && channels <= kStageChannels[stage]; }

// Runs stages 0 .. last.  With tap_out, copies stage `last` (NHWC, or [B, 2048] for stage 19) there; with feat, writes
// the spatial mean of stage `last` (4, 7, 15 or 18) to feat [B, C].  With spatial, channels [0, sp_channels) of every pixel
// of stage sp_stage (1 .. min(last, 18)) are gathered to spatial [B, h * w * sp_channels] as soon as that stage is complete:
// its buffer is written again two stages later.
int run(const void* blob, void* ws, size_t ws_bytes, const float* x, int B, int H, int W, int last, float* tap_out,
        float* feat, hipStream_t st, float* spatial = nullptr, int sp_stage = 0, int sp_channels = 0) {
    if (!blob || !ws || !x || B <= 0 || H <= 0 || W <= 0 || last < 0 || last >= kNumStages) return USPACE_ERR_ARG;
    if (spatial && (!spatial_args_ok(sp_stage, sp_channels) || sp_stage > last)) return USPACE_ERR_ARG;
    // every NHWC tensor (and the input) stays below 2^31 elements
    if ((long)B * kBigPer >= (1L << 31) || (long)B * 3 * H * W >= (1L << 31)) return USPACE_ERR_ARG;
    if (ws_bytes < workspace_bytes_for(B)) return USPACE_ERR_WORKSPACE;
    const Work w = carve(ws, B);
    Runner R{(const float*)blob, st, B};
    int stage = 0;
    Act cur{w.T1, kIn, kIn, 3};
    {
        const long n = (long)B * kIn * kIn;
        hipLaunchKernelGGL(resize_input_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x, w.T1, B, H, W);
        US_CHECK_LAUNCH();
    }
    float* bufs[2] = {w.P, w.Q};
    int nb = 0;
    auto next = [&]() { float* p = bufs[nb]; nb ^= 1; return p; };
    // stem and the blocks, one stage each
    for (stage = 1; stage <= last && stage <= 18; ++stage) {
        Act o;
        float* y = next();
        switch (stage) {
            case 1: case 2: case 3: case 5: case 6: US_TRY(R.conv(cur, y, conv_specs()[R.conv_i].cout, 0, &o)); break;
            case 4: case 7: US_TRY(R.pool(cur, true, 2, 0, y, cur.C, 0, &o)); break;
            case 8: US_TRY(block_a(R, cur, y, w, 32, &o)); break;
            case 9: case 10: US_TRY(block_a(R, cur, y, w, 64, &o)); break;
            case 11: US_TRY(block_b(R, cur, y, w, &o)); break;
            case 12: US_TRY(block_c(R, cur, y, w, 128, &o)); break;
            case 13: case 14: US_TRY(block_c(R, cur, y, w, 160, &o)); break;
            case 15: US_TRY(block_c(R, cur, y, w, 192, &o)); break;
            case 16: US_TRY(block_d(R, cur, y, w, &o)); break;
            case 17: US_TRY(block_e(R, cur, y, w, false, &o)); break;
            case 18: US_TRY(block_e(R, cur, y, w, true, &o)); break;
        }
        o.p = y;
        cur = o;
        if (spatial && stage == sp_stage) {
            const long npix = (long)B * cur.H * cur.W;
            hipLaunchKernelGGL(gather_channels_kernel, dim3((unsigned)((npix * sp_channels + 255) / 256)), dim3(256), 0, st, cur.p,
                               spatial, npix, cur.C, sp_channels);
            US_CHECK_LAUNCH();
        }
    }
    if (tap_out) {
        if (last == 19) return spatial_mean(cur, tap_out, B, st);
        const size_t bytes = (size_t)B * cur.H * cur.W * cur.C * sizeof(float);
        if (hipMemcpyAsync(tap_out, cur.p, bytes, hipMemcpyDeviceToDevice, st) != hipSuccess) return USPACE_ERR_LAUNCH;
        return USPACE_OK;
    }
    return spatial_mean(cur, feat, B, st);
}

}  // namespace

extern "C" int uspace_inception_num_params(void) { return blob_layout().t.n_params; }

extern "C" long uspace_inception_param_numel(int index) { return blob_layout().t.numel(index); }

extern "C" size_t uspace_inception_weight_bytes(void) { return blob_layout().t.bytes(); }

extern "C" size_t uspace_inception_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return workspace_bytes_for(B);
}

extern "C" int uspace_inception_pack_weights(const float* const* params, int n_params, void* blob, size_t blob_bytes,
                                             uspace_stream_t stream) {
    const BlobLayout& L = blob_layout();
    US_TRY(us_pack_table(L.t, params, n_params, blob, blob_bytes, stream));      // the checks: every entry is the pack step's below
    float* out = (float*)blob;
    for (size_t i = 0; i < L.i_w.size(); ++i)
        US_TRY(conv_f32_pack(conv_specs()[i], params[L.i_w[i]], ConvPackSource::batch_norm(params + L.i_w[i] + 1, kBnEps),
                             out + L.w_off[i], out + L.b_off[i], (hipStream_t)stream));
    return USPACE_OK;
}

extern "C" int uspace_inception_forward(const void* blob, void* workspace, size_t workspace_bytes, const float* x, int B,
                                        int H, int W, int last_block, float* feat, uspace_stream_t stream) {
    static const int block_stage[4] = {4, 7, 15, 18};
    if (!feat || last_block < 0 || last_block > 3) return USPACE_ERR_ARG;
    return run(blob, workspace, workspace_bytes, x, B, H, W, block_stage[last_block], nullptr, feat, (hipStream_t)stream);
}

extern "C" int uspace_inception_tap(const void* blob, void* workspace, size_t workspace_bytes, const float* x, int B, int H,
                                    int W, int stage, float* out, uspace_stream_t stream) {
    if (!out) return USPACE_ERR_ARG;
    return run(blob, workspace, workspace_bytes, x, B, H, W, stage, out, nullptr, (hipStream_t)stream);
}

extern "C" int uspace_inception_forward_suite(const void* blob, void* workspace, size_t workspace_bytes, const float* x, int B,
                                              int H, int W, float* pool, float* spatial, int spatial_stage, int spatial_channels,
                                              uspace_stream_t stream) {
    if (!pool) return USPACE_ERR_ARG;
    if (!spatial_args_ok(spatial_stage, spatial_channels)) return USPACE_ERR_ARG;      // whether or not the gather is asked for
    return run(blob, workspace, workspace_bytes, x, B, H, W, 18, nullptr, pool, (hipStream_t)stream, spatial, spatial_stage,
               spatial_channels);
}

extern "C" int uspace_fid_stats_accumulate(const float* feat, int B, int F, const double* shift, double* s1, double* s2,
                                           uspace_stream_t stream) {
    if (!feat || !shift || !s1 || !s2 || B <= 0 || F <= 0 || (long)B * F >= (1L << 31)) return USPACE_ERR_ARG;
    const int tiles = us_cdiv(F, 64);
    const long blocks = (long)tiles * (tiles + 1) / 2;
    hipLaunchKernelGGL(stats_s2_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, feat, shift, s2, B, F, tiles);
    US_CHECK_LAUNCH();
    hipLaunchKernelGGL(stats_s1_kernel, dim3(us_cdiv(F, 256)), dim3(256), 0, (hipStream_t)stream, feat, shift, s1, B, F);
    US_CHECK_LAUNCH();
    return USPACE_OK;
}
