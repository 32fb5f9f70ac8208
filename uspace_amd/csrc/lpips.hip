// Paired edit-fidelity metrics on gfx950: LPIPS (Zhang et al. 2018; AlexNet and VGG-16 feature stacks with the linear
// heads of the lpips package), SSIM (Wang et al. 2004, 11-tap Gaussian window, sigma 1.5, "valid" region) and PSNR.
//
// LPIPS: the pair runs as ONE batch of 2B images (rows b and B + b belong together) through the fp32-MFMA convolution of
// conv_f32.h (bias + ReLU in its epilogue; no batch norm), activations NHWC fp32 in the caller's workspace.  After stage l
// (the l-th tapped ReLU) the distance head runs on that stage's map, so a tap need not outlive its stage:
//   d_l[b] = (1 / HW) sum_pixels sum_c w_c (a_c / (sqrt(sum a^2) + 1e-10) - b_c / (sqrt(sum b^2) + 1e-10))^2
// in exactly this form (the expanded form with dot products cancels for near-identical pairs): one wave per pixel, a
// lane holds C / 64 channels, the norms and the weighted sum are fp32 wave reductions, the sum over pixels is fp64.
//
// Every fp64 sum has one fixed order that neither B nor the image's place in the batch changes: per-workgroup partial
// sums over a constant number of pixels (elements, window positions), then one wave per image over the partials.  No
// atomics.  Nothing of a workspace is read before it is written.
#include <math.h>

#include <vector>

#include "blob.h"
#include "common.h"
#include "conv_f32.h"

namespace {

// ------------------------------------------------------------------------------------------------ the two backbones
enum { OP_CONV = 0, OP_POOL3 = 1, OP_POOL2 = 2 };   // convolution (+ bias + ReLU) | max pool 3 x 3 stride 2 | max pool 2 x 2 stride 2 (floor)
struct Op {
    int kind, conv;
};
constexpr int kNumTaps = 5;
struct Net {
    std::vector<ConvSpec> convs;
    std::vector<Op> stage[kNumTaps];      // stage l + 1 of uspace_lpips_tap: the operations from tap l - 1 (or the scaled input) to tap l
    int tap_c[kNumTaps];
    // The caller's parameters: per conv weight and bias, then lin0 .. lin4.  Packed blob (offsets in floats): per conv W [K_pad, Cout]
    // then bias [Cout]; then the lin vectors, copied by the table; every piece starting at a multiple of 16 floats
    ParamTable t;
    std::vector<size_t> w_off, b_off;
    std::vector<int> i_w;                 // parameter index of a conv's weight; its bias is i_w + 1
    size_t lin_off[kNumTaps];
};

Net make_net(int which) {
    Net n;
    auto conv = [&](int l, int ci, int co, int k, int s, int p) {
        n.stage[l].push_back({OP_CONV, (int)n.convs.size()});
        n.convs.push_back({ci, co, k, k, s, p, p});
    };
    if (which == 0) {                     // torchvision alexnet.features, taps after the five ReLUs
        conv(0, 3, 64, 11, 4, 2);
        n.stage[1].push_back({OP_POOL3, 0});
        conv(1, 64, 192, 5, 1, 2);
        n.stage[2].push_back({OP_POOL3, 0});
        conv(2, 192, 384, 3, 1, 1);
        conv(3, 384, 256, 3, 1, 1);
        conv(4, 256, 256, 3, 1, 1);
    } else {                              // torchvision vgg16.features, taps after relu1_2, 2_2, 3_3, 4_3, 5_3
        const int width[kNumTaps] = {64, 128, 256, 512, 512}, count[kNumTaps] = {2, 2, 3, 3, 3};
        int ci = 3;
        for (int l = 0; l < kNumTaps; ++l) {
            if (l) n.stage[l].push_back({OP_POOL2, 0});
            for (int j = 0; j < count[l]; ++j) {
                conv(l, ci, width[l], 3, 1, 1);
                ci = width[l];
            }
        }
    }
    n.t.arena.align = 16 * sizeof(float);
    for (const ConvSpec& c : n.convs) {
        n.w_off.push_back(n.t.arena.take((size_t)conv_kpad(c) * c.cout * sizeof(float)) / sizeof(float));
        n.b_off.push_back(n.t.arena.take(c.cout * sizeof(float)) / sizeof(float));
        n.i_w.push_back(n.t.add((long)c.cout * c.cin * c.kh * c.kw, P_OWNER));
        n.t.add(c.cout, P_OWNER);
    }
    for (int l = 0; l < kNumTaps; ++l) {
        n.tap_c[l] = n.convs[n.stage[l].back().conv].cout;
        n.lin_off[l] = n.t.at(n.t.add(n.tap_c[l], P_F32)) / sizeof(float);
    }
    return n;
}

const Net* net_of(int which) {
    static const Net nets[2] = {make_net(0), make_net(1)};
    return which == 0 || which == 1 ? &nets[which] : nullptr;
}

// What the walk produces for an H x W input: the size of every tap and the largest activation of one image (floats).
// false where a map would vanish (an input too small for the stack).
struct Walk {
    int h[kNumTaps], w[kNumTaps];
    size_t max_act = 0;
};
bool walk(const Net& n, int H, int W, Walk* out) {
    Walk k;
    int h = H, w = W, c = 3;
    for (int l = 0; l < kNumTaps; ++l) {
        for (const Op& op : n.stage[l]) {
            if (op.kind == OP_CONV) {
                const ConvSpec& s = n.convs[op.conv];
                if (h + 2 * s.ph < s.kh || w + 2 * s.pw < s.kw) return false;
                h = (h + 2 * s.ph - s.kh) / s.s + 1;
                w = (w + 2 * s.pw - s.kw) / s.s + 1;
                c = s.cout;
            } else if (op.kind == OP_POOL3) {
                if (h < 3 || w < 3) return false;
                h = (h - 3) / 2 + 1;
                w = (w - 3) / 2 + 1;
            } else {
                if (h < 2 || w < 2) return false;
                h /= 2;
                w /= 2;
            }
            const size_t act = (size_t)h * w * c;
            if (act > k.max_act) k.max_act = act;
        }
        k.h[l] = h;
        k.w[l] = w;
    }
    *out = k;
    return true;
}

// ------------------------------------------------------------------------------------------------ small kernels
// the ScalingLayer of lpips: NCHW fp32 [B, 3, H, W] -> NHWC (v - shift_c) / scale_c, v = x (images in [-1, 1]) or 2 x - 1
// (normalize: images in [0, 1]).  The shift is not folded into the first convolution: its zero padding pads this tensor.
__global__ __launch_bounds__(256) void scale_input_kernel(const float* __restrict__ x, float* __restrict__ out, long npix, int HW,
                                                          int normalize) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;   // (b, y, x)
    if (idx >= npix) return;
    const long b = idx / HW;
    const int r = (int)(idx - b * HW);
    const float shift[3] = {-0.030f, -0.088f, -0.188f}, scale[3] = {0.458f, 0.448f, 0.450f};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float v = x[(b * 3 + c) * HW + r];
        if (normalize) v = 2.f * v - 1.f;
        out[idx * 3 + c] = (v - shift[c]) / scale[c];
    }
}

// 2 x 2 max pool, stride 2, floor (a last odd row / column is dropped), NHWC, 4 channels per thread
__global__ __launch_bounds__(256) void pool2_kernel(const float* __restrict__ x, float* __restrict__ y, int B, int H, int W, int C,
                                                    int Ho, int Wo) {
    const int C4 = C >> 2;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)B * Ho * Wo * C4) return;
    const int c = (int)(idx % C4) * 4;
    const long pix = idx / C4;
    const int b = (int)(pix / ((long)Ho * Wo));
    const int r = (int)(pix - (long)b * Ho * Wo);
    const int oy = r / Wo, ox = r - oy * Wo;
    const float* p = x + (((long)b * H + 2 * oy) * W + 2 * ox) * C + c;     // 2 oy + 1 <= H - 1 and 2 ox + 1 <= W - 1 by the floor
    const f32x4 v00 = *(const f32x4*)p, v01 = *(const f32x4*)(p + C);
    const f32x4 v10 = *(const f32x4*)(p + (long)W * C), v11 = *(const f32x4*)(p + (long)W * C + C);
    f32x4 m;
#pragma unroll
    for (int j = 0; j < 4; ++j) m[j] = fmaxf(fmaxf(v00[j], v01[j]), fmaxf(v10[j], v11[j]));
    *(f32x4*)(y + pix * C + c) = m;
}

// the four waves' sums joined in wave order; every thread passes its wave's value, thread 0 receives the sum
__device__ __forceinline__ double block_sum_f64(double wave_total, double* red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) red[wave] = wave_total;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// sum of part[0 .. n): 64 lane-strided chains joined by a butterfly (one wave)
__device__ __forceinline__ double wave_sum_partials(const double* __restrict__ part, long n) {
    double s = 0.0;
    for (long i = threadIdx.x; i < n; i += 64) s += part[i];
    return wave_sum_f64(s);
}

// ------------------------------------------------------------------------------------------------ the distance head
constexpr int kHeadPix = 64;      // pixels per partial sum (a constant of the summation order, not of the launch)

// f0, f1: [B, HW, C] NHWC maps of the two sides, C = 64 NPL; part[b, chunk] = sum over the chunk's pixels of
// sum_c w_c (a_c / (|a| + eps) - b_c / (|b| + eps))^2.  Wave v of the workgroup takes pixels v, v + 4, ... of the chunk.
template <int NPL>
__global__ __launch_bounds__(256) void lpips_head_kernel(const float* __restrict__ f0, const float* __restrict__ f1,
                                                         const float* __restrict__ w, double* __restrict__ part, int HW, int nchunk) {
    __shared__ double red[4];
    constexpr int C = 64 * NPL;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.y, chunk = blockIdx.x;
    const float* pa = f0 + (size_t)b * HW * C;
    const float* pb = f1 + (size_t)b * HW * C;
    float wj[NPL];
#pragma unroll
    for (int j = 0; j < NPL; ++j) wj[j] = w[lane + 64 * j];
    double acc = 0.0;
    for (int i = wave; i < kHeadPix; i += 4) {
        const int pix = chunk * kHeadPix + i;
        if (pix >= HW) break;                                   // wave-uniform
        float a[NPL], c[NPL];
#pragma unroll
        for (int j = 0; j < NPL; ++j) {
            a[j] = pa[(size_t)pix * C + lane + 64 * j];
            c[j] = pb[(size_t)pix * C + lane + 64 * j];
        }
        float sa = 0.f, sc = 0.f;
#pragma unroll
        for (int j = 0; j < NPL; ++j) {
            sa = fmaf(a[j], a[j], sa);
            sc = fmaf(c[j], c[j], sc);
        }
        const float na = sqrtf(wave_sum(sa)) + 1e-10f, nc = sqrtf(wave_sum(sc)) + 1e-10f;
        float t = 0.f;
#pragma unroll
        for (int j = 0; j < NPL; ++j) {
            const float d = a[j] / na - c[j] / nc;
            t = fmaf(wj[j], d * d, t);
        }
        acc += (double)wave_sum(t);
    }
    const double s = block_sum_f64(acc, red);
    if (threadIdx.x == 0) part[(size_t)b * nchunk + chunk] = s;
}

// d[b] = (sum of the image's partials) / HW; one wave per image
__global__ __launch_bounds__(64) void lpips_head_finish_kernel(const double* __restrict__ part, double* __restrict__ d, int nchunk,
                                                               int HW) {
    const int b = blockIdx.x;
    const double s = wave_sum_partials(part + (size_t)b * nchunk, nchunk);
    if (threadIdx.x == 0) d[b] = s / HW;
}

// out[b] = d_0[b] + d_1[b] + ... + d_4[b], in layer order
__global__ __launch_bounds__(256) void lpips_total_kernel(const double* __restrict__ layer, double* __restrict__ out, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double s = 0.0;
    for (int l = 0; l < kNumTaps; ++l) s += layer[(size_t)l * B + b];
    out[b] = s;
}

bool head_args_ok(int B, int HW, int C) { return B >= 1 && B <= 65535 && HW >= 1 && C >= 64 && C <= 512 && C % 64 == 0; }
int head_chunks(int HW) { return us_cdiv(HW, kHeadPix); }

int head_launch(const float* f0, const float* f1, const float* w, int B, int HW, int C, double* part, double* d, hipStream_t st) {
    const int nchunk = head_chunks(HW);
    const dim3 grid(nchunk, B);
#define US_HEAD(NPL)                                                                                               \
    case NPL:                                                                                                      \
        hipLaunchKernelGGL(lpips_head_kernel<NPL>, grid, dim3(256), 0, st, f0, f1, w, part, HW, nchunk);           \
        break;
    switch (C / 64) {
        US_HEAD(1) US_HEAD(2) US_HEAD(3) US_HEAD(4) US_HEAD(5) US_HEAD(6) US_HEAD(7) US_HEAD(8)
        default: return USPACE_ERR_ARG;
    }
#undef US_HEAD
    US_CHECK_LAUNCH();
    hipLaunchKernelGGL(lpips_head_finish_kernel, dim3(B), dim3(64), 0, st, part, d, nchunk, HW);
    US_CHECK_LAUNCH();
    return USPACE_OK;
}

// ------------------------------------------------------------------------------------------------ SSIM
constexpr int kWin = 11, kTile = 16, kSpan = kTile + kWin - 1;     // window taps; outputs per tile side; inputs per tile side
struct SsimWindow {
    float g[kWin];
};

// One workgroup = one 16 x 16 tile of the (H - 10) x (W - 10) SSIM map of one channel of one image.  The 26 x 26 inputs of
// both images go to LDS; the five moments (x, y, x^2, y^2, x y) are filtered along rows into LDS, then along columns, one
// output per thread.  part[(b, c), tile] = the tile's sum of SSIM values in fp64 (positions beyond the map add 0).
__global__ __launch_bounds__(256) void ssim_kernel(const float* __restrict__ x, const float* __restrict__ y, double* __restrict__ part,
                                                   int H, int W, int tiles_x, SsimWindow win, float C1, float C2) {
    __shared__ float sx[kSpan][kSpan + 1], sy[kSpan][kSpan + 1];
    __shared__ float hm[5][kSpan][kTile];
    __shared__ double red[4];
    const int tid = threadIdx.x;
    const int plane = blockIdx.z * gridDim.y + blockIdx.y;
    const int ty0 = (blockIdx.x / tiles_x) * kTile, tx0 = (blockIdx.x % tiles_x) * kTile;
    const float* px = x + (size_t)plane * H * W;
    const float* py = y + (size_t)plane * H * W;
    for (int i = tid; i < kSpan * kSpan; i += 256) {
        const int r = i / kSpan, c = i - r * kSpan;
        const int gy = ty0 + r, gx = tx0 + c;
        const bool in = gy < H && gx < W;
        sx[r][c] = in ? px[(size_t)gy * W + gx] : 0.f;
        sy[r][c] = in ? py[(size_t)gy * W + gx] : 0.f;
    }
    __syncthreads();
    for (int i = tid; i < kSpan * kTile; i += 256) {
        const int r = i / kTile, c = i - r * kTile;
        float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < kWin; ++t) {
            const float a = sx[r][c + t], b = sy[r][c + t], g = win.g[t];
            m[0] = fmaf(g, a, m[0]);
            m[1] = fmaf(g, b, m[1]);
            m[2] = fmaf(g, a * a, m[2]);
            m[3] = fmaf(g, b * b, m[3]);
            m[4] = fmaf(g, a * b, m[4]);
        }
#pragma unroll
        for (int k = 0; k < 5; ++k) hm[k][r][c] = m[k];
    }
    __syncthreads();
    const int oy = tid / kTile, ox = tid - oy * kTile;
    float v[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < kWin; ++t) {
        const float g = win.g[t];
#pragma unroll
        for (int k = 0; k < 5; ++k) v[k] = fmaf(g, hm[k][oy + t][ox], v[k]);
    }
    const float mxx = v[0] * v[0], myy = v[1] * v[1], mxy = v[0] * v[1];
    const float num = (2.f * mxy + C1) * (2.f * (v[4] - mxy) + C2);
    const float den = (mxx + myy + C1) * ((v[2] - mxx) + (v[3] - myy) + C2);
    const bool valid = ty0 + oy < H - (kWin - 1) && tx0 + ox < W - (kWin - 1);
    const double s = block_sum_f64(wave_sum_f64(valid ? (double)(num / den) : 0.0), red);
    if (tid == 0) part[(size_t)plane * gridDim.x + blockIdx.x] = s;
}

// out[b] = (sum of the image's C * tiles partials) / (C (H - 10) (W - 10)); one wave per image
__global__ __launch_bounds__(64) void ssim_finish_kernel(const double* __restrict__ part, double* __restrict__ out, long nper,
                                                         double count) {
    const int b = blockIdx.x;
    const double s = wave_sum_partials(part + (size_t)b * nper, nper);
    if (threadIdx.x == 0) out[b] = s / count;
}

bool ssim_args_ok(int B, int C, int H, int W) {
    if (B < 1 || B > 65535 || C < 1 || C > 65535 || H < kWin || W < kWin) return false;
    return (long)us_cdiv(H - kWin + 1, kTile) * us_cdiv(W - kWin + 1, kTile) < (1L << 31) && (long)B * C * H * W < (1L << 40);
}
long ssim_tiles(int H, int W) { return (long)us_cdiv(H - kWin + 1, kTile) * us_cdiv(W - kWin + 1, kTile); }

// ------------------------------------------------------------------------------------------------ PSNR
constexpr int kPsnrChunk = 4096;  // elements per partial sum: 16 per thread, strided by 256

__global__ __launch_bounds__(256) void psnr_sse_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                       double* __restrict__ part, long n) {
    __shared__ double red[4];
    const int b = blockIdx.y;
    const long base = (long)blockIdx.x * kPsnrChunk;
    const float* px = x + (size_t)b * n;
    const float* py = y + (size_t)b * n;
    double s = 0.0;
#pragma unroll 4
    for (int j = 0; j < kPsnrChunk / 256; ++j) {
        const long i = base + j * 256 + threadIdx.x;
        if (i < n) {
            const double d = (double)px[i] - (double)py[i];
            s = fma(d, d, s);
        }
    }
    s = block_sum_f64(wave_sum_f64(s), red);
    if (threadIdx.x == 0) part[(size_t)b * gridDim.x + blockIdx.x] = s;
}

// out[b] = 10 log10(L^2 / mse), mse = (sum of the image's partials) / n; identical images: L^2 / 0 = +inf
__global__ __launch_bounds__(64) void psnr_finish_kernel(const double* __restrict__ part, double* __restrict__ out, long nchunk,
                                                         long n, double range2) {
    const int b = blockIdx.x;
    const double s = wave_sum_partials(part + (size_t)b * nchunk, nchunk);
    if (threadIdx.x == 0) out[b] = 10.0 * log10(range2 / (s / (double)n));
}

bool psnr_args_ok(int B, long n) { return B >= 1 && B <= 65535 && n >= 1 && (n + kPsnrChunk - 1) / kPsnrChunk < (1L << 31); }

// ------------------------------------------------------------------------------------------------ the LPIPS forward
constexpr size_t kAlign = 64;     // floats: every carved buffer starts 256 bytes apart at least
size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// one image pair's share of the workspace is 2 images: input [H, W, 3] and two activation buffers of the largest map
struct Carve {
    size_t part_doubles, layer_doubles, in_floats, act_floats;
    size_t bytes() const { return (part_doubles + layer_doubles) * sizeof(double) + (in_floats + 2 * act_floats) * sizeof(float); }
};
bool plan(const Net& n, int B, int H, int W, Walk* k, Carve* c) {
    if (B < 1 || B > 32767 || H < 1 || W < 1 || !walk(n, H, W, k)) return false;
    // every NHWC tensor of the 2B images (and the input) stays below 2^31 elements: the convolution counts pixels in int
    const size_t N = 2 * (size_t)B;
    if (N * k->max_act >= ((size_t)1 << 31) || N * 3 * (size_t)H * W >= ((size_t)1 << 31)) return false;
    int max_chunks = 0;
    for (int l = 0; l < kNumTaps; ++l) max_chunks = max(max_chunks, head_chunks(k->h[l] * k->w[l]));
    c->part_doubles = round_up((size_t)B * max_chunks, kAlign);
    c->layer_doubles = round_up((size_t)B * kNumTaps, kAlign);
    c->in_floats = round_up(N * 3 * (size_t)H * W, kAlign);
    c->act_floats = round_up(N * k->max_act, kAlign);
    return true;
}

// Runs the scaled input and stages 1 .. last.  With dump: copies stage `last` (NHWC [2B, h, w, c]; stage 0 is the scaled
// input) there and runs no head.  Otherwise (last == 5) the head of tap l runs right after stage l + 1, d_l lands in
// per_layer[l, b] (or in the workspace when per_layer is NULL) and out[b] is their sum.
int run(int which, const void* blob, void* ws, size_t ws_bytes, const float* x0, const float* x1, int B, int H, int W, int normalize,
        int last, float* dump, double* out, double* per_layer, hipStream_t st) {
    const Net* np = net_of(which);
    if (!np || !blob || !ws || !x0 || !x1 || last < 0 || last > kNumTaps) return USPACE_ERR_ARG;
    const Net& n = *np;
    Walk k;
    Carve cv;
    if (!plan(n, B, H, W, &k, &cv)) return USPACE_ERR_ARG;
    if (ws_bytes < cv.bytes()) return USPACE_ERR_WORKSPACE;
    double* part = (double*)ws;
    double* layer = part + cv.part_doubles;
    float* xin = (float*)(layer + cv.layer_doubles);
    float* bufs[2] = {xin + cv.in_floats, xin + cv.in_floats + cv.act_floats};
    if (per_layer) layer = per_layer;
    const float* wts = (const float*)blob;
    const int N = 2 * B, HW = H * W;
    {
        const long half = (long)B * HW;
        const unsigned blocks = (unsigned)((half + 255) / 256);
        hipLaunchKernelGGL(scale_input_kernel, dim3(blocks), dim3(256), 0, st, x0, xin, half, HW, normalize);
        US_CHECK_LAUNCH();
        hipLaunchKernelGGL(scale_input_kernel, dim3(blocks), dim3(256), 0, st, x1, xin + half * 3, half, HW, normalize);
        US_CHECK_LAUNCH();
    }
    const float* cur = xin;
    int h = H, w = W, c = 3, nb = 0;
    for (int l = 0; l < last; ++l) {
        for (const Op& op : n.stage[l]) {
            float* y = bufs[nb];
            nb ^= 1;
            if (op.kind == OP_CONV) {
                const ConvSpec& s = n.convs[op.conv];
                if (s.cin != c) return USPACE_ERR_ARG;
                US_TRY(conv_f32_launch(s, cur, N, h, w, wts + n.w_off[op.conv], wts + n.b_off[op.conv], y, s.cout, 0, st, &h, &w));
                c = s.cout;
            } else if (op.kind == OP_POOL3) {
                US_TRY(pool3_launch(cur, N, h, w, c, true, 2, 0, y, c, 0, st, &h, &w));
            } else {
                const int ho = h / 2, wo = w / 2;
                const long cnt = (long)N * ho * wo * (c / 4);
                hipLaunchKernelGGL(pool2_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, cur, y, N, h, w, c, ho, wo);
                US_CHECK_LAUNCH();
                h = ho;
                w = wo;
            }
            cur = y;
        }
        if (h != k.h[l] || w != k.w[l] || c != n.tap_c[l]) return USPACE_ERR_ARG;      // the walk sized the workspace
        if (!dump)
            US_TRY(head_launch(cur, cur + (size_t)B * h * w * c, wts + n.lin_off[l], B, h * w, c, part, layer + (size_t)l * B, st));
    }
    if (dump) {
        const size_t bytes = (size_t)N * h * w * c * sizeof(float);
        if (hipMemcpyAsync(dump, cur, bytes, hipMemcpyDeviceToDevice, st) != hipSuccess) return USPACE_ERR_LAUNCH;
        return USPACE_OK;
    }
    hipLaunchKernelGGL(lpips_total_kernel, dim3(us_cdiv(B, 256)), dim3(256), 0, st, layer, out, B);
    US_CHECK_LAUNCH();
    return USPACE_OK;
}

}  // namespace

extern "C" int uspace_lpips_num_params(int net) {
    const Net* n = net_of(net);
    return n ? n->t.n_params : USPACE_ERR_ARG;
}

extern "C" long uspace_lpips_param_numel(int net, int index) {
    const Net* n = net_of(net);
    return n ? n->t.numel(index) : USPACE_ERR_ARG;
}

extern "C" size_t uspace_lpips_weight_bytes(int net) {
    const Net* n = net_of(net);
    return n ? n->t.bytes() : 0;
}

extern "C" size_t uspace_lpips_workspace_bytes(int net, int B, int H, int W) {
    const Net* n = net_of(net);
    Walk k;
    Carve c;
    if (!n || !plan(*n, B, H, W, &k, &c)) return 0;
    return c.bytes();
}

extern "C" int uspace_lpips_pack_weights(int net, const float* const* params, int n_params, void* blob, size_t blob_bytes,
                                         uspace_stream_t stream) {
    const Net* n = net_of(net);
    if (!n) return USPACE_ERR_ARG;
    US_TRY(us_pack_table(n->t, params, n_params, blob, blob_bytes, stream));      // the checks and the lin vectors
    float* out = (float*)blob;
    for (size_t i = 0; i < n->convs.size(); ++i)
        US_TRY(conv_f32_pack(n->convs[i], params[n->i_w[i]], ConvPackSource::with_bias(params[n->i_w[i] + 1]), out + n->w_off[i],
                             out + n->b_off[i], (hipStream_t)stream));
    return USPACE_OK;
}

extern "C" int uspace_lpips_forward(int net, const void* blob, void* workspace, size_t workspace_bytes, const float* x0,
                                    const float* x1, int B, int H, int W, int normalize, double* out, double* per_layer,
                                    uspace_stream_t stream) {
    if (!out) return USPACE_ERR_ARG;
    return run(net, blob, workspace, workspace_bytes, x0, x1, B, H, W, normalize, kNumTaps, nullptr, out, per_layer,
               (hipStream_t)stream);
}

extern "C" int uspace_lpips_tap(int net, const void* blob, void* workspace, size_t workspace_bytes, const float* x0, const float* x1,
                                int B, int H, int W, int normalize, int stage, float* dump, uspace_stream_t stream) {
    if (!dump) return USPACE_ERR_ARG;
    return run(net, blob, workspace, workspace_bytes, x0, x1, B, H, W, normalize, stage, dump, nullptr, nullptr, (hipStream_t)stream);
}

extern "C" size_t uspace_lpips_distance_workspace_bytes(int B, int HW, int C) {
    if (!head_args_ok(B, HW, C)) return 0;
    return (size_t)B * head_chunks(HW) * sizeof(double);
}

extern "C" int uspace_lpips_distance_f64(const float* f0, const float* f1, const float* w, int B, int HW, int C, void* workspace,
                                         size_t workspace_bytes, double* out, uspace_stream_t stream) {
    if (!f0 || !f1 || !w || !workspace || !out || !head_args_ok(B, HW, C)) return USPACE_ERR_ARG;
    if (workspace_bytes < uspace_lpips_distance_workspace_bytes(B, HW, C)) return USPACE_ERR_WORKSPACE;
    return head_launch(f0, f1, w, B, HW, C, (double*)workspace, out, (hipStream_t)stream);
}

extern "C" size_t uspace_ssim_workspace_bytes(int B, int C, int H, int W) {
    if (!ssim_args_ok(B, C, H, W)) return 0;
    return (size_t)B * C * ssim_tiles(H, W) * sizeof(double);
}

extern "C" int uspace_ssim_f64(const float* x, const float* y, int B, int C, int H, int W, double data_range, void* workspace,
                               size_t workspace_bytes, double* out, uspace_stream_t stream) {
    if (!x || !y || !workspace || !out || !ssim_args_ok(B, C, H, W) || !(data_range > 0.0)) return USPACE_ERR_ARG;
    if (workspace_bytes < uspace_ssim_workspace_bytes(B, C, H, W)) return USPACE_ERR_WORKSPACE;
    SsimWindow win;
    double g[kWin], sum = 0.0;
    for (int i = 0; i < kWin; ++i) {
        const double d = i - kWin / 2;
        g[i] = exp(-d * d / (2.0 * 1.5 * 1.5));
        sum += g[i];
    }
    for (int i = 0; i < kWin; ++i) win.g[i] = (float)(g[i] / sum);
    const double c1 = (0.01 * data_range) * (0.01 * data_range), c2 = (0.03 * data_range) * (0.03 * data_range);
    const int Ho = H - kWin + 1, Wo = W - kWin + 1;
    const int tiles_x = us_cdiv(Wo, kTile);
    const long tiles = ssim_tiles(H, W);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(ssim_kernel, dim3((unsigned)tiles, C, B), dim3(256), 0, st, x, y, (double*)workspace, H, W, tiles_x, win,
                       (float)c1, (float)c2);
    US_CHECK_LAUNCH();
    hipLaunchKernelGGL(ssim_finish_kernel, dim3(B), dim3(64), 0, st, (const double*)workspace, out, (long)C * tiles,
                       (double)C * Ho * Wo);
    US_CHECK_LAUNCH();
    return USPACE_OK;
}

extern "C" size_t uspace_psnr_workspace_bytes(int B, long n_per_image) {
    if (!psnr_args_ok(B, n_per_image)) return 0;
    return (size_t)B * ((n_per_image + kPsnrChunk - 1) / kPsnrChunk) * sizeof(double);
}

extern "C" int uspace_psnr_f64(const float* x, const float* y, int B, long n_per_image, double data_range, void* workspace,
                               size_t workspace_bytes, double* out, uspace_stream_t stream) {
    if (!x || !y || !workspace || !out || !psnr_args_ok(B, n_per_image) || !(data_range > 0.0)) return USPACE_ERR_ARG;
    if (workspace_bytes < uspace_psnr_workspace_bytes(B, n_per_image)) return USPACE_ERR_WORKSPACE;
    const long nchunk = (n_per_image + kPsnrChunk - 1) / kPsnrChunk;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(psnr_sse_kernel, dim3((unsigned)nchunk, B), dim3(256), 0, st, x, y, (double*)workspace, n_per_image);
    US_CHECK_LAUNCH();
    hipLaunchKernelGGL(psnr_finish_kernel, dim3(B), dim3(64), 0, st, (const double*)workspace, out, nchunk, n_per_image,
                       data_range * data_range);
    US_CHECK_LAUNCH();
    return USPACE_OK;
}
