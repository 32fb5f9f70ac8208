// ArcFace identity tower on gfx950: Backbone(input_size, num_layers, mode) of TreB1eN's InsightFace_Pytorch model_irse.py in eval
// mode (IR-SE50 is the network behind the ID similarity of pSp / e4e), the preprocessing in front of it and the fp64 dot product
// of two embeddings.
//
// Activations are NHWC fp32 in the caller's workspace; every convolution is the fp32-MFMA implicit GEMM of conv_f32.h (a
// k-ordered fp32 fma chain per output).  Folded at pack time, in fp64 and rounded once: every batch norm that FOLLOWS a
// convolution or the Linear (input_layer.1, res_layer.4, shortcut_layer.1, output_layer.4) and output_layer.0, which precedes the
// Linear with no padding in between.  NOT folded: res_layer.0, the batch norm in front of a unit's first 3 x 3 convolution -- the
// reference zero-pads the normalised map, so a folded shift would leak through the padding into every border pixel.  It is
// applied to in-bounds operands only: an elementwise pass writes the operand map, which the convolution then pads with zeros
// (the other form, the affine map in the convolution's A-operand load, measured 14 % slower over the tower: profiles/id_metrics.md).
// One unit:
//   t1 = PReLU(conv3x3(BN(x)))   t2 = conv3x3_stride(t1) (+ folded BN)   gate = sigmoid(fc2 relu(fc1 mean_pixels(t2)))
//   out = t2 * gate + shortcut,  shortcut = x[:, ::s, ::s] (in == depth) or the folded strided 1 x 1 convolution.
//
// Every sum has one fixed order that neither B nor the sample's place in the batch changes: the SE mean is per-workgroup fp64
// partial sums over a constant number of pixels, then one wave per sample; the head's K = 512 hw sum is fp32 fma chains over a
// constant number of channels of one pixel, joined in chunk order.  No atomics.  Nothing of a workspace is read before it is written.
#include <math.h>

#include <algorithm>
#include <vector>

#include "blob.h"
#include "common.h"
#include "conv_f32.h"

namespace {

constexpr double kBnEps = 1e-5;
constexpr int kWidth[4] = {64, 128, 256, 512};
constexpr int kEmb = 512;
constexpr int kSePix = 64;        // pixels per partial sum of the SE mean (a constant of the summation order)
constexpr int kHeadCh = 128;      // channels per partial sum of the head (likewise)
constexpr int kHeadB = 8;         // samples per workgroup of the head

// ------------------------------------------------------------------------------------------------ the network and its blob
struct Unit {
    int cin, d, s;
    bool conv_sc;
    // blob offsets in floats
    size_t pre_s, pre_b, w1, slope, w2, b2, wsc, bsc, fc1, fc2;
    // parameter indices: the weights of the shortcut convolution and of the two 3 x 3 convolutions (the batch norm after i_sc and
    // i_w2 is the next four parameters), res_layer.0's batch norm (four)
    int i_sc, i_pre, i_w1, i_w2;
};
struct Net {
    int S, se, side;              // input side; SE modules present; side of the last map (S / 16)
    std::vector<Unit> units;
    size_t in_w, in_b, in_slope, zeros, head_w, head_b;
    int i_in, i_head;             // input_layer's convolution (its batch norm follows); output_layer's ten parameters
    ParamTable t;                 // the caller's parameters in state-dict order (num_batches_tracked left out)
};

// The blob, piece by piece in the order the pieces lie in it, and beside each piece the parameters it is made from.  Convolutions,
// batch norms and the output layer are P_OWNER: uspace_idnet_pack_weights folds them into the pieces taken here.
bool make_net(const uspace_idnet_config* cfg, Net* out) {
    if (!cfg || cfg->input_size < 16 || cfg->input_size % 16 || cfg->input_size > 4096) return false;
    for (int l = 0; l < 4; ++l)
        if (cfg->blocks[l] < 1 || cfg->blocks[l] > 4096) return false;
    if (cfg->se != 0 && cfg->se != 1) return false;
    Net n;
    n.S = cfg->input_size;
    n.se = cfg->se;
    n.side = n.S / 16;
    ParamTable& t = n.t;
    auto take = [&](size_t floats) { return t.arena.take(floats * sizeof(float)) / sizeof(float); };
    auto copied = [&](long numel) { return t.at(t.add(numel, P_F32)) / sizeof(float); };
    auto own = [&](long numel) { return t.add(numel, P_OWNER); };
    auto own_bn = [&](int c) {
        const int i = own(c);
        for (int j = 1; j < 4; ++j) own(c);
        return i;
    };
    const ConvSpec in_conv{3, 64, 3, 3, 1, 1, 1};
    n.in_w = take((size_t)conv_kpad(in_conv) * 64);
    n.in_b = take(64);
    n.i_in = own(64 * 27);
    own_bn(64);
    n.in_slope = copied(64);
    n.zeros = take(kEmb);
    const long K = (long)kEmb * n.side * n.side;
    n.head_w = take((size_t)K * kEmb);
    n.head_b = take(kEmb);
    n.i_head = own_bn(512);
    own(K * kEmb);
    own(kEmb);
    own_bn(kEmb);
    for (int l = 0; l < 4; ++l)
        for (int j = 0; j < cfg->blocks[l]; ++j) {
            Unit u{};
            u.d = kWidth[l];
            u.cin = j ? u.d : (l ? kWidth[l - 1] : 64);
            u.s = j ? 1 : 2;
            u.conv_sc = u.cin != u.d;
            const int r = u.d / 16;
            if (u.conv_sc) {
                u.wsc = take((size_t)u.cin * u.d);
                u.bsc = take(u.d);
                u.i_sc = own((long)u.d * u.cin);
                own_bn(u.d);
            }
            u.pre_s = take(u.cin);
            u.pre_b = take(u.cin);
            u.i_pre = own_bn(u.cin);
            u.w1 = take((size_t)9 * u.cin * u.d);
            u.i_w1 = own((long)u.d * u.cin * 9);
            u.slope = copied(u.d);
            u.w2 = take((size_t)9 * u.d * u.d);
            u.b2 = take(u.d);
            u.i_w2 = own((long)u.d * u.d * 9);
            own_bn(u.d);
            if (n.se) {
                u.fc1 = copied((long)r * u.d);
                u.fc2 = copied((long)u.d * r);
            }
            n.units.push_back(u);
        }
    *out = std::move(n);
    return true;
}

// What one unit needs of each workspace role for B maps of H x W (floats; se_part in doubles)
struct Need {
    size_t x = 0, pre = 0, t1 = 0, t2 = 0, se_part = 0;
    void max_with(const Need& o) {
        x = std::max(x, o.x), pre = std::max(pre, o.pre), t1 = std::max(t1, o.t1), t2 = std::max(t2, o.t2);
        se_part = std::max(se_part, o.se_part);
    }
};
inline int out_side(int h, int s) { return (h - 1) / s + 1; }     // 3 x 3 pad 1 and 1 x 1 pad 0 alike
Need unit_need(const Unit& u, size_t B, int H, int W) {
    const size_t ho = out_side(H, u.s), wo = out_side(W, u.s);
    Need n;
    n.x = B * ho * wo * u.d;
    n.pre = B * H * W * u.cin;
    n.t1 = B * H * W * u.d;
    n.t2 = B * ho * wo * u.d;
    n.se_part = B * us_cdiv((int)(ho * wo), kSePix) * u.d;
    return n;
}

struct Carve {
    size_t head_part, off_x[2], off_pre, off_t1, off_t2, off_sc, off_se, off_gate, off_head, off_vec, bytes;
};
bool carve(const Need& need, size_t B, size_t head_parts, Carve* c) {
    // every tensor stays below 2^31 elements: the convolution counts pixels in int
    const size_t lim = (size_t)1 << 31;
    if (need.x >= lim || need.pre >= lim || need.t1 >= lim || need.t2 >= lim) return false;
    Arena ar;
    c->head_part = B * head_parts * kEmb;
    c->off_x[0] = ar.take(need.x * sizeof(float));
    c->off_x[1] = ar.take(need.x * sizeof(float));
    c->off_pre = ar.take(need.pre * sizeof(float));
    c->off_t1 = ar.take(need.t1 * sizeof(float));
    c->off_t2 = ar.take(need.t2 * sizeof(float));
    c->off_sc = ar.take(need.t2 * sizeof(float));
    c->off_se = ar.take(need.se_part * sizeof(double));
    c->off_gate = ar.take(B * kEmb * sizeof(float));
    c->off_head = ar.take(c->head_part * sizeof(float));
    c->off_vec = ar.take(B * kEmb * sizeof(float));
    c->bytes = ar.off;
    return true;
}
int head_parts(const Net& n) { return n.side * n.side * (kEmb / kHeadCh); }

bool plan(const Net& n, int B, Carve* c) {
    if (B < 1 || B > 32767) return false;
    Need need;
    need.x = (size_t)B * n.S * n.S * 64;      // input_layer's output
    int h = n.S;
    for (const Unit& u : n.units) {
        need.max_with(unit_need(u, B, h, h));
        h = out_side(h, u.s);
    }
    return carve(need, B, head_parts(n), c);
}

// ------------------------------------------------------------------------------------------------ pack kernels
// an eval-mode batch norm as y = x s_c + t_c
__global__ __launch_bounds__(256) void idnet_bn_affine_kernel(const float* __restrict__ gamma, const float* __restrict__ beta,
                                                              const float* __restrict__ mean, const float* __restrict__ var,
                                                              float* __restrict__ s_out, float* __restrict__ t_out, int C) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const double s = (double)gamma[c] / sqrt((double)var[c] + kBnEps);
    s_out[c] = (float)s;
    t_out[c] = (float)((double)beta[c] - (double)mean[c] * s);
}

// The head: out_n = BN1d(Linear(flatten_cyx(BN2d(x)))) as one matrix and one bias.  bn0 / bn1: gamma, beta, mean, var.
// wout[(p * 512 + c) * 512 + n] = W[n][c * hw + p] * s0_c * s1_n      (the (c, y, x) flatten permuted to (y, x, c))
__global__ __launch_bounds__(256) void idnet_pack_head_w_kernel(const float* __restrict__ w, const float* __restrict__ g0,
                                                                const float* __restrict__ v0, const float* __restrict__ g1,
                                                                const float* __restrict__ v1, float* __restrict__ wout, int hw) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)hw * kEmb * kEmb) return;
    const int n = (int)(idx % kEmb);
    const long pc = idx / kEmb;
    const int c = (int)(pc % kEmb), p = (int)(pc / kEmb);
    const double s0 = (double)g0[c] / sqrt((double)v0[c] + kBnEps), s1 = (double)g1[n] / sqrt((double)v1[n] + kBnEps);
    wout[idx] = (float)((double)w[(long)n * kEmb * hw + (long)c * hw + p] * s0 * s1);
}
// bout[n] = (b_n + sum_k W[n][k] t0_{c(k)}) s1_n + t1_n; one wave per n, 64 lane-strided fp64 chains joined by a butterfly
__global__ __launch_bounds__(64) void idnet_pack_head_b_kernel(const float* __restrict__ w, const float* __restrict__ b,
                                                               const float* __restrict__ g0, const float* __restrict__ b0,
                                                               const float* __restrict__ m0, const float* __restrict__ v0,
                                                               const float* __restrict__ g1, const float* __restrict__ b1,
                                                               const float* __restrict__ m1, const float* __restrict__ v1,
                                                               float* __restrict__ bout, int hw) {
    const int n = blockIdx.x;
    const long K = (long)kEmb * hw;
    double s = 0.0;
    for (long k = threadIdx.x; k < K; k += 64) {
        const int c = (int)(k / hw);
        const double s0 = (double)g0[c] / sqrt((double)v0[c] + kBnEps);
        s += (double)w[(long)n * K + k] * ((double)b0[c] - (double)m0[c] * s0);
    }
    s = wave_sum_f64(s);
    if (threadIdx.x == 0) {
        const double s1 = (double)g1[n] / sqrt((double)v1[n] + kBnEps);
        bout[n] = (float)(((double)b[n] + s) * s1 + ((double)b1[n] - (double)m1[n] * s1));
    }
}

// ------------------------------------------------------------------------------------------------ forward kernels
// y = x s_c + t_c over an NHWC map, 4 channels per thread (the batch norm in front of a unit's first convolution)
__global__ __launch_bounds__(256) void idnet_bn_apply_kernel(const float* __restrict__ x, const float* __restrict__ s,
                                                             const float* __restrict__ t, float* __restrict__ y, long n4, int C4) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n4) return;
    const int c = (int)(idx % C4) * 4;
    const f32x4 v = *(const f32x4*)(x + idx * 4), sc = *(const f32x4*)(s + c), sh = *(const f32x4*)(t + c);
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = fmaf(v[j], sc[j], sh[j]);
    *(f32x4*)(y + idx * 4) = o;
}

// part[b, chunk, c] = the fp64 sum of t [B, HW, C] over the chunk's kSePix pixels in pixel order; a thread owns channels
__global__ __launch_bounds__(256) void idnet_se_partial_kernel(const float* __restrict__ t, double* __restrict__ part, int HW, int C,
                                                               int nchunk) {
    const int b = blockIdx.y, chunk = blockIdx.x;
    const int p0 = chunk * kSePix, p1 = min(p0 + kSePix, HW);
    const float* tb = t + (size_t)b * HW * C;
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        double s = 0.0;
        for (int p = p0; p < p1; ++p) s += (double)tb[(size_t)p * C + c];
        part[((size_t)b * nchunk + chunk) * C + c] = s;
    }
}

// One wave per sample: mean_c (the partials in chunk order) -> h_j = relu(sum_c fc1[j, c] mean_c), a wave-level dot product per
// output -> gate_c = sigmoid(sum_j fc2[c, j] h_j), the R <= 32 terms in j order per lane.
__global__ __launch_bounds__(64) void idnet_se_gate_kernel(const double* __restrict__ part, const float* __restrict__ fc1,
                                                           const float* __restrict__ fc2, float* __restrict__ gate, int HW, int C,
                                                           int nchunk) {
    __shared__ float mean[kEmb];
    __shared__ float hid[kEmb / 16];
    const int b = blockIdx.x, lane = threadIdx.x, R = C / 16;
    for (int c = lane; c < C; c += 64) {
        double s = 0.0;
        for (int j = 0; j < nchunk; ++j) s += part[((size_t)b * nchunk + j) * C + c];
        mean[c] = (float)(s / (double)HW);
    }
    __syncthreads();
    for (int j = 0; j < R; ++j) {
        float t = 0.f;
        for (int c = lane; c < C; c += 64) t = fmaf(fc1[(size_t)j * C + c], mean[c], t);
        t = wave_sum(t);
        if (lane == 0) hid[j] = fmaxf(t, 0.f);
    }
    __syncthreads();
    for (int c = lane; c < C; c += 64) {
        float t = 0.f;
        for (int j = 0; j < R; ++j) t = fmaf(fc2[(size_t)c * R + j], hid[j], t);
        gate[(size_t)b * C + c] = 1.f / (1.f + expf(-t));
    }
}

// out = t2 * gate + shortcut over [B, Ho, Wo, C], 4 channels per thread.  sc != NULL: the shortcut convolution's map;
// otherwise the subsample x[b, oy s, ox s, c] of the unit's input x [B, H, W, C].  gate == NULL (mode "ir"): out = t2 + shortcut.
__global__ __launch_bounds__(256) void idnet_combine_kernel(const float* __restrict__ t2, const float* __restrict__ gate,
                                                            const float* __restrict__ sc, const float* __restrict__ x,
                                                            float* __restrict__ out, int B, int H, int W, int Ho, int Wo, int C,
                                                            int s) {
    const int C4 = C >> 2;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)B * Ho * Wo * C4) return;
    const int c = (int)(idx % C4) * 4;
    const long pix = idx / C4;
    const int b = (int)(pix / ((long)Ho * Wo));
    const f32x4 v = *(const f32x4*)(t2 + pix * C + c);
    f32x4 r;
    if (sc) {
        r = *(const f32x4*)(sc + pix * C + c);
    } else {
        const int q = (int)(pix - (long)b * Ho * Wo);
        const int oy = q / Wo, ox = q - oy * Wo;                   // oy s <= H - 1 and ox s <= W - 1 by Ho = (H - 1) / s + 1
        r = *(const f32x4*)(x + (((long)b * H + (long)oy * s) * W + (long)ox * s) * C + c);
    }
    f32x4 o;
    if (gate) {
        const f32x4 g = *(const f32x4*)(gate + (size_t)b * C + c);
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = fmaf(v[j], g[j], r[j]);
    } else {
        o = v + r;
    }
    *(f32x4*)(out + pix * C + c) = o;
}

// The head's partial sums: x [B, hw, 512] NHWC, w [hw, 512, 512] (pixel, channel, output).  Workgroup (part, sample group):
// part = (pixel p, quarter q of the channels); part_out[b, part, n] = the fp32 fma chain over the kHeadCh channels in order.
// A thread owns outputs tid and tid + 256 for the group's kHeadB samples.
__global__ __launch_bounds__(256) void idnet_head_partial_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                 float* __restrict__ part_out, int B, int hw, int nparts) {
    __shared__ float xs[kHeadB][kHeadCh];
    const int tid = threadIdx.x, part = blockIdx.x, b0 = blockIdx.y * kHeadB;
    const int p = part / (kEmb / kHeadCh), c0 = (part % (kEmb / kHeadCh)) * kHeadCh;
    for (int i = tid; i < kHeadB * kHeadCh; i += 256) {
        const int bb = i / kHeadCh, cc = i - bb * kHeadCh;
        xs[bb][cc] = b0 + bb < B ? x[((size_t)(b0 + bb) * hw + p) * kEmb + c0 + cc] : 0.f;
    }
    __syncthreads();
    float acc0[kHeadB], acc1[kHeadB];
#pragma unroll
    for (int bb = 0; bb < kHeadB; ++bb) acc0[bb] = acc1[bb] = 0.f;
    const float* wp = w + ((size_t)p * kEmb + c0) * kEmb;
#pragma unroll 4
    for (int cc = 0; cc < kHeadCh; ++cc) {
        const float w0 = wp[(size_t)cc * kEmb + tid], w1 = wp[(size_t)cc * kEmb + tid + 256];
#pragma unroll
        for (int bb = 0; bb < kHeadB; ++bb) {
            acc0[bb] = fmaf(xs[bb][cc], w0, acc0[bb]);
            acc1[bb] = fmaf(xs[bb][cc], w1, acc1[bb]);
        }
    }
#pragma unroll
    for (int bb = 0; bb < kHeadB; ++bb)
        if (b0 + bb < B) {
            float* o = part_out + ((size_t)(b0 + bb) * nparts + part) * kEmb;
            o[tid] = acc0[bb];
            o[tid + 256] = acc1[bb];
        }
}

// vec[b, n] = (the partials in part order) + bias_n; emb[b, :] = vec / |vec| (the norm: 64 lane-strided fp32 chains over n joined
// by a butterfly; a division, no eps, as the reference's l2_norm).  emb == NULL: vec alone.
__global__ __launch_bounds__(256) void idnet_head_finish_kernel(const float* __restrict__ part, const float* __restrict__ bias,
                                                                float* __restrict__ vec, float* __restrict__ emb, int nparts) {
    __shared__ float v[kEmb];
    __shared__ float norm;
    const int b = blockIdx.x, tid = threadIdx.x;
    for (int n = tid; n < kEmb; n += 256) {
        float s = 0.f;
        for (int j = 0; j < nparts; ++j) s += part[((size_t)b * nparts + j) * kEmb + n];
        s += bias[n];
        v[n] = s;
        vec[(size_t)b * kEmb + n] = s;
    }
    if (!emb) return;
    __syncthreads();
    if (tid < 64) {
        float s = 0.f;
        for (int n = tid; n < kEmb; n += 64) s = fmaf(v[n], v[n], s);
        s = wave_sum(s);
        if (tid == 0) norm = sqrtf(s);
    }
    __syncthreads();
    for (int n = tid; n < kEmb; n += 256) emb[(size_t)b * kEmb + n] = v[n] / norm;
}

// out[b] = sum_k ea[b, k] eb[b, k], products and sum in fp64, in k order: one thread per pair
__global__ __launch_bounds__(64) void idnet_similarity_kernel(const float* __restrict__ ea, const float* __restrict__ eb,
                                                              double* __restrict__ out, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double s = 0.0;
    for (int k = 0; k < kEmb; ++k) s = fma((double)ea[(size_t)b * kEmb + k], (double)eb[(size_t)b * kEmb + k], s);
    out[b] = s;
}

// ---- preprocess.  Adaptive average pooling: output index i of O averages inputs floor(i N / O) .. ceil((i + 1) N / O) - 1.
__device__ __forceinline__ int pool_lo(int i, int N, int O) { return (int)(((long)i * N) / O); }
__device__ __forceinline__ int pool_hi(int i, int N, int O) { return (int)((((long)i + 1) * N + O - 1) / O); }   // exclusive

// One thread per output pixel.  crop: the value at (Y, X) of the 256 x 256 map is the input pixel itself (H == W == 256) or its
// window mean of the H x W input; the output averages rows 35 + window and columns 32 + window of the 188 x 188 crop.
// Without crop the output averages its window of the input.  Every window sum is fp32 in row-major order, then / count.
__global__ __launch_bounds__(256) void idnet_preprocess_kernel(const float* __restrict__ x, float* __restrict__ out, int B, int H, int W,
                                                               int normalize, int crop, int O) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)B * O * O) return;
    const int b = (int)(idx / ((long)O * O));
    const int r = (int)(idx - (long)b * O * O);
    const int oy = r / O, ox = r - oy * O;
    const bool pool256 = crop && !(H == 256 && W == 256);
    const int NY = crop ? 188 : H, NX = crop ? 188 : W, offy = crop ? 35 : 0, offx = crop ? 32 : 0;
    const int y0 = offy + pool_lo(oy, NY, O), y1 = offy + pool_hi(oy, NY, O);
    const int x0 = offx + pool_lo(ox, NX, O), x1 = offx + pool_hi(ox, NX, O);
    for (int c = 0; c < 3; ++c) {
        const float* xc = x + ((size_t)b * 3 + c) * H * W;
        float s = 0.f;
        for (int Y = y0; Y < y1; ++Y)
            for (int X = x0; X < x1; ++X) {
                float v;
                if (pool256) {
                    const int iy0 = pool_lo(Y, H, 256), iy1 = pool_hi(Y, H, 256), ix0 = pool_lo(X, W, 256), ix1 = pool_hi(X, W, 256);
                    float t = 0.f;
                    for (int iy = iy0; iy < iy1; ++iy)
                        for (int ix = ix0; ix < ix1; ++ix) {
                            const float u = xc[(size_t)iy * W + ix];
                            t += normalize ? 2.f * u - 1.f : u;
                        }
                    v = t / (float)((iy1 - iy0) * (ix1 - ix0));
                } else {
                    const float u = xc[(size_t)Y * W + X];
                    v = normalize ? 2.f * u - 1.f : u;
                }
                s += v;
            }
        out[idx * 3 + c] = s / (float)((y1 - y0) * (x1 - x0));
    }
}

// ------------------------------------------------------------------------------------------------ the forward
struct Bufs {
    float *pre, *t1, *t2, *sc, *gate;
    double* se;
};

// One unit on x [B, H, W, cin] -> out [B, Ho, Wo, d]
int run_unit(const Net& n, const Unit& u, const float* wts, const float* x, int B, int H, int W, const Bufs& bf, float* out,
             hipStream_t st, int* Ho, int* Wo) {
    const ConvSpec c1{u.cin, u.d, 3, 3, 1, 1, 1}, c2{u.d, u.d, 3, 3, u.s, 1, 1}, cs{u.cin, u.d, 1, 1, u.s, 0, 0};
    int h1, w1, ho, wo;
    const long n4 = (long)B * H * W * (u.cin / 4);
    hipLaunchKernelGGL(idnet_bn_apply_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, x, wts + u.pre_s, wts + u.pre_b, bf.pre,
                       n4, u.cin / 4);
    US_CHECK_LAUNCH();
    US_TRY(conv_f32_launch<CONV_EPI_PRELU>(c1, bf.pre, B, H, W, wts + u.w1, wts + n.zeros, bf.t1, u.d, 0, st, &h1, &w1, wts + u.slope));
    US_TRY(conv_f32_launch<CONV_EPI_BIAS>(c2, bf.t1, B, h1, w1, wts + u.w2, wts + u.b2, bf.t2, u.d, 0, st, &ho, &wo));
    const float* sc = nullptr;
    if (u.conv_sc) {
        int hs, ws_;
        US_TRY(conv_f32_launch<CONV_EPI_BIAS>(cs, x, B, H, W, wts + u.wsc, wts + u.bsc, bf.sc, u.d, 0, st, &hs, &ws_));
        if (hs != ho || ws_ != wo) return USPACE_ERR_ARG;
        sc = bf.sc;
    }
    const float* gate = nullptr;
    if (n.se) {
        const int hw = ho * wo, nchunk = us_cdiv(hw, kSePix);
        hipLaunchKernelGGL(idnet_se_partial_kernel, dim3(nchunk, B), dim3(std::min(u.d, 256)), 0, st, bf.t2, bf.se, hw, u.d, nchunk);
        US_CHECK_LAUNCH();
        hipLaunchKernelGGL(idnet_se_gate_kernel, dim3(B), dim3(64), 0, st, bf.se, wts + u.fc1, wts + u.fc2, bf.gate, hw, u.d, nchunk);
        US_CHECK_LAUNCH();
        gate = bf.gate;
    }
    const long cnt = (long)B * ho * wo * (u.d / 4);
    hipLaunchKernelGGL(idnet_combine_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, bf.t2, gate, sc, x, out, B, H, W, ho,
                       wo, u.d, u.s);
    US_CHECK_LAUNCH();
    *Ho = ho;
    *Wo = wo;
    return USPACE_OK;
}

Bufs bufs_of(char* base, const Carve& cv) {
    return Bufs{(float*)(base + cv.off_pre), (float*)(base + cv.off_t1), (float*)(base + cv.off_t2), (float*)(base + cv.off_sc),
                (float*)(base + cv.off_gate), (double*)(base + cv.off_se)};
}

// Stages 0 (input_layer) .. 1 + u (unit u) .. 1 + U (the 512-vector before the l2 normalisation).  dump != NULL: stage `last`
// is copied there and nothing later runs; dump == NULL: the whole tower runs (`last` is ignored) and emb receives the unit embeddings.
int run(const uspace_idnet_config* cfg, const void* blob, void* ws, size_t ws_bytes, const float* x, int B, int last, float* dump,
        float* emb, hipStream_t st) {
    Net n;
    if (!make_net(cfg, &n) || !blob || !ws || !x) return USPACE_ERR_ARG;
    const int U = (int)n.units.size();
    if (!dump) last = U + 1;
    if (last < 0 || last > U + 1) return USPACE_ERR_ARG;
    Carve cv;
    if (!plan(n, B, &cv)) return USPACE_ERR_ARG;
    if (ws_bytes < cv.bytes) return USPACE_ERR_WORKSPACE;
    char* base = (char*)ws;
    float* xb[2] = {(float*)(base + cv.off_x[0]), (float*)(base + cv.off_x[1])};
    const Bufs bf = bufs_of(base, cv);
    const float* wts = (const float*)blob;
    int h, w, cur = 0, c = 64;
    US_TRY(conv_f32_launch<CONV_EPI_PRELU>(ConvSpec{3, 64, 3, 3, 1, 1, 1}, x, B, n.S, n.S, wts + n.in_w, wts + n.in_b, xb[0], 64, 0, st,
                                           &h, &w, wts + n.in_slope));
    for (int u = 0; u < U && u < last; ++u) {
        US_TRY(run_unit(n, n.units[u], wts, xb[cur], B, h, w, bf, xb[cur ^ 1], st, &h, &w));
        cur ^= 1;
        c = n.units[u].d;
    }
    if (last <= U) {
        const size_t bytes = (size_t)B * h * w * c * sizeof(float);
        if (hipMemcpyAsync(dump, xb[cur], bytes, hipMemcpyDeviceToDevice, st) != hipSuccess) return USPACE_ERR_LAUNCH;
        return USPACE_OK;
    }
    if (h != n.side || w != n.side || c != kEmb) return USPACE_ERR_ARG;      // the plan sized the head
    const int nparts = head_parts(n);
    float* part = (float*)(base + cv.off_head);
    float* vec = dump ? dump : (float*)(base + cv.off_vec);
    hipLaunchKernelGGL(idnet_head_partial_kernel, dim3(nparts, us_cdiv(B, kHeadB)), dim3(256), 0, st, xb[cur], wts + n.head_w, part, B,
                       h * w, nparts);
    US_CHECK_LAUNCH();
    hipLaunchKernelGGL(idnet_head_finish_kernel, dim3(B), dim3(256), 0, st, part, wts + n.head_b, vec, dump ? nullptr : emb, nparts);
    US_CHECK_LAUNCH();
    return USPACE_OK;
}

}  // namespace

extern "C" int uspace_idnet_num_params(const uspace_idnet_config* cfg) {
    Net n;
    return make_net(cfg, &n) ? n.t.n_params : USPACE_ERR_ARG;
}

extern "C" long uspace_idnet_param_numel(const uspace_idnet_config* cfg, int index) {
    Net n;
    return make_net(cfg, &n) ? n.t.numel(index) : USPACE_ERR_ARG;
}

extern "C" size_t uspace_idnet_weight_bytes(const uspace_idnet_config* cfg) {
    Net n;
    return make_net(cfg, &n) ? n.t.bytes() : 0;
}

extern "C" size_t uspace_idnet_workspace_bytes(const uspace_idnet_config* cfg, int B) {
    Net n;
    Carve c;
    return make_net(cfg, &n) && plan(n, B, &c) ? c.bytes : 0;
}

extern "C" int uspace_idnet_pack_weights(const uspace_idnet_config* cfg, const float* const* params, int n_params, void* blob,
                                         size_t blob_bytes, uspace_stream_t stream) {
    Net n;
    if (!make_net(cfg, &n)) return USPACE_ERR_ARG;
    US_TRY(us_pack_table(n.t, params, n_params, blob, blob_bytes, stream));      // the checks; the PReLU slopes and the SE weights
    hipStream_t st = (hipStream_t)stream;
    float* out = (float*)blob;
    // a convolution with the batch norm after it (the four parameters behind its weight) folded in
    auto conv_bn = [&](const ConvSpec& c, int i_w, size_t w_off, size_t b_off) {
        return conv_f32_pack(c, params[i_w], ConvPackSource::batch_norm(params + i_w + 1, kBnEps), out + w_off, out + b_off, st);
    };
    if (hipMemsetAsync(out + n.zeros, 0, kEmb * sizeof(float), st) != hipSuccess) return USPACE_ERR_LAUNCH;
    US_TRY(conv_bn(ConvSpec{3, 64, 3, 3, 1, 1, 1}, n.i_in, n.in_w, n.in_b));
    {   // output_layer: BN2d (4), Linear weight, bias, BN1d (4)
        const float* const* p = params + n.i_head;
        const int hw = n.side * n.side;
        hipLaunchKernelGGL(idnet_pack_head_w_kernel, dim3((unsigned)(((long)hw * kEmb * kEmb + 255) / 256)), dim3(256), 0, st, p[4], p[0],
                           p[3], p[6], p[9], out + n.head_w, hw);
        US_CHECK_LAUNCH();
        hipLaunchKernelGGL(idnet_pack_head_b_kernel, dim3(kEmb), dim3(64), 0, st, p[4], p[5], p[0], p[1], p[2], p[3], p[6], p[7], p[8],
                           p[9], out + n.head_b, hw);
        US_CHECK_LAUNCH();
    }
    for (const Unit& u : n.units) {
        if (u.conv_sc) US_TRY(conv_bn(ConvSpec{u.cin, u.d, 1, 1, u.s, 0, 0}, u.i_sc, u.wsc, u.bsc));
        const float* const* pre = params + u.i_pre;
        hipLaunchKernelGGL(idnet_bn_affine_kernel, dim3(us_cdiv(u.cin, 256)), dim3(256), 0, st, pre[0], pre[1], pre[2], pre[3],
                           out + u.pre_s, out + u.pre_b, u.cin);
        US_CHECK_LAUNCH();
        US_TRY(conv_f32_pack(ConvSpec{u.cin, u.d, 3, 3, 1, 1, 1}, params[u.i_w1], ConvPackSource{}, out + u.w1, nullptr, st));
        US_TRY(conv_bn(ConvSpec{u.d, u.d, 3, 3, u.s, 1, 1}, u.i_w2, u.w2, u.b2));
    }
    return USPACE_OK;
}

extern "C" int uspace_idnet_preprocess(const float* x, int B, int H, int W, int normalize, int crop, int out_size, float* out,
                                       uspace_stream_t stream) {
    if (!x || !out || B < 1 || H < 1 || W < 1 || out_size < 1 || out_size > 4096 || H > 16384 || W > 16384) return USPACE_ERR_ARG;
    if ((size_t)B * 3 * H * W >= ((size_t)1 << 31) || (size_t)B * 3 * out_size * out_size >= ((size_t)1 << 31)) return USPACE_ERR_ARG;
    const long cnt = (long)B * out_size * out_size;
    hipLaunchKernelGGL(idnet_preprocess_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, out, B, H, W,
                       normalize ? 1 : 0, crop ? 1 : 0, out_size);
    US_CHECK_LAUNCH();
    return USPACE_OK;
}

extern "C" int uspace_idnet_forward(const uspace_idnet_config* cfg, const void* blob, void* workspace, size_t workspace_bytes,
                                    const float* x_nhwc, int B, float* emb, uspace_stream_t stream) {
    if (!emb) return USPACE_ERR_ARG;
    return run(cfg, blob, workspace, workspace_bytes, x_nhwc, B, 0, nullptr, emb, (hipStream_t)stream);
}

extern "C" int uspace_idnet_tap(const uspace_idnet_config* cfg, const void* blob, void* workspace, size_t workspace_bytes,
                                const float* x_nhwc, int B, int stage, float* dump, uspace_stream_t stream) {
    if (!dump) return USPACE_ERR_ARG;
    return run(cfg, blob, workspace, workspace_bytes, x_nhwc, B, stage, dump, nullptr, (hipStream_t)stream);
}

extern "C" size_t uspace_idnet_unit_workspace_bytes(const uspace_idnet_config* cfg, int unit, int B, int H, int W) {
    Net n;
    Carve c;
    if (!make_net(cfg, &n) || unit < 0 || unit >= (int)n.units.size() || B < 1 || B > 32767 || H < 1 || W < 1 || H > 4096 || W > 4096)
        return 0;
    return carve(unit_need(n.units[unit], B, H, W), B, 0, &c) ? c.bytes : 0;
}

extern "C" int uspace_idnet_unit(const uspace_idnet_config* cfg, const void* blob, void* workspace, size_t workspace_bytes, int unit,
                                 const float* x_nhwc, int B, int H, int W, float* out, uspace_stream_t stream) {
    Net n;
    Carve cv;
    if (!make_net(cfg, &n) || !blob || !workspace || !x_nhwc || !out || unit < 0 || unit >= (int)n.units.size() || B < 1 ||
        B > 32767 || H < 1 || W < 1 || H > 4096 || W > 4096)
        return USPACE_ERR_ARG;
    if (!carve(unit_need(n.units[unit], B, H, W), B, 0, &cv)) return USPACE_ERR_ARG;
    if (workspace_bytes < cv.bytes) return USPACE_ERR_WORKSPACE;
    int ho, wo;
    return run_unit(n, n.units[unit], (const float*)blob, x_nhwc, B, H, W, bufs_of((char*)workspace, cv), out,
                    (hipStream_t)stream, &ho, &wo);
}

extern "C" int uspace_idnet_similarity_f64(const float* ea, const float* eb, int B, double* out, uspace_stream_t stream) {
    if (!ea || !eb || !out || B < 1) return USPACE_ERR_ARG;
    hipLaunchKernelGGL(idnet_similarity_kernel, dim3(us_cdiv(B, 64)), dim3(64), 0, (hipStream_t)stream, ea, eb, out, B);
    US_CHECK_LAUNCH();
    return USPACE_OK;
}
