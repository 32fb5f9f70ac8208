// Attribute-classifier tower on gfx950: a torchvision-layout ResNet (BasicBlock or the "v1.5" Bottleneck, groups 1) in eval mode,
// the input normalisation in front of it and the fp64 edit-effect columns of tools/attr_metrics.py.
//
// Activations are NHWC fp32 in the caller's workspace; every convolution is the fp32-MFMA implicit GEMM of conv_f32.h (a
// k-ordered fp32 fma chain per output).  Every batch norm follows a convolution, so all of them are folded at pack time, in fp64
// and rounded once.  NOT folded: the input's (x - mean_c) / std_c -- the reference zero-pads the normalised image, so a shift
// folded into conv1 would leak through the padding into every border pixel (the remark about res_layer.0 at the top of
// idnet.hip); an elementwise kernel writes the normalised NHWC image, which conv1 then pads with zeros.
//   stem:        relu(bn1(conv1 7x7 s2 p3)) -> max pool 3x3 s2 p1 (floor mode)
//   BasicBlock:  relu(bn1(conv3x3_s)) -> bn2(conv3x3) ;  Bottleneck: relu(bn1(conv1x1)) -> relu(bn2(conv3x3_s)) -> bn3(conv1x1)
//   out = relu((branch + its folded shift) + shortcut), the last convolution's epilogue (CONV_EPI_ADD_RELU);
//   shortcut = x, or downsample.1(downsample.0 1x1_s) exactly when s != 1 or in != out
//   tail:        mean over the pixels -> fc with bias
//
// Every sum has one fixed order that neither B nor the sample's place in the batch changes: the pixel mean is per-workgroup fp64
// partial sums over a constant number of pixels, then one wave per sample; a logit is one fp32 fma chain over the features in
// order.  No atomics.  Nothing of a workspace is read before it is written.
#include <math.h>

#include <algorithm>
#include <vector>

#include "blob.h"
#include "common.h"
#include "conv_f32.h"

namespace {

constexpr double kBnEps = 1e-5;
constexpr int kMaxCh = 2048;
constexpr int kPoolPix = 64;      // pixels per partial sum of the pixel mean (a constant of the summation order)

// ------------------------------------------------------------------------------------------------ the network and its blob
struct Conv {
    ConvSpec c;
    size_t w, b;      // blob offsets in floats
    int i_w;          // parameter index of the weight; the batch norm behind it is the next four parameters
};
struct Block {
    int cin, cout, s, nconv;
    Conv c[3];
    bool ds;
    Conv d;
};
struct Net {
    int stem, F, A;
    Conv conv1;
    std::vector<Block> blocks;
    size_t fc_w, fc_b;
    int i_fc;
    ParamTable t;     // the caller's parameters in state-dict order (num_batches_tracked left out)
};

bool channels_ok(int c) { return c >= 4 && c % 4 == 0 && c <= kMaxCh; }

// The blob, piece by piece in the order the pieces lie in it, and beside each piece the parameters it is made from.  Convolutions,
// batch norms and fc.weight are P_OWNER: uspace_resnet_pack_weights folds (or transposes) them into the pieces taken here.
bool make_net(const uspace_resnet_config* cfg, Net* out) {
    if (!cfg || !channels_ok(cfg->stem) || (cfg->bottleneck != 0 && cfg->bottleneck != 1)) return false;
    if (cfg->num_outputs < 1 || cfg->num_outputs > 65536) return false;
    const int exp = cfg->bottleneck ? 4 : 1;
    for (int l = 0; l < 4; ++l) {
        if (cfg->blocks[l] < 1 || cfg->blocks[l] > 4096) return false;
        if (!channels_ok(cfg->planes[l]) || cfg->planes[l] > kMaxCh / exp) return false;
    }
    Net n;
    n.stem = cfg->stem;
    n.A = cfg->num_outputs;
    ParamTable& t = n.t;
    auto take = [&](size_t floats) { return t.arena.take(floats * sizeof(float)) / sizeof(float); };
    auto conv = [&](int cin, int cout, int k, int s, int p) {
        Conv v;
        v.c = ConvSpec{cin, cout, k, k, s, p, p};
        v.w = take((size_t)conv_kpad(v.c) * cout);
        v.b = take(cout);
        v.i_w = t.add((long)cout * cin * k * k, P_OWNER);
        for (int j = 0; j < 4; ++j) t.add(cout, P_OWNER);
        return v;
    };
    n.conv1 = conv(3, n.stem, 7, 2, 3);
    int cin = n.stem;
    for (int l = 0; l < 4; ++l)
        for (int j = 0; j < cfg->blocks[l]; ++j) {
            Block b{};
            const int p = cfg->planes[l];
            b.cin = cin;
            b.cout = p * exp;
            b.s = (j == 0 && l > 0) ? 2 : 1;
            if (cfg->bottleneck) {
                b.nconv = 3;
                b.c[0] = conv(cin, p, 1, 1, 0);
                b.c[1] = conv(p, p, 3, b.s, 1);      // the stride on the 3 x 3: "v1.5"
                b.c[2] = conv(p, b.cout, 1, 1, 0);
            } else {
                b.nconv = 2;
                b.c[0] = conv(cin, p, 3, b.s, 1);
                b.c[1] = conv(p, p, 3, 1, 1);
            }
            b.ds = b.s != 1 || b.cin != b.cout;
            if (b.ds) b.d = conv(cin, b.cout, 1, b.s, 0);
            n.blocks.push_back(b);
            cin = b.cout;
        }
    n.F = cin;
    n.fc_w = take((size_t)n.F * n.A);
    n.i_fc = t.add((long)n.A * n.F, P_OWNER);
    n.fc_b = t.at(t.add(n.A, P_F32)) / sizeof(float);
    *out = std::move(n);
    return true;
}

inline int conv_out(int h, const ConvSpec& c) { return (h + 2 * c.ph - c.kh) / c.s + 1; }
inline int pool_out(int h) { return (h + 2 - 3) / 2 + 1; }

// The workspace: the stem's map and a block's first intermediate share `a`, the bottleneck's second intermediate is `b`, the
// downsample's map `sc`, the blocks' outputs alternate between x[0] and x[1]; then the fp64 partial sums and the pooled vectors.
struct Carve {
    size_t off_x[2], off_a, off_b, off_sc, off_part, off_pool, bytes;
    int hf, wf;       // the last map's size
};
bool plan(const Net& n, int B, int H, int W, Carve* c) {
    if (B < 1 || B > 32767 || H < 32 || W < 32 || H > 16384 || W > 16384) return false;
    const size_t lim = (size_t)1 << 31;       // every tensor stays below 2^31 elements: the convolution counts pixels in int
    if ((size_t)B * H * W * 3 >= lim) return false;
    size_t x = 0, a = 0, b = 0, sc = 0;
    int h = conv_out(H, n.conv1.c), w = conv_out(W, n.conv1.c);
    a = (size_t)B * h * w * n.stem;
    h = pool_out(h), w = pool_out(w);
    x = (size_t)B * h * w * n.stem;
    for (const Block& k : n.blocks) {
        const int ho = (h - 1) / k.s + 1, wo = (w - 1) / k.s + 1;      // 3 x 3 pad 1 and 1 x 1 pad 0 alike
        const size_t p = k.c[0].c.cout;
        if (k.nconv == 3) {
            a = std::max(a, (size_t)B * h * w * p);
            b = std::max(b, (size_t)B * ho * wo * p);
        } else {
            a = std::max(a, (size_t)B * ho * wo * p);
        }
        if (k.ds) sc = std::max(sc, (size_t)B * ho * wo * k.cout);
        x = std::max(x, (size_t)B * ho * wo * k.cout);
        h = ho, w = wo;
    }
    if (x >= lim || a >= lim || b >= lim || sc >= lim) return false;
    Arena ar;
    c->off_x[0] = ar.take(x * sizeof(float));
    c->off_x[1] = ar.take(x * sizeof(float));
    c->off_a = ar.take(a * sizeof(float));
    c->off_b = ar.take(b * sizeof(float));
    c->off_sc = ar.take(sc * sizeof(float));
    c->off_part = ar.take((size_t)B * us_cdiv(h * w, kPoolPix) * n.F * sizeof(double));
    c->off_pool = ar.take((size_t)B * n.F * sizeof(float));
    c->bytes = ar.off;
    c->hf = h, c->wf = w;
    return true;
}

// ------------------------------------------------------------------------------------------------ kernels
// fc.weight [A][F] -> [F][A]: the logits kernel's threads read consecutive outputs of one feature
__global__ __launch_bounds__(256) void resnet_pack_fc_kernel(const float* __restrict__ w, float* __restrict__ wout, int F, int A) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)F * A) return;
    const int k = (int)(idx / A), n = (int)(idx - (long)k * A);
    wout[idx] = w[(long)n * F + k];
}

struct Norm3 {
    float mean[3], std[3];
};
// x NCHW [B, 3, H, W] -> out NHWC [B, H, W, 3], (x - mean_c) / std_c; one thread per pixel
__global__ __launch_bounds__(256) void resnet_input_kernel(const float* __restrict__ x, float* __restrict__ out, long B, long HW,
                                                           Norm3 nm) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= B * HW) return;
    const long b = idx / HW, p = idx - b * HW;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[idx * 3 + c] = (x[(b * 3 + c) * HW + p] - nm.mean[c]) / nm.std[c];
}

// part[b, chunk, c] = the fp64 sum of t [B, HW, C] over the chunk's kPoolPix pixels in pixel order; a thread owns channels
__global__ __launch_bounds__(256) void resnet_pool_partial_kernel(const float* __restrict__ t, double* __restrict__ part, int HW, int C,
                                                                  int nchunk) {
    const int b = blockIdx.y, chunk = blockIdx.x;
    const int p0 = chunk * kPoolPix, p1 = min(p0 + kPoolPix, HW);
    const float* tb = t + (size_t)b * HW * C;
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        double s = 0.0;
        for (int p = p0; p < p1; ++p) s += (double)tb[(size_t)p * C + c];
        part[((size_t)b * nchunk + chunk) * C + c] = s;
    }
}

// One wave per sample: pooled[b, c] = (the partials in chunk order) / HW, rounded once
__global__ __launch_bounds__(64) void resnet_pool_finish_kernel(const double* __restrict__ part, float* __restrict__ pooled, int HW,
                                                                int C, int nchunk) {
    const int b = blockIdx.x;
    for (int c = threadIdx.x; c < C; c += 64) {
        double s = 0.0;
        for (int j = 0; j < nchunk; ++j) s += part[((size_t)b * nchunk + j) * C + c];
        pooled[(size_t)b * C + c] = (float)(s / (double)HW);
    }
}

// logits[b, n] = fma(..fma(pooled[b, 0], w[0, n], 0)..) + bias_n: one thread per output, the features in order.  wt [F][A].
__global__ __launch_bounds__(64) void resnet_fc_kernel(const float* __restrict__ pooled, const float* __restrict__ wt,
                                                       const float* __restrict__ bias, float* __restrict__ logits, int F, int A) {
    const int b = blockIdx.y, n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= A) return;
    const float* pb = pooled + (size_t)b * F;
    float s = 0.f;
    for (int k = 0; k < F; ++k) s = fmaf(pb[k], wt[(size_t)k * A + n], s);
    logits[(size_t)b * A + n] = s + bias[n];
}

// The edit-effect columns of one pair per thread, fp64, in attribute order.  d_j = zb_j - za_j, t the pair's target:
// out[b] = { sign d_t,  sign zb_t > 0,  mean_{j != t} |d_j| / sigma_j,  |d_t| / sigma_t over (that + sum_{j != t} |d_j| / sigma_j) };
// the last is 0 where nothing moved; sigma == NULL: all ones.  A target outside 0 .. A - 1 gives four NaNs.
__global__ __launch_bounds__(64) void attr_effect_kernel(const float* __restrict__ za, const float* __restrict__ zb,
                                                         const int* __restrict__ target, const float* __restrict__ sign,
                                                         const float* __restrict__ sigma, int B, int A, double* __restrict__ out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int t = target[b];
    double* o = out + (size_t)b * 4;
    if (t < 0 || t >= A) {
        o[0] = o[1] = o[2] = o[3] = nan("");
        return;
    }
    const float* a = za + (size_t)b * A;
    const float* e = zb + (size_t)b * A;
    const double sg = (double)sign[b];
    double off = 0.0;
    for (int j = 0; j < A; ++j) {
        if (j == t) continue;
        const double d = fabs((double)e[j] - (double)a[j]);
        off += sigma ? d / (double)sigma[j] : d;
    }
    const double dt = (double)e[t] - (double)a[t];
    const double hit = sigma ? fabs(dt) / (double)sigma[t] : fabs(dt);
    o[0] = sg * dt;
    o[1] = sg * (double)e[t] > 0.0 ? 1.0 : 0.0;
    o[2] = A > 1 ? off / (double)(A - 1) : 0.0;
    o[3] = hit + off > 0.0 ? hit / (hit + off) : 0.0;
}

// ------------------------------------------------------------------------------------------------ the forward
struct Bufs {
    float *a, *b, *sc;
};

// One block on x [B, H, W, cin] -> out [B, Ho, Wo, cout]
int run_block(const Block& k, const float* wts, const float* x, int B, int H, int W, const Bufs& bf, float* out, hipStream_t st,
              int* Ho, int* Wo) {
    int h, w, ho, wo;
    const float* res = x;
    int ldr = k.cin;
    if (k.ds) {
        US_TRY(conv_f32_launch<CONV_EPI_BIAS>(k.d.c, x, B, H, W, wts + k.d.w, wts + k.d.b, bf.sc, k.cout, 0, st, &h, &w));
        res = bf.sc;
        ldr = k.cout;
    }
    const Conv& last = k.c[k.nconv - 1];
    US_TRY(conv_f32_launch<CONV_EPI_RELU>(k.c[0].c, x, B, H, W, wts + k.c[0].w, wts + k.c[0].b, bf.a, k.c[0].c.cout, 0, st, &ho, &wo));
    const float* mid = bf.a;
    if (k.nconv == 3) {
        US_TRY(conv_f32_launch<CONV_EPI_RELU>(k.c[1].c, bf.a, B, ho, wo, wts + k.c[1].w, wts + k.c[1].b, bf.b, k.c[1].c.cout, 0, st, &ho,
                                              &wo));
        mid = bf.b;
    }
    if (k.ds && (h != ho || w != wo)) return USPACE_ERR_ARG;
    US_TRY(conv_f32_launch<CONV_EPI_ADD_RELU>(last.c, mid, B, ho, wo, wts + last.w, wts + last.b, out, k.cout, 0, st, &ho, &wo, nullptr,
                                              res, ldr));
    *Ho = ho;
    *Wo = wo;
    return USPACE_OK;
}

// Stages 0 (the stem after the max pool) .. 1 + u (block u) .. 1 + U (the pooled vector).  dump != NULL: stage `last` is copied
// there and nothing later runs; dump == NULL: the whole tower runs (`last` is ignored), logits and, if asked for, pooled are written.
int run(const uspace_resnet_config* cfg, const void* blob, void* ws, size_t ws_bytes, const float* x, int B, int H, int W, int last,
        float* dump, float* pooled, float* logits, hipStream_t st) {
    Net n;
    if (!make_net(cfg, &n) || !blob || !ws || !x) return USPACE_ERR_ARG;
    const int U = (int)n.blocks.size();
    if (!dump) last = U + 1;
    if (last < 0 || last > U + 1) return USPACE_ERR_ARG;
    Carve cv;
    if (!plan(n, B, H, W, &cv)) return USPACE_ERR_ARG;
    if (ws_bytes < cv.bytes) return USPACE_ERR_WORKSPACE;
    char* base = (char*)ws;
    float* xb[2] = {(float*)(base + cv.off_x[0]), (float*)(base + cv.off_x[1])};
    const Bufs bf{(float*)(base + cv.off_a), (float*)(base + cv.off_b), (float*)(base + cv.off_sc)};
    const float* wts = (const float*)blob;
    int h, w, cur = 0, c = n.stem;
    US_TRY(conv_f32_launch<CONV_EPI_RELU>(n.conv1.c, x, B, H, W, wts + n.conv1.w, wts + n.conv1.b, bf.a, n.stem, 0, st, &h, &w));
    US_TRY(pool3_launch(bf.a, B, h, w, n.stem, true, 2, 1, xb[0], n.stem, 0, st, &h, &w));
    for (int u = 0; u < U && u < last; ++u) {
        US_TRY(run_block(n.blocks[u], wts, xb[cur], B, h, w, bf, xb[cur ^ 1], st, &h, &w));
        cur ^= 1;
        c = n.blocks[u].cout;
    }
    if (last <= U) {
        const size_t bytes = (size_t)B * h * w * c * sizeof(float);
        if (hipMemcpyAsync(dump, xb[cur], bytes, hipMemcpyDeviceToDevice, st) != hipSuccess) return USPACE_ERR_LAUNCH;
        return USPACE_OK;
    }
    if (h != cv.hf || w != cv.wf || c != n.F) return USPACE_ERR_ARG;      // the plan sized the partial sums
    const int hw = h * w, nchunk = us_cdiv(hw, kPoolPix);
    double* part = (double*)(base + cv.off_part);
    float* pool = dump ? dump : (pooled ? pooled : (float*)(base + cv.off_pool));
    hipLaunchKernelGGL(resnet_pool_partial_kernel, dim3(nchunk, B), dim3(std::min(n.F, 256)), 0, st, xb[cur], part, hw, n.F, nchunk);
    US_CHECK_LAUNCH();
    hipLaunchKernelGGL(resnet_pool_finish_kernel, dim3(B), dim3(64), 0, st, part, pool, hw, n.F, nchunk);
    US_CHECK_LAUNCH();
    if (dump) return USPACE_OK;
    hipLaunchKernelGGL(resnet_fc_kernel, dim3(us_cdiv(n.A, 64), B), dim3(64), 0, st, pool, wts + n.fc_w, wts + n.fc_b, logits, n.F, n.A);
    US_CHECK_LAUNCH();
    return USPACE_OK;
}

}  // namespace

extern "C" int uspace_resnet_num_params(const uspace_resnet_config* cfg) {
    Net n;
    return make_net(cfg, &n) ? n.t.n_params : USPACE_ERR_ARG;
}

extern "C" long uspace_resnet_param_numel(const uspace_resnet_config* cfg, int index) {
    Net n;
    return make_net(cfg, &n) ? n.t.numel(index) : USPACE_ERR_ARG;
}

extern "C" size_t uspace_resnet_weight_bytes(const uspace_resnet_config* cfg) {
    Net n;
    return make_net(cfg, &n) ? n.t.bytes() : 0;
}

extern "C" size_t uspace_resnet_workspace_bytes(const uspace_resnet_config* cfg, int B, int H, int W) {
    Net n;
    Carve c;
    return make_net(cfg, &n) && plan(n, B, H, W, &c) ? c.bytes : 0;
}

extern "C" int uspace_resnet_pack_weights(const uspace_resnet_config* cfg, const float* const* params, int n_params, void* blob,
                                          size_t blob_bytes, uspace_stream_t stream) {
    Net n;
    if (!make_net(cfg, &n)) return USPACE_ERR_ARG;
    US_TRY(us_pack_table(n.t, params, n_params, blob, blob_bytes, stream));      // the checks; fc.bias
    hipStream_t st = (hipStream_t)stream;
    float* out = (float*)blob;
    // a convolution with the batch norm after it (the four parameters behind its weight) folded in
    auto conv_bn = [&](const Conv& v) {
        return conv_f32_pack(v.c, params[v.i_w], ConvPackSource::batch_norm(params + v.i_w + 1, kBnEps), out + v.w, out + v.b, st);
    };
    US_TRY(conv_bn(n.conv1));
    for (const Block& k : n.blocks) {
        for (int j = 0; j < k.nconv; ++j) US_TRY(conv_bn(k.c[j]));
        if (k.ds) US_TRY(conv_bn(k.d));
    }
    const long cnt = (long)n.F * n.A;
    hipLaunchKernelGGL(resnet_pack_fc_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, params[n.i_fc], out + n.fc_w, n.F, n.A);
    US_CHECK_LAUNCH();
    return USPACE_OK;
}

extern "C" int uspace_resnet_preprocess(const float* x, int B, int H, int W, const float* mean, const float* std, float* out,
                                        uspace_stream_t stream) {
    if (!x || !out || !mean || !std || B < 1 || H < 1 || W < 1 || H > 16384 || W > 16384) return USPACE_ERR_ARG;
    if ((size_t)B * 3 * H * W >= ((size_t)1 << 31)) return USPACE_ERR_ARG;
    Norm3 nm;
    for (int c = 0; c < 3; ++c) {
        if (!(std[c] > 0.f) || !isfinite(std[c]) || !isfinite(mean[c])) return USPACE_ERR_ARG;
        nm.mean[c] = mean[c];
        nm.std[c] = std[c];
    }
    const long cnt = (long)B * H * W;
    hipLaunchKernelGGL(resnet_input_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, out, (long)B,
                       (long)H * W, nm);
    US_CHECK_LAUNCH();
    return USPACE_OK;
}

extern "C" int uspace_resnet_forward(const uspace_resnet_config* cfg, const void* blob, void* workspace, size_t workspace_bytes,
                                     const float* x_nhwc, int B, int H, int W, float* pooled, float* logits, uspace_stream_t stream) {
    if (!logits) return USPACE_ERR_ARG;
    return run(cfg, blob, workspace, workspace_bytes, x_nhwc, B, H, W, 0, nullptr, pooled, logits, (hipStream_t)stream);
}

extern "C" int uspace_resnet_tap(const uspace_resnet_config* cfg, const void* blob, void* workspace, size_t workspace_bytes,
                                 const float* x_nhwc, int B, int H, int W, int stage, float* dump, uspace_stream_t stream) {
    if (!dump) return USPACE_ERR_ARG;
    return run(cfg, blob, workspace, workspace_bytes, x_nhwc, B, H, W, stage, dump, nullptr, nullptr, (hipStream_t)stream);
}

extern "C" int uspace_attr_effect_f64(const float* za, const float* zb, const int* target, const float* sign, const float* sigma, int B,
                                      int A, double* out, uspace_stream_t stream) {
    if (!za || !zb || !target || !sign || !out || B < 1 || A < 1 || (long)B * A >= (1L << 31)) return USPACE_ERR_ARG;
    hipLaunchKernelGGL(attr_effect_kernel, dim3(us_cdiv(B, 64)), dim3(64), 0, (hipStream_t)stream, za, zb, target, sign, sigma, B, A,
                       out);
    US_CHECK_LAUNCH();
    return USPACE_OK;
}
