// SD KL-VAE decoder on gfx950: latents [B,4,h,w] -> images [B,3,R,R]
// (reference: libs/autoencoder.py:303-409 Decoder.forward, :446-450 FrozenAutoencoderKL.decode).
//
// Layout: every feature map is "zero-bordered NHWC": rows = pixels of [B, H+2, W+2], C channels per
// row, with (W+3) guard rows before and after, so a 3x3 convolution is the sum of 9 row-shifted GEMMs
// on the bf16 MFMA kernel (uspace_gemm_slabs_bf16) and the zero border IS the conv padding.  fp32 maps
// carry the residual stream; GroupNorm(+SiLU) turns them into the bf16 operand maps (border re-zeroed).
// Nearest-2x upsampling writes the next resolution's bf16 operand directly.  The single-head mid-block
// attention (1024 tokens x 512 channels) runs as two GEMMs per image around a row softmax.
//
// The encoder (images [B,3,R,R] -> moments [B,8,h,w], libs/autoencoder.py:215-300,428-431) runs on the same helpers
// (VaeRun); its stride-2 downsample convolves four bf16 phase maps of the input with the same slab GEMM.
#include <algorithm>
#include <vector>

#include "blob.h"

namespace {

// ------------------------------------------------------------------------------------------ kernels
// z/scale -> post_quant_conv (1x1) -> conv_in (3x3, pad 1): one block per latent pixel.
__global__ __launch_bounds__(128) void vae_conv_in_kernel(const float* __restrict__ z, float inv_scale,
                                                          const float* __restrict__ wq, const float* __restrict__ bq,
                                                          const float* __restrict__ w, const float* __restrict__ bias,
                                                          float* __restrict__ out, int h, int wd, int C0) {
    __shared__ float nb[36];   // post-quant values of the 3x3 neighbourhood, (c, dy, dx) order; 0 outside the image
    const int pix = blockIdx.x;
    const int b = pix / (h * wd), yx = pix % (h * wd), y = yx / wd, x = yx % wd;
    if (threadIdx.x < 36) {
        const int c = threadIdx.x / 9, t = threadIdx.x % 9, dy = t / 3 - 1, dx = t % 3 - 1;
        const int yy = y + dy, xx = x + dx;
        float v = 0.f;
        if (yy >= 0 && yy < h && xx >= 0 && xx < wd) {
            v = bq[c];
            for (int ci = 0; ci < 4; ++ci) v += wq[c * 4 + ci] * (z[((size_t)(b * 4 + ci) * h + yy) * wd + xx] * inv_scale);
        }
        nb[threadIdx.x] = v;
    }
    __syncthreads();
    float* o = out + ((size_t)(b * (h + 2) + y + 1) * (wd + 2) + x + 1) * C0;
    for (int d = threadIdx.x; d < C0; d += blockDim.x) {
        const float* wr = w + (size_t)d * 36;
        float s = bias[d];
#pragma unroll
        for (int e = 0; e < 36; ++e) s += wr[e] * nb[e];
        o[d] = s;
    }
}

// GroupNorm statistics over the interior pixels.  Block = (image, pixel chunk); a thread owns one 4-channel
// vector (16 B loads, a pixel row of C floats is read by C/4 adjacent lanes) and strides over the chunk's
// pixels.  Per-thread half-vector sums go through LDS and 32 threads add the 16 contributions of their group
// in a fixed order; gn_finish_kernel adds the chunks, again in a fixed order, so repeated decodes are
// bit-identical (no atomics).  The sums are of x - K, K = the group's first channel at the first interior pixel
// (one value per (image, group), read by every chunk): var = E[(x-K)^2] - E[x-K]^2 then does not cancel when
// the group's mean is large against its spread (on raw values it lost all digits at mean/std ~ 3e3 at 256^2).
__device__ __forceinline__ float gn_pilot(const float* __restrict__ x, int b, int H, int W, int C, int g) {
    return x[((size_t)b * (H + 2) + 1) * (W + 2) * C + (size_t)C + g * (C >> 5)];
}
__global__ __launch_bounds__(256) void gn_stats_kernel(const float* __restrict__ x, float* __restrict__ partial,
                                                       int H, int W, int C, int c4_log2, int chunks) {
    __shared__ float red[256 * 4];
    const int b = blockIdx.x / chunks, ck = blockIdx.x % chunks;
    const int tid = threadIdx.x;
    const int C4 = 1 << c4_log2;
    const int q = tid & (C4 - 1), ps = tid >> c4_log2, PS = 256 >> c4_log2;
    const int npix = H * W;
    const int per = (npix + chunks - 1) / chunks;
    const int p0 = ck * per, p1 = min(npix, p0 + per);
    float s0 = 0.f, q0 = 0.f, s1 = 0.f, q1 = 0.f;
    const float* xb = x + (size_t)b * (H + 2) * (W + 2) * C + 4 * q;
    const int cg = C >> 5;                        // channels per group: a half-vector never straddles two groups
    const float k0 = gn_pilot(x, b, H, W, C, (4 * q) / cg), k1 = gn_pilot(x, b, H, W, C, (4 * q + 2) / cg);
#pragma unroll 4
    for (int p = p0 + ps; p < p1; p += PS) {
        const int y = p / W, xx = p - y * W;
        const f32x4 v = *(const f32x4*)(xb + (size_t)((y + 1) * (W + 2) + xx + 1) * C);
        const float d0 = v[0] - k0, d1 = v[1] - k0, d2 = v[2] - k1, d3 = v[3] - k1;
        s0 += d0 + d1;
        q0 += d0 * d0 + d1 * d1;
        s1 += d2 + d3;
        q1 += d2 * d2 + d3 * d3;
    }
    red[tid * 4 + 0] = s0;
    red[tid * 4 + 1] = q0;
    red[tid * 4 + 2] = s1;
    red[tid * 4 + 3] = q1;
    __syncthreads();
    if (tid < 32) {
        const int hpg = C >> 6;                   // half-vectors (2 channels) per group: 1..8
        float s = 0.f, ss = 0.f;
        for (int r = 0; r < PS; ++r)
            for (int j = 0; j < hpg; ++j) {
                const int hq = tid * hpg + j;     // half-vector index inside the pixel row
                const float* e = red + ((r << c4_log2) + (hq >> 1)) * 4 + (hq & 1) * 2;
                s += e[0];
                ss += e[1];
            }
        float* o = partial + (((size_t)b * chunks + ck) * 32 + tid) * 2;
        o[0] = s;
        o[1] = ss;
    }
}

// (sum, sumsq) partials of x - K -> (mean, rstd) per (image, group): one wave per pair, butterfly reduction
__global__ __launch_bounds__(64) void gn_finish_kernel(const float* __restrict__ partial, float* __restrict__ stats,
                                                       int chunks, float inv_n, float eps, const float* __restrict__ x,
                                                       int H, int W, int C) {
    const int i = blockIdx.x;
    const int b = i >> 5, g = i & 31;
    float s = 0.f, ss = 0.f;
    for (int ck = threadIdx.x; ck < chunks; ck += 64) {
        const float* p = partial + (((size_t)b * chunks + ck) * 32 + g) * 2;
        s += p[0];
        ss += p[1];
    }
    s = wave_sum(s);
    ss = wave_sum(ss);
    if (threadIdx.x == 0) {
        const float dm = s * inv_n;
        const float var = fmaxf(ss * inv_n - dm * dm, 0.f);
        stats[2 * i] = gn_pilot(x, b, H, W, C, g) + dm;
        stats[2 * i + 1] = rsqrtf(var + eps);
    }
}

// y = (x - mean) * rstd * gamma + beta (+ SiLU) -> bf16 operand map with the border rows zeroed.
// Block = 256 threads = 256/C4 padded-map rows per step; 32-bit index arithmetic only.
__global__ __launch_bounds__(256) void gn_apply_kernel(const float* __restrict__ x, const float* __restrict__ stats,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       bf16_t* __restrict__ y, int B, int H, int W, int C, int c4_log2,
                                                       int silu) {
    const int tid = threadIdx.x;
    const int C4 = 1 << c4_log2;
    const int c = (tid & (C4 - 1)) * 4, rsub = tid >> c4_log2, RS = 256 >> c4_log2;
    const unsigned rows_img = (unsigned)(H + 2) * (unsigned)(W + 2);
    const unsigned rows = (unsigned)B * rows_img;
    const int cg = C >> 5;                       // 2 at C=64: a 4-channel vector then spans two groups
    const f32x4 gm = *(const f32x4*)(gamma + c);
    const f32x4 bt = *(const f32x4*)(beta + c);
    const int g0 = c / cg, g1 = (c + 2) / cg;
    for (unsigned row = blockIdx.x * RS + rsub; row < rows; row += gridDim.x * RS) {
        const unsigned b = row / rows_img, rr = row - b * rows_img;
        const unsigned yy = rr / (unsigned)(W + 2), xx = rr - yy * (unsigned)(W + 2);
        uint2 o = make_uint2(0u, 0u);
        if (xx >= 1 && xx <= (unsigned)W && yy >= 1 && yy <= (unsigned)H) {
            const f32x4 v = *(const f32x4*)(x + (size_t)row * C + c);
            const float m0 = stats[(b * 32 + g0) * 2], r0 = stats[(b * 32 + g0) * 2 + 1];
            const float m1 = stats[(b * 32 + g1) * 2], r1 = stats[(b * 32 + g1) * 2 + 1];
            f32x4 r;
            r[0] = (v[0] - m0) * r0 * gm[0] + bt[0];
            r[1] = (v[1] - m0) * r0 * gm[1] + bt[1];
            r[2] = (v[2] - m1) * r1 * gm[2] + bt[2];
            r[3] = (v[3] - m1) * r1 * gm[3] + bt[3];
            if (silu) {
#pragma unroll
                for (int e = 0; e < 4; ++e) r[e] = r[e] / (1.0f + __expf(-r[e]));
            }
            o.x = pack_bf2(r[0], r[1]);
            o.y = pack_bf2(r[2], r[3]);
        }
        *(uint2*)(y + (size_t)row * C + c) = o;
    }
}

// nearest 2x: fp32 map [B,H+2,W+2,C] interior -> bf16 operand map [B,2H+2,2W+2,C] (border zero)
__global__ __launch_bounds__(256) void upsample_kernel(const float* __restrict__ x, bf16_t* __restrict__ y,
                                                       int B, int H, int W, int C) {
    const int C4 = C >> 2, H2 = 2 * H, W2 = 2 * W;
    const long total = (long)B * (H2 + 2) * (W2 + 2) * C4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long row = i / C4;
        const int c = (int)(i % C4) * 4;
        const int xx = row % (W2 + 2), yy = (row / (W2 + 2)) % (H2 + 2), b = (int)(row / ((long)(W2 + 2) * (H2 + 2)));
        uint2 o = make_uint2(0u, 0u);
        if (xx >= 1 && xx <= W2 && yy >= 1 && yy <= H2) {
            const int sy = (yy - 1) / 2 + 1, sx = (xx - 1) / 2 + 1;
            const f32x4 v = *(const f32x4*)(x + ((size_t)(b * (H + 2) + sy) * (W + 2) + sx) * C + c);
            o.x = pack_bf2(v[0], v[1]);
            o.y = pack_bf2(v[2], v[3]);
        }
        *(uint2*)(y + row * C + c) = o;
    }
}

// bf16 operand map interior -> compact token rows [B*H*W, C]
__global__ __launch_bounds__(256) void gather_interior_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ y,
                                                              int B, int H, int W, int C) {
    const int C8 = C >> 3;
    const long total = (long)B * H * W * C8;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long tokn = i / C8;
        const int c = (int)(i % C8) * 8;
        const int xx = tokn % W, yy = (tokn / W) % H, b = (int)(tokn / ((long)W * H));
        *(uint4*)(y + tokn * C + c) = *(const uint4*)(x + ((size_t)(b * (H + 2) + yy + 1) * (W + 2) + xx + 1) * C + c);
    }
}

// fp32 map interior += compact rows
__global__ __launch_bounds__(256) void scatter_add_kernel(float* __restrict__ x, const float* __restrict__ t,
                                                          int B, int H, int W, int C) {
    const int C4 = C >> 2;
    const long total = (long)B * H * W * C4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long tokn = i / C4;
        const int c = (int)(i % C4) * 4;
        const int xx = tokn % W, yy = (tokn / W) % H, b = (int)(tokn / ((long)W * H));
        f32x4* d = (f32x4*)(x + ((size_t)(b * (H + 2) + yy + 1) * (W + 2) + xx + 1) * C + c);
        *d += *(const f32x4*)(t + tokn * C + c);
    }
}

// row softmax of S * scale (fp32 [R, N]) -> bf16 P; one wave per row
__global__ __launch_bounds__(256) void softmax_rows_kernel(const float* __restrict__ s, bf16_t* __restrict__ p,
                                                           long R, int N, float scale) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= R) return;
    const float* sr = s + row * N;
    float mx = -INFINITY;
    for (int j = lane; j < N; j += 64) mx = fmaxf(mx, sr[j]);
    mx = wave_max(mx);
    float sum = 0.f;
    for (int j = lane; j < N; j += 64) sum += __expf((sr[j] - mx) * scale);
    sum = wave_sum(sum);
    const float inv = 1.0f / sum;
    for (int j = lane; j < N; j += 64) p[row * N + j] = f2bf(__expf((sr[j] - mx) * scale) * inv);
}

// [nb][R][C] bf16 -> [nb][C][R]
__global__ __launch_bounds__(256) void transpose_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ y, int R, int C) {
    __shared__ bf16_t tile[32][33];
    const int bz = blockIdx.z;
    const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
    const bf16_t* xs = x + (size_t)bz * R * C;
    bf16_t* ys = y + (size_t)bz * R * C;
    for (int j = ty; j < 32; j += 8)
        if (r0 + j < R && c0 + tx < C) tile[j][tx] = xs[(size_t)(r0 + j) * C + c0 + tx];
    __syncthreads();
    for (int j = ty; j < 32; j += 8)
        if (c0 + j < C && r0 + tx < R) ys[(size_t)(c0 + j) * R + r0 + tx] = tile[tx][j];
}

// conv_out (C -> 3, libs/autoencoder.py:379,407): too narrow for an MFMA tile.  LPP = C/8 adjacent lanes share a
// pixel, each holding its 8 channels' 3x9x8 weights in registers for the whole launch; a tap is one coalesced
// 16 B load per lane (C*2 contiguous bytes per pixel), the three sums are reduced across the LPP lanes.
// x: bf16 zero-bordered map; w: fp32 [3][9][C]; out: NCHW fp32.
template <int LPP>
__global__ __launch_bounds__(256) void vae_conv_out_kernel(const bf16_t* __restrict__ x, const float* __restrict__ w,
                                                           const float* __restrict__ bias, float* __restrict__ out,
                                                           int B, int H, int W) {
    constexpr int C = LPP * 8;
    const int l = threadIdx.x % LPP;
    const unsigned slot = (blockIdx.x * 256u + threadIdx.x) / LPP, slots = gridDim.x * 256u / LPP;
    float wr[3][9][8];
#pragma unroll
    for (int o = 0; o < 3; ++o)
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int e = 0; e < 8; ++e) wr[o][t][e] = w[(o * 9 + t) * C + l * 8 + e];
    const float b0 = bias[0], b1 = bias[1], b2 = bias[2];
    const unsigned plane = (unsigned)H * (unsigned)W, npix = (unsigned)B * plane;
    for (unsigned pix = slot; pix < npix; pix += slots) {
        const unsigned b = pix / plane, rr = pix - b * plane;
        const unsigned yy = rr / (unsigned)W, xx = rr - yy * (unsigned)W;
        const bf16_t* xc = x + ((size_t)(b * (H + 2) + yy + 1) * (W + 2) + xx + 1) * C + l * 8;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int dy = t / 3 - 1, dx = t % 3 - 1;
            const uint4 q = *(const uint4*)(xc + (dy * (W + 2) + dx) * C);
            const uint32_t u[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float lo = __uint_as_float(u[e] << 16), hi = __uint_as_float(u[e] & 0xffff0000u);
                a0 += lo * wr[0][t][2 * e] + hi * wr[0][t][2 * e + 1];
                a1 += lo * wr[1][t][2 * e] + hi * wr[1][t][2 * e + 1];
                a2 += lo * wr[2][t][2 * e] + hi * wr[2][t][2 * e + 1];
            }
        }
#pragma unroll
        for (int o = LPP / 2; o > 0; o >>= 1) {
            a0 += __shfl_xor(a0, o, 64);
            a1 += __shfl_xor(a1, o, 64);
            a2 += __shfl_xor(a2, o, 64);
        }
        if (l == 0) {
            float* op = out + (size_t)b * 3 * plane + rr;
            op[0] = a0 + b0;
            op[plane] = a1 + b1;
            op[2 * plane] = a2 + b2;
        }
    }
}

// ------------------------------------------------------------------------------------------ encoder kernels
// Encoder conv_in (3 -> C0, 3x3, pad 1, libs/autoencoder.py:224-228) on NCHW fp32 images -> fp32 zero-bordered NHWC
// map (interior only).  K = 27 is too narrow for an MFMA tile and the kernel is store-bound (R^2 * C0 * 4 bytes per
// image): C0/4 adjacent lanes share a pixel, each holding its 4 channels' 27 weights in registers for the whole launch
// and writing one 16 B vector.  w: fp32 checkpoint layout [C0][3][3][3].  64-bit pixel offsets.
__global__ __launch_bounds__(256) void vae_enc_conv_in_kernel(const float* __restrict__ img, const float* __restrict__ w,
                                                              const float* __restrict__ bias, float* __restrict__ out,
                                                              int B, int R, int C0) {
    const int C4 = C0 >> 2;
    const int q = threadIdx.x % C4;
    const long slot = ((long)blockIdx.x * 256 + threadIdx.x) / C4, slots = (long)gridDim.x * 256 / C4;
    float wr[4][27];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 27; ++e) wr[j][e] = w[(4 * q + j) * 27 + e];
    const f32x4 bs = *(const f32x4*)(bias + 4 * q);
    const long plane = (long)R * R, npix = (long)B * plane;
    for (long pix = slot; pix < npix; pix += slots) {
        const long b = pix / plane;
        const int rr = (int)(pix - b * plane), y = rr / R, x = rr - (rr / R) * R;
        float nb[27];   // (c, dy, dx) order, 0 outside the image
#pragma unroll
        for (int e = 0; e < 27; ++e) {
            const int c = e / 9, dy = (e % 9) / 3 - 1, dx = e % 3 - 1;
            const int yy = y + dy, xx = x + dx;
            nb[e] = (yy >= 0 && yy < R && xx >= 0 && xx < R) ? img[((b * 3 + c) * R + yy) * R + xx] : 0.f;
        }
        f32x4 s = bs;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int e = 0; e < 27; ++e) s[j] += wr[j][e] * nb[e];
        *(f32x4*)(out + ((b * (R + 2) + y + 1) * (R + 2) + x + 1) * C0 + 4 * q) = s;
    }
}

// Downsample operand (libs/autoencoder.py:53-70: pad (0,1,0,1), 3x3 stride 2): fp32 map [B,H+2,H+2,C] interior -> four
// bf16 phase maps E[py,px][a,b] = x[2a+py, 2b+px] in the zero-bordered layout of the output resolution Ho = H/2,
// phase p = 2*py+px at rows p*prow.  The conv's bottom / right pad x[H] = 0 is the phase maps' border row / column Ho+1,
// written as zero from the index here (never read from the fp32 map, whose border holds conv garbage).
__global__ __launch_bounds__(256) void downsample_phases_kernel(const float* __restrict__ x, bf16_t* __restrict__ y,
                                                                int B, int H, int C, long prow) {
    const int C4 = C >> 2, Ho = H >> 1, P = Ho + 2;
    const long rows = (long)B * P * P;
    const long total = 4 * rows * C4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long ra = i / C4;
        const int c = (int)(i % C4) * 4;
        const int ph = (int)(ra / rows);
        const long row = ra - ph * rows;
        const int xx = (int)(row % P), yy = (int)((row / P) % P);
        const long b = row / ((long)P * P);
        uint2 o = make_uint2(0u, 0u);
        if (xx >= 1 && xx <= Ho && yy >= 1 && yy <= Ho) {
            const int sy = 2 * (yy - 1) + (ph >> 1), sx = 2 * (xx - 1) + (ph & 1);
            const f32x4 v = *(const f32x4*)(x + ((b * (H + 2) + sy + 1) * (H + 2) + sx + 1) * C + c);
            o.x = pack_bf2(v[0], v[1]);
            o.y = pack_bf2(v[2], v[3]);
        }
        *(uint2*)(y + (ph * prow + row) * C + c) = o;
    }
}

// Encoder conv_out (C -> 8, 3x3, libs/autoencoder.py:269-273) fused with quant_conv (8 -> 8, 1x1, :419,430) -> NCHW fp32
// moments.  LPP = C/8 adjacent lanes share a group of 4 consecutive pixels of one row, each lane owning 8 channels; eight
// outputs of 9x8 weights each do not fit in registers, so a lane streams its weights (fp32 [8][9][C], L1 / L2 resident)
// once per tap and output and uses them for the 4 pixels.  The 32 sums are reduced across the LPP lanes, and lane 0 adds
// the bias and applies quant_conv.  x: bf16 zero-bordered map; wq: fp32 [8][8]; out [B,8,H,W].
__global__ __launch_bounds__(256) void vae_enc_conv_out_kernel(const bf16_t* __restrict__ x, const float* __restrict__ w,
                                                               const float* __restrict__ bias, const float* __restrict__ wq,
                                                               const float* __restrict__ bq, float* __restrict__ out,
                                                               int B, int H, int W, int C) {
    const int LPP = C >> 3;
    const int l = threadIdx.x % LPP;
    const int WG = (W + 3) >> 2;   // pixel groups per row
    const long slot = ((long)blockIdx.x * 256 + threadIdx.x) / LPP, slots = (long)gridDim.x * 256 / LPP;
    const long ngroups = (long)B * H * WG;
    for (long gi = slot; gi < ngroups; gi += slots) {
        const int xg = (int)(gi % WG), yy = (int)((gi / WG) % H);
        const long b = gi / ((long)WG * H);
        const int x0 = xg * 4;
        const bf16_t* xc = x + ((b * (H + 2) + yy + 1) * (W + 2) + x0 + 1) * C + l * 8;
        float acc[4][8];
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int o = 0; o < 8; ++o) acc[p][o] = 0.f;
#pragma unroll 1
        for (int t = 0; t < 9; ++t) {
            const int dy = t / 3 - 1, dx = t % 3 - 1;
            float a[4][8];
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                uint4 q = make_uint4(0u, 0u, 0u, 0u);
                if (x0 + p < W) q = *(const uint4*)(xc + ((long)dy * (W + 2) + dx + p) * C);
                const uint32_t u[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    a[p][2 * e] = __uint_as_float(u[e] << 16);
                    a[p][2 * e + 1] = __uint_as_float(u[e] & 0xffff0000u);
                }
            }
#pragma unroll
            for (int o = 0; o < 8; ++o) {
                const float* wr = w + (size_t)(o * 9 + t) * C + l * 8;
                const f32x4 w0 = *(const f32x4*)wr, w1 = *(const f32x4*)(wr + 4);
#pragma unroll
                for (int p = 0; p < 4; ++p)
                    acc[p][o] += a[p][0] * w0[0] + a[p][1] * w0[1] + a[p][2] * w0[2] + a[p][3] * w0[3] +
                                 a[p][4] * w1[0] + a[p][5] * w1[1] + a[p][6] * w1[2] + a[p][7] * w1[3];
            }
        }
        for (int off = LPP >> 1; off > 0; off >>= 1)
#pragma unroll
            for (int p = 0; p < 4; ++p)
#pragma unroll
                for (int o = 0; o < 8; ++o) acc[p][o] += __shfl_xor(acc[p][o], off, 64);
        if (l == 0) {
            const long plane = (long)H * W;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                if (x0 + p >= W) continue;
                float h[8];
#pragma unroll
                for (int o = 0; o < 8; ++o) h[o] = acc[p][o] + bias[o];
                float* op = out + b * 8 * plane + (long)yy * W + x0 + p;
#pragma unroll
                for (int o2 = 0; o2 < 8; ++o2) {
                    float m = bq[o2];
#pragma unroll
                    for (int o = 0; o < 8; ++o) m += wq[o2 * 8 + o] * h[o];
                    op[o2 * plane] = m;
                }
            }
        }
    }
}

// FrozenAutoencoderKL.sample (libs/autoencoder.py:433-439): z = scale * (mean + exp(0.5 * clamp(logvar, -30, 20)) * eps),
// moments [B,8,h,w] = (mean, logvar) along channels, eps / z [B,4,h,w].  Rounded step by step as the reference's
// elementwise ops are (no contraction into FMAs).
__global__ __launch_bounds__(256) void vae_sample_kernel(const float* __restrict__ m, const float* __restrict__ eps,
                                                         float scale, float* __restrict__ z, int B, int hw) {
    const long half = 4L * hw, total = (long)B * half;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long b = i / half, r = i - b * half;
        const float mean = m[b * 2 * half + r];
        const float lv = fminf(fmaxf(m[b * 2 * half + half + r], -30.0f), 20.0f);
        const float sd = expf(__fmul_rn(0.5f, lv));
        z[i] = __fmul_rn(scale, __fadd_rn(mean, __fmul_rn(sd, eps[i])));
    }
}

// weight repacks (fp32 checkpoint layout -> kernel layout)
__global__ void repack_conv3_bf16_kernel(const float* __restrict__ src, bf16_t* __restrict__ dst, int Co, int Ci) {
    const long n = (long)Co * Ci * 9;   // src [Co][Ci][3][3] -> dst [Co][9][Ci]
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int ci = i % Ci, t = (i / Ci) % 9;
        const long co = i / ((long)Ci * 9);
        dst[i] = f2bf(src[(co * Ci + ci) * 9 + t]);
    }
}
__global__ void repack_conv3_f32_kernel(const float* __restrict__ src, float* __restrict__ dst, int Co, int Ci) {
    const long n = (long)Co * Ci * 9;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int ci = i % Ci, t = (i / Ci) % 9;
        const long co = i / ((long)Ci * 9);
        dst[i] = src[(co * Ci + ci) * 9 + t];
    }
}

constexpr int USPACE_GN_MAX_CHUNKS = 256;

inline int grid_for(long items, int cap = 4096) {
    long g = (items + 255) / 256;
    return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

// ------------------------------------------------------------------------------------------ model description
struct ResIdx {
    int n1w, n1b, c1w, c1b, n2w, n2b, c2w, c2b, sw = -1, sb = -1;
    int cin, cout;
};

struct AttnIdx {   // single-head AttnBlock (libs/autoencoder.py:139-195): norm, q, k, v, proj_out
    int nw, nb, q_w, q_b, k_w, k_b, v_w, v_b, po_w, po_b;
};

// parameter list of one packed blob, in the reference's state_dict order
struct VaeTable : ParamTable {
    ResIdx add_res(int cin, int cout) {
        ResIdx r;
        r.cin = cin; r.cout = cout;
        r.n1w = add(cin, P_F32); r.n1b = add(cin, P_F32);
        r.c1w = add((long)cout * cin * 9, P_CONV3_BF16, cout, cin); r.c1b = add(cout, P_F32);
        r.n2w = add(cout, P_F32); r.n2b = add(cout, P_F32);
        r.c2w = add((long)cout * cout * 9, P_CONV3_BF16, cout, cout); r.c2b = add(cout, P_F32);
        if (cin != cout) { r.sw = add((long)cout * cin, P_BF16, cout, cin); r.sb = add(cout, P_F32); }
        return r;
    }
    AttnIdx add_attn(int c) {
        AttnIdx a;
        a.nw = add(c, P_F32); a.nb = add(c, P_F32);
        a.q_w = add((long)c * c, P_BF16, c, c); a.q_b = add(c, P_F32);
        a.k_w = add((long)c * c, P_BF16, c, c); a.k_b = add(c, P_F32);
        a.v_w = add((long)c * c, P_BF16, c, c); a.v_b = add(c, P_F32);
        a.po_w = add((long)c * c, P_BF16, c, c); a.po_b = add(c, P_F32);
        return a;
    }
};

struct VaeModel : VaeTable {
    int conv_in_w, conv_in_b;
    ResIdx mid1, mid2;
    AttnIdx attn;
    std::vector<std::vector<ResIdx>> up;   // [level][block]
    std::vector<int> us_w, us_b;           // upsample conv per level (-1 at level 0)
    int no_w, no_b, co_w, co_b, pq_w, pq_b;
    int n_levels, c_top, z_res, res;
};

bool valid_vae(const uspace_vae_config* c) {
    if (!c || c->ch <= 0 || c->ch % 64 || c->n_levels < 1 || c->n_levels > 4 || c->num_res_blocks < 0) return false;
    if (c->resolution <= 0 || c->resolution % (1 << (c->n_levels - 1))) return false;
    for (int i = 0; i < c->n_levels; ++i) {
        const int ch = c->ch * c->ch_mult[i];
        if (c->ch_mult[i] <= 0 || (ch & (ch - 1)) || ch > 512) return false;   // power-of-two channel counts <= 512
    }
    return true;
}

// parameter order = the reference's state_dict order (decoder.*, then post_quant_conv.*)
VaeModel build_vae(const uspace_vae_config& c) {
    VaeModel m;
    m.n_levels = c.n_levels;
    m.res = c.resolution;
    m.z_res = c.resolution >> (c.n_levels - 1);
    int block_in = c.ch * c.ch_mult[c.n_levels - 1];
    m.c_top = block_in;
    m.conv_in_w = m.add((long)block_in * 4 * 9, P_F32); m.conv_in_b = m.add(block_in, P_F32);
    m.mid1 = m.add_res(block_in, block_in);
    m.attn = m.add_attn(block_in);
    m.mid2 = m.add_res(block_in, block_in);
    // channel flow follows construction order (levels reversed); state_dict lists up.0 .. up.{n-1}
    std::vector<int> in_at(c.n_levels);
    {
        int bi = block_in;
        for (int lvl = c.n_levels - 1; lvl >= 0; --lvl) { in_at[lvl] = bi; bi = c.ch * c.ch_mult[lvl]; }
    }
    m.up.resize(c.n_levels);
    m.us_w.assign(c.n_levels, -1);
    m.us_b.assign(c.n_levels, -1);
    for (int lvl = 0; lvl < c.n_levels; ++lvl) {
        int bi = in_at[lvl];
        const int bo = c.ch * c.ch_mult[lvl];
        for (int j = 0; j < c.num_res_blocks + 1; ++j) { m.up[lvl].push_back(m.add_res(bi, bo)); bi = bo; }
        if (lvl != 0) { m.us_w[lvl] = m.add((long)bo * bo * 9, P_CONV3_BF16, bo, bo); m.us_b[lvl] = m.add(bo, P_F32); }
    }
    const int c_last = c.ch * c.ch_mult[0];
    m.no_w = m.add(c_last, P_F32); m.no_b = m.add(c_last, P_F32);
    m.co_w = m.add((long)3 * c_last * 9, P_CONV3_F32T, 3, c_last); m.co_b = m.add(3, P_F32);
    m.pq_w = m.add(16, P_F32); m.pq_b = m.add(4, P_F32);
    return m;
}

// Encoder (libs/autoencoder.py:215-300) with double_z, 3 input channels and no attention in the down path, then quant_conv
struct EncModel : VaeTable {
    int conv_in_w, conv_in_b;
    std::vector<std::vector<ResIdx>> down;   // [level][block]
    std::vector<int> ds_w, ds_b;             // downsample conv per level (-1 at the last level)
    ResIdx mid1, mid2;
    AttnIdx attn;
    int no_w, no_b, co_w, co_b, qc_w, qc_b;
    int n_levels, c_top, z_res, res;
};

bool valid_enc(const uspace_vae_config* c) {
    return valid_vae(c) && c->ch <= 512 && (c->ch & (c->ch - 1)) == 0;   // conv_in's C0 = ch feeds a GroupNorm
}

// parameter order = the reference's state_dict order (encoder.*, then quant_conv.*)
EncModel build_enc(const uspace_vae_config& c) {
    EncModel m;
    m.n_levels = c.n_levels;
    m.res = c.resolution;
    m.z_res = c.resolution >> (c.n_levels - 1);
    m.conv_in_w = m.add((long)c.ch * 3 * 9, P_F32); m.conv_in_b = m.add(c.ch, P_F32);
    m.down.resize(c.n_levels);
    m.ds_w.assign(c.n_levels, -1);
    m.ds_b.assign(c.n_levels, -1);
    int bi = c.ch;
    for (int lvl = 0; lvl < c.n_levels; ++lvl) {
        const int bo = c.ch * c.ch_mult[lvl];
        for (int j = 0; j < c.num_res_blocks; ++j) { m.down[lvl].push_back(m.add_res(bi, bo)); bi = bo; }
        if (lvl != c.n_levels - 1) { m.ds_w[lvl] = m.add((long)bi * bi * 9, P_CONV3_BF16, bi, bi); m.ds_b[lvl] = m.add(bi, P_F32); }
    }
    m.c_top = bi;
    m.mid1 = m.add_res(bi, bi);
    m.attn = m.add_attn(bi);
    m.mid2 = m.add_res(bi, bi);
    m.no_w = m.add(bi, P_F32); m.no_b = m.add(bi, P_F32);
    m.co_w = m.add((long)8 * bi * 9, P_CONV3_F32T, 8, bi); m.co_b = m.add(8, P_F32);
    m.qc_w = m.add(64, P_F32); m.qc_b = m.add(8, P_F32);
    return m;
}

struct VaeWs {
    size_t fa, fb, hb, xb, stats, tok, q, k, v, vt, s, pr, o, po, total;
    long guard_rows;
};

inline size_t map_rows(int B, int res) { return (size_t)B * (res + 2) * (res + 2) + 2 * (size_t)(res + 3); }

// one downsample phase map (guard rows included): the phase stride of the stride-2 convolution, in rows
inline long phase_rows(int B, int Ho) { return (long)map_rows(B, Ho); }

// A map the walk holds: `chan` channels at resolution `res`, as one fp32 map and `phases` bf16 operand maps (4: the phase maps
// of a downsample, one otherwise).
struct MapStep { int res, chan, phases; };

// decode: at each level the widest res block, then the upsample conv keeps that level's channels at twice the resolution
std::vector<MapStep> dec_steps(const uspace_vae_config& c, const VaeModel& m) {
    std::vector<MapStep> st;
    int res = m.z_res, chan = m.c_top;
    for (int lvl = c.n_levels - 1; lvl >= 0; --lvl) {
        st.push_back({res, std::max(chan, c.ch * c.ch_mult[lvl]), 1});
        chan = c.ch * c.ch_mult[lvl];
        if (lvl != 0) {
            res *= 2;
            st.push_back({res, chan, 1});
        }
    }
    return st;
}

// encode: at each level the widest res block, then the four phase maps of the downsample at half the resolution
std::vector<MapStep> enc_steps(const uspace_vae_config& c) {
    std::vector<MapStep> st;
    int res = c.resolution, chan = c.ch;
    for (int lvl = 0; lvl < c.n_levels; ++lvl) {
        st.push_back({res, std::max(chan, c.ch * c.ch_mult[lvl]), 1});
        chan = c.ch * c.ch_mult[lvl];
        if (lvl != c.n_levels - 1) {
            res /= 2;
            st.push_back({res, chan, 4});
        }
    }
    return st;
}

// The mid-block attention over H x H tokens: up to 1 024 tokens the whole fp32 S = q k^T per image (HW^2 * 6 bytes of workspace,
// three launches per image), beyond that uspace_attention_wide_bf16 (one launch per chunk, no S) -- and also below wherever the token
// count is no multiple of the GEMM's 64-element K step, which the P.V GEMM of the first path refuses (any side that is no multiple
// of 8).  plan_ws and mid_attn both ask here.
inline bool wide_attn(int H) { return (long)H * H > 1024 || (H * H) % 64 != 0; }

// two fp32 maps and two bf16 operand buffers sized for the largest step, GroupNorm statistics, the mid-block attention's buffers
VaeWs plan_ws(const std::vector<MapStep>& steps, int B, int z_res, int c_top) {
    VaeWs w;
    size_t max_f = 0, max_h = 0;
    for (const MapStep& st : steps) {
        const size_t elems = map_rows(B, st.res) * st.chan;
        max_f = std::max(max_f, elems * 4);
        max_h = std::max(max_h, st.phases * elems * 2);
    }
    Arena a;
    w.fa = a.take(max_f); w.fb = a.take(max_f); w.hb = a.take(max_h); w.xb = a.take(max_h);
    w.stats = a.take((size_t)B * (1 + USPACE_GN_MAX_CHUNKS) * 64 * 4);
    const size_t T = (size_t)B * z_res * z_res, Cc = c_top, HW = (size_t)z_res * z_res;
    w.tok = a.take(T * Cc * 2); w.q = a.take(T * Cc * 2); w.k = a.take(T * Cc * 2); w.v = a.take(T * Cc * 2);
    if (wide_attn(z_res)) {
        // the streaming kernel keeps S and P in registers and reads V as it lies: linear in HW
        w.vt = w.s = w.pr = a.off;
    } else {
        w.vt = a.take(T * Cc * 2); w.s = a.take(HW * HW * 4); w.pr = a.take(HW * HW * 2);
    }
    w.o = a.take(T * Cc * 2);
    w.po = a.take(T * Cc * 4);
    w.total = a.off;
    return w;
}
VaeWs plan_vae_ws(const uspace_vae_config& c, const VaeModel& m, int B) { return plan_ws(dec_steps(c, m), B, m.z_res, m.c_top); }
VaeWs plan_enc_ws(const uspace_vae_config& c, const EncModel& m, int B) { return plan_ws(enc_steps(c), B, m.z_res, m.c_top); }

// What the decode and the encode share: the workspace maps, GroupNorm(+SiLU), the 9-slab 3x3 convolution, the ResnetBlock
// and the mid-block attention.  Two fp32 maps alternate as the residual stream (cur / tmp); hb / xb hold bf16 operands.
struct VaeRun {
    int B;
    hipStream_t s;
    uspace_stream_t stream;
    const char* wb;
    char* ws;
    const ParamTable* m;
    const VaeWs* w;
    float* stats;
    size_t cur_off, tmp_off;

    VaeRun(const ParamTable& m_, const VaeWs& w_, const void* blob, void* workspace, int B_, uspace_stream_t st)
        : B(B_), s((hipStream_t)st), stream(st), wb((const char*)blob), ws((char*)workspace), m(&m_), w(&w_),
          stats((float*)((char*)workspace + w_.stats)), cur_off(w_.fa), tmp_off(w_.fb) {}

    const float* PF(int i) const { return (const float*)(wb + m->p[i].offset); }
    const uint16_t* PH(int i) const { return (const uint16_t*)(wb + m->p[i].offset); }
    long rows_of(int h) const { return (long)B * (h + 2) * (h + 2); }
    static long guard(int h) { return (long)(h + 3); }
    // map pointers (row 0 sits `guard` rows into the buffer)
    float* fmap(size_t off, int h, int C) const { return (float*)(ws + off) + guard(h) * C; }
    uint16_t* hmap(size_t off, int h, int C) const { return (uint16_t*)(ws + off) + guard(h) * C; }

    int group_norm(const float* x, int h, int C, int gw, int gb, bool silu, uint16_t* y) const {
        return uspace_groupnorm_map_bf16(x, PF(gw), PF(gb), y, stats, B, h, C, silu ? 1 : 0, 1e-6f, stream);
    }
    int conv3(const uint16_t* a, int h, int Cin, int Cout, int wi, int bi, const float* resid, float* o) const {
        constexpr int B_ = USPACE_EPI_BIAS, R_ = USPACE_EPI_RESIDUAL, F_ = USPACE_EPI_OUT_F32;
        const int P = h + 2;
        int shifts[9];
        for (int t = 0; t < 9; ++t) shifts[t] = (t / 3 - 1) * P + (t % 3 - 1);
        return uspace_gemm_slabs_bf16(a, Cin, PH(wi), 9 * Cin, (int)rows_of(h), Cout, Cin, 9, shifts,
                                      resid ? (B_ | R_ | F_) : (B_ | F_), PF(bi), resid, Cout, o, Cout, nullptr, 0, stream);
    }
    // ResnetBlock (libs/autoencoder.py:73-134, temb None) on the current map, in place or into tmp (then swapped)
    int resblock(const ResIdx& r, int h) {
        constexpr int B_ = USPACE_EPI_BIAS, F_ = USPACE_EPI_OUT_F32;
        float* x = fmap(cur_off, h, r.cin);
        uint16_t* hb = hmap(w->hb, h, r.cin > r.cout ? r.cin : r.cout);
        US_TRY(group_norm(x, h, r.cin, r.n1w, r.n1b, true, hb));
        float* t1 = fmap(tmp_off, h, r.cout);
        US_TRY(conv3(hb, h, r.cin, r.cout, r.c1w, r.c1b, nullptr, t1));
        US_TRY(group_norm(t1, h, r.cout, r.n2w, r.n2b, true, hb));
        if (r.cin != r.cout) {
            // nin_shortcut (1x1) on x, written over t1 (already consumed by norm2), then conv2 accumulates onto it
            uint16_t* xb = hmap(w->xb, h, r.cin);
            US_TRY(uspace_cast_f32_bf16(x, xb, rows_of(h) * r.cin, stream));
            US_TRY(uspace_gemm_bf16(xb, r.cin, nullptr, 0, r.cin, PH(r.sw), r.cin, (int)rows_of(h), r.cout, r.cin, B_ | F_,
                                    PF(r.sb), nullptr, 0, t1, r.cout, nullptr, 0, stream));
            US_TRY(conv3(hb, h, r.cout, r.cout, r.c2w, r.c2b, t1, t1));
            std::swap(cur_off, tmp_off);
        } else {
            US_TRY(conv3(hb, h, r.cout, r.cout, r.c2w, r.c2b, x, x));   // x += conv2(...)
        }
        return USPACE_OK;
    }
    // AttnBlock over H*H tokens of Cc channels, in place on the current map
    int mid_attn(const AttnIdx& a, int H, int Cc) {
        constexpr int B_ = USPACE_EPI_BIAS, F_ = USPACE_EPI_OUT_F32, H_ = USPACE_EPI_OUT_BF16;
        const int HW = H * H;
        const long T = (long)B * HW;
        float* x = fmap(cur_off, H, Cc);
        uint16_t* hb = hmap(w->hb, H, Cc);
        US_TRY(group_norm(x, H, Cc, a.nw, a.nb, false, hb));
        uint16_t* tok = (uint16_t*)(ws + w->tok);
        hipLaunchKernelGGL(gather_interior_kernel, dim3(grid_for(T * (Cc / 8))), dim3(256), 0, s, hb, tok, B, H, H, Cc);
        US_CHECK_LAUNCH();
        uint16_t *q = (uint16_t*)(ws + w->q), *k = (uint16_t*)(ws + w->k), *v = (uint16_t*)(ws + w->v);
        uint16_t *vt = (uint16_t*)(ws + w->vt), *pr = (uint16_t*)(ws + w->pr), *o = (uint16_t*)(ws + w->o);
        float* sc = (float*)(ws + w->s);
        float* po = (float*)(ws + w->po);
        US_TRY(uspace_gemm_bf16(tok, Cc, nullptr, 0, Cc, PH(a.q_w), Cc, (int)T, Cc, Cc, B_ | H_, PF(a.q_b), nullptr, 0, nullptr, 0, q, Cc, stream));
        US_TRY(uspace_gemm_bf16(tok, Cc, nullptr, 0, Cc, PH(a.k_w), Cc, (int)T, Cc, Cc, B_ | H_, PF(a.k_b), nullptr, 0, nullptr, 0, k, Cc, stream));
        US_TRY(uspace_gemm_bf16(tok, Cc, nullptr, 0, Cc, PH(a.v_w), Cc, (int)T, Cc, Cc, B_ | H_, PF(a.v_b), nullptr, 0, nullptr, 0, v, Cc, stream));
        const float scale = 1.0f / sqrtf((float)Cc);
        if (wide_attn(H)) {
            // one streaming launch for the chunk; vt, s and pr are not reserved on this branch (plan_ws)
            US_TRY(uspace_attention_wide_bf16(q, k, v, Cc, o, Cc, B, HW, Cc, scale, stream));
        } else {
            hipLaunchKernelGGL(transpose_kernel, dim3(us_cdiv(Cc, 32), us_cdiv(HW, 32), B), dim3(256), 0, s, v, vt, HW, Cc);
            US_CHECK_LAUNCH();
        }
        for (int b = 0; b < (wide_attn(H) ? 0 : B); ++b) {
            // w_ = softmax(q k^T * c^-0.5) over keys; h_ = w_ v   (libs/autoencoder.py:179-191)
            US_TRY(uspace_gemm_bf16(q + (size_t)b * HW * Cc, Cc, nullptr, 0, Cc, k + (size_t)b * HW * Cc, Cc, HW, HW, Cc, F_,
                                    nullptr, nullptr, 0, sc, HW, nullptr, 0, stream));
            hipLaunchKernelGGL(softmax_rows_kernel, dim3(us_cdiv(HW, 4)), dim3(256), 0, s, sc, pr, (long)HW, HW, scale);
            US_CHECK_LAUNCH();
            US_TRY(uspace_gemm_bf16(pr, HW, nullptr, 0, HW, vt + (size_t)b * HW * Cc, HW, HW, Cc, HW, H_, nullptr, nullptr, 0,
                                    nullptr, 0, o + (size_t)b * HW * Cc, Cc, stream));
        }
        US_TRY(uspace_gemm_bf16(o, Cc, nullptr, 0, Cc, PH(a.po_w), Cc, (int)T, Cc, Cc, B_ | F_, PF(a.po_b), nullptr, 0, po, Cc, nullptr, 0, stream));
        hipLaunchKernelGGL(scatter_add_kernel, dim3(grid_for(T * (Cc / 4))), dim3(256), 0, s, x, po, B, H, H, Cc);
        US_CHECK_LAUNCH();
        return USPACE_OK;
    }
    // Downsample (pad (0,1,0,1), 3x3 stride 2) of the current H map into tmp at H/2, then swapped.  Tap (dy, dx) reads
    // phase (dy%2, dx%2) shifted by (dy/2, dx/2) pixels of the output layout, so it is the 9-slab GEMM with K1 = C over the
    // phase maps.  The shifts reach 3 phase maps (~3 * B * (H/2+2)^2 rows) past A: gemm.hip's a_base() adds a slab's
    // shift to the base pointer in 64 bits and builds that slab's buffer descriptor from the shifted base, so the 32-bit
    // per-lane offsets stay within one map (M * lda < 2^30, checked there).
    int downsample(int wi, int bi, int H, int C) {
        constexpr int B_ = USPACE_EPI_BIAS, F_ = USPACE_EPI_OUT_F32;
        const int Ho = H / 2, P = Ho + 2;
        const long prow = phase_rows(B, Ho);
        uint16_t* ph = hmap(w->hb, Ho, C);   // phase 0, row 0
        hipLaunchKernelGGL(downsample_phases_kernel, dim3(grid_for(4 * rows_of(Ho) * (C / 4))), dim3(256), 0, s,
                           fmap(cur_off, H, C), (bf16_t*)ph, B, H, C, prow);
        US_CHECK_LAUNCH();
        int shifts[9];
        for (int t = 0; t < 9; ++t) {
            const int dy = t / 3, dx = t % 3;
            shifts[t] = (int)(((dy & 1) * 2 + (dx & 1)) * prow) + (dy >> 1) * P + (dx >> 1);
        }
        US_TRY(uspace_gemm_slabs_bf16(ph, C, PH(wi), 9 * C, (int)rows_of(Ho), C, C, 9, shifts, B_ | F_, PF(bi), nullptr, C,
                                      fmap(tmp_off, Ho, C), C, nullptr, 0, stream));
        std::swap(cur_off, tmp_off);
        return USPACE_OK;
    }
};

}  // namespace

// GroupNorm(32, C, eps) (+ SiLU) over a zero-bordered NHWC fp32 map -> bf16 operand map (libs/autoencoder.py:31-32,26-28)
extern "C" int uspace_groupnorm_map_bf16(const float* x, const float* gamma, const float* beta, uint16_t* y,
                                         float* stats_scratch, int B, int H, int C, int silu, float eps,
                                         uspace_stream_t stream) {
    if (!x || !gamma || !beta || !y || !stats_scratch || B <= 0 || H <= 0) return USPACE_ERR_ARG;
    if (C < 64 || C > 512 || (C & (C - 1))) return USPACE_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const int chunks = std::max(1, std::min(USPACE_GN_MAX_CHUNKS, (H * H) / 64));
    int c4_log2 = 0;
    while ((4 << c4_log2) < C) ++c4_log2;
    float* partial = stats_scratch + (size_t)B * 64;
    hipLaunchKernelGGL(gn_stats_kernel, dim3(B * chunks), dim3(256), 0, s, x, partial, H, H, C, c4_log2, chunks);
    US_CHECK_LAUNCH();
    hipLaunchKernelGGL(gn_finish_kernel, dim3(B * 32), dim3(64), 0, s, partial, stats_scratch, chunks,
                       1.0f / ((float)H * (float)H * (float)(C / 32)), eps, x, H, H, C);
    US_CHECK_LAUNCH();
    const long rows = (long)B * (H + 2) * (H + 2);
    const int rs = 256 >> c4_log2;
    hipLaunchKernelGGL(gn_apply_kernel, dim3((unsigned)std::min<long>((rows + rs - 1) / rs, 8192)), dim3(256), 0, s, x,
                       stats_scratch, gamma, beta, y, B, H, H, C, c4_log2, silu ? 1 : 0);
    US_CHECK_LAUNCH();
    return USPACE_OK;
}

int us_repack_conv3(const float* src, void* dst, int co, int ci, bool to_bf16, hipStream_t s) {
    const dim3 grid(grid_for((long)co * ci * 9)), block(256);
    if (to_bf16) hipLaunchKernelGGL(repack_conv3_bf16_kernel, grid, block, 0, s, src, (bf16_t*)dst, co, ci);
    else hipLaunchKernelGGL(repack_conv3_f32_kernel, grid, block, 0, s, src, (float*)dst, co, ci);
    US_CHECK_LAUNCH();
    return USPACE_OK;
}

extern "C" int uspace_vae_num_params(const uspace_vae_config* cfg) {
    return valid_vae(cfg) ? build_vae(*cfg).n_params : USPACE_ERR_ARG;
}

extern "C" long uspace_vae_param_numel(const uspace_vae_config* cfg, int index) {
    return valid_vae(cfg) ? build_vae(*cfg).numel(index) : (long)USPACE_ERR_ARG;
}

extern "C" size_t uspace_vae_weight_bytes(const uspace_vae_config* cfg) {
    return valid_vae(cfg) ? build_vae(*cfg).bytes() : 0;
}

extern "C" size_t uspace_vae_workspace_bytes(const uspace_vae_config* cfg, int B) {
    if (!valid_vae(cfg) || B <= 0) return 0;
    return plan_vae_ws(*cfg, build_vae(*cfg), B).total;
}

extern "C" int uspace_vae_pack_weights(const uspace_vae_config* cfg, const float* const* params, int n_params,
                                       void* blob, size_t blob_bytes, uspace_stream_t stream) {
    if (!valid_vae(cfg)) return USPACE_ERR_ARG;
    return us_pack_table(build_vae(*cfg), params, n_params, blob, blob_bytes, stream);
}

static int vae_decode_impl(const uspace_vae_config* cfg, const void* blob, void* workspace, size_t workspace_bytes,
                           const float* z, float scale_factor, float* out, int B, uspace_stream_t stream,
                           int stop_after, float* dump, int* dump_hc) {
    if (!valid_vae(cfg) || !blob || !workspace || !z || !out || B <= 0 || scale_factor == 0.f) return USPACE_ERR_ARG;
    const uspace_vae_config& c = *cfg;
    const VaeModel m = build_vae(c);
    const VaeWs w = plan_vae_ws(c, m, B);
    if (workspace_bytes < w.total) return USPACE_ERR_WORKSPACE;
    VaeRun r(m, w, blob, workspace, B, stream);
    hipStream_t s = r.s;

    int stage = 0, cur_c = m.c_top;
    int H = m.z_res;   // current resolution (square)

    // ---- z/scale -> post_quant_conv -> conv_in
    hipLaunchKernelGGL(vae_conv_in_kernel, dim3(B * H * H), dim3(128), 0, s, z, 1.0f / scale_factor, r.PF(m.pq_w), r.PF(m.pq_b),
                       r.PF(m.conv_in_w), r.PF(m.conv_in_b), r.fmap(r.cur_off, H, m.c_top), H, H, m.c_top);
    US_CHECK_LAUNCH();
#define VAE_STAGE_DONE(CH)                                                                              \
    do {                                                                                                 \
        cur_c = (CH);                                                                                    \
        if (stage++ == stop_after && dump) {                                                             \
            if (hipMemcpyAsync(dump, r.fmap(r.cur_off, H, cur_c), (size_t)r.rows_of(H) * cur_c * 4,       \
                               hipMemcpyDeviceToDevice, s) != hipSuccess) return USPACE_ERR_LAUNCH;       \
            dump_hc[0] = H; dump_hc[1] = cur_c;                                                          \
            return USPACE_OK;                                                                            \
        }                                                                                                \
    } while (0)
    VAE_STAGE_DONE(m.c_top);
    // ---- mid: ResnetBlock, AttnBlock, ResnetBlock
    US_TRY(r.resblock(m.mid1, H));
    VAE_STAGE_DONE(m.c_top);
    US_TRY(r.mid_attn(m.attn, H, m.c_top));
    VAE_STAGE_DONE(m.c_top);
    US_TRY(r.resblock(m.mid2, H));
    VAE_STAGE_DONE(m.c_top);
    // ---- up path, highest level first
    for (int lvl = c.n_levels - 1; lvl >= 0; --lvl) {
        for (const ResIdx& rb : m.up[lvl]) {
            US_TRY(r.resblock(rb, H));
            VAE_STAGE_DONE(rb.cout);
        }
        if (lvl != 0) {
            const int Cc = c.ch * c.ch_mult[lvl];
            float* x = r.fmap(r.cur_off, H, Cc);
            uint16_t* hb = r.hmap(w.hb, 2 * H, Cc);
            hipLaunchKernelGGL(upsample_kernel, dim3(grid_for(r.rows_of(2 * H) * (Cc / 4))), dim3(256), 0, s, x, hb, B, H, H, Cc);
            US_CHECK_LAUNCH();
            H *= 2;
            float* y = r.fmap(r.tmp_off, H, Cc);
            US_TRY(r.conv3(hb, H, Cc, Cc, m.us_w[lvl], m.us_b[lvl], nullptr, y));
            std::swap(r.cur_off, r.tmp_off);
            VAE_STAGE_DONE(Cc);
        }
    }
    // ---- norm_out + SiLU + conv_out -> NCHW image
    {
        const int Cc = c.ch * c.ch_mult[0];
        float* x = r.fmap(r.cur_off, H, Cc);
        uint16_t* hb = r.hmap(w.hb, H, Cc);
        US_TRY(r.group_norm(x, H, Cc, m.no_w, m.no_b, true, hb));
        const long npix = (long)B * H * H;
        // 2 waves/SIMD at ~240 VGPRs: 512 workgroups fill the chip once and amortise the per-thread weight load
        const dim3 grid((unsigned)std::min<long>((npix * (Cc / 8) + 255) / 256, 512));
#define US_CONV_OUT(LPP)                                                                                              \
    hipLaunchKernelGGL(vae_conv_out_kernel<LPP>, grid, dim3(256), 0, s, (const bf16_t*)hb, r.PF(m.co_w), r.PF(m.co_b), out, B, H, H)
        switch (Cc) {
            case 64:  US_CONV_OUT(8); break;
            case 128: US_CONV_OUT(16); break;
            case 256: US_CONV_OUT(32); break;
            case 512: US_CONV_OUT(64); break;
            default: return USPACE_ERR_ARG;
        }
#undef US_CONV_OUT
        US_CHECK_LAUNCH();
    }
    return USPACE_OK;
}

extern "C" int uspace_vae_decode(const uspace_vae_config* cfg, const void* blob, void* workspace, size_t workspace_bytes,
                                 const float* z, float scale_factor, float* out, int B, uspace_stream_t stream) {
    return vae_decode_impl(cfg, blob, workspace, workspace_bytes, z, scale_factor, out, B, stream, -1, nullptr, nullptr);
}

// Test aid: run the decode up to (and including) stage `stop_after` -- 0 conv_in, 1 mid.block_1, 2 mid.attn_1,
// 3 mid.block_2, then one per res block / upsample conv in execution order -- and copy that stage's fp32
// zero-bordered NHWC map ([B, H+2, H+2, C]) to `dump`; hc_out (host) receives {H, C}.
extern "C" int uspace_vae_decode_tap(const uspace_vae_config* cfg, const void* blob, void* workspace, size_t workspace_bytes,
                                     const float* z, float scale_factor, int B, int stop_after, float* dump, int* hc_out,
                                     uspace_stream_t stream) {
    if (!dump || !hc_out || stop_after < 0) return USPACE_ERR_ARG;
    hc_out[0] = hc_out[1] = 0;
    float dummy_out = 0.f;
    (void)dummy_out;
    return vae_decode_impl(cfg, blob, workspace, workspace_bytes, z, scale_factor, dump /*unused unless the tap is past the end*/,
                           B, stream, stop_after, dump, hc_out);
}

// ------------------------------------------------------------------------------------------ encoder
extern "C" int uspace_vae_enc_num_params(const uspace_vae_config* cfg) {
    return valid_enc(cfg) ? build_enc(*cfg).n_params : USPACE_ERR_ARG;
}

extern "C" long uspace_vae_enc_param_numel(const uspace_vae_config* cfg, int index) {
    return valid_enc(cfg) ? build_enc(*cfg).numel(index) : (long)USPACE_ERR_ARG;
}

extern "C" size_t uspace_vae_enc_weight_bytes(const uspace_vae_config* cfg) {
    return valid_enc(cfg) ? build_enc(*cfg).bytes() : 0;
}

extern "C" size_t uspace_vae_enc_workspace_bytes(const uspace_vae_config* cfg, int B) {
    if (!valid_enc(cfg) || B <= 0) return 0;
    return plan_enc_ws(*cfg, build_enc(*cfg), B).total;
}

extern "C" int uspace_vae_enc_pack_weights(const uspace_vae_config* cfg, const float* const* params, int n_params,
                                           void* blob, size_t blob_bytes, uspace_stream_t stream) {
    if (!valid_enc(cfg)) return USPACE_ERR_ARG;
    return us_pack_table(build_enc(*cfg), params, n_params, blob, blob_bytes, stream);
}

static int vae_encode_impl(const uspace_vae_config* cfg, const void* blob, void* workspace, size_t workspace_bytes,
                           const float* img, float* moments, int B, uspace_stream_t stream, int stop_after, float* dump,
                           int* dump_hc) {
    if (!valid_enc(cfg) || !blob || !workspace || !img || B <= 0 || (!moments && !dump)) return USPACE_ERR_ARG;
    const uspace_vae_config& c = *cfg;
    const EncModel m = build_enc(c);
    // 32-bit element offsets (GEMM operands, GroupNorm rows): every map of the chunk stays below 2^30 elements
    for (const MapStep& st : enc_steps(c))
        if ((long)B * (st.res + 2) * (st.res + 2) * st.chan >= (1L << 30)) return USPACE_ERR_ARG;
    const VaeWs w = plan_enc_ws(c, m, B);
    if (workspace_bytes < w.total) return USPACE_ERR_WORKSPACE;
    VaeRun r(m, w, blob, workspace, B, stream);
    hipStream_t s = r.s;

    int stage = 0, cur_c = c.ch;
    int H = c.resolution;

    // ---- conv_in on the NCHW images
    {
        const long items = (long)B * H * H * (c.ch / 4);
        hipLaunchKernelGGL(vae_enc_conv_in_kernel, dim3(grid_for(items, 2048)), dim3(256), 0, s, img, r.PF(m.conv_in_w),
                           r.PF(m.conv_in_b), r.fmap(r.cur_off, H, c.ch), B, H, c.ch);
        US_CHECK_LAUNCH();
    }
    VAE_STAGE_DONE(c.ch);
    // ---- down path
    for (int lvl = 0; lvl < c.n_levels; ++lvl) {
        for (const ResIdx& rb : m.down[lvl]) {
            US_TRY(r.resblock(rb, H));
            VAE_STAGE_DONE(rb.cout);
        }
        if (lvl != c.n_levels - 1) {
            US_TRY(r.downsample(m.ds_w[lvl], m.ds_b[lvl], H, cur_c));
            H /= 2;
            VAE_STAGE_DONE(cur_c);
        }
    }
    // ---- mid: ResnetBlock, AttnBlock, ResnetBlock
    US_TRY(r.resblock(m.mid1, H));
    VAE_STAGE_DONE(m.c_top);
    US_TRY(r.mid_attn(m.attn, H, m.c_top));
    VAE_STAGE_DONE(m.c_top);
    US_TRY(r.resblock(m.mid2, H));
    VAE_STAGE_DONE(m.c_top);
    if (!moments) return USPACE_ERR_ARG;   // a tap past the last stage
    // ---- norm_out + SiLU + conv_out + quant_conv -> NCHW moments
    {
        const int Cc = m.c_top;
        uint16_t* hb = r.hmap(w.hb, H, Cc);
        US_TRY(r.group_norm(r.fmap(r.cur_off, H, Cc), H, Cc, m.no_w, m.no_b, true, hb));
        const long items = (long)B * H * ((H + 3) / 4) * (Cc / 8);
        hipLaunchKernelGGL(vae_enc_conv_out_kernel, dim3(grid_for(items, 1024)), dim3(256), 0, s, (const bf16_t*)hb,
                           r.PF(m.co_w), r.PF(m.co_b), r.PF(m.qc_w), r.PF(m.qc_b), moments, B, H, H, Cc);
        US_CHECK_LAUNCH();
    }
    return USPACE_OK;
}
#undef VAE_STAGE_DONE

extern "C" int uspace_vae_encode_moments(const uspace_vae_config* cfg, const void* blob, void* workspace,
                                         size_t workspace_bytes, const float* img, float* moments, int B,
                                         uspace_stream_t stream) {
    if (!moments) return USPACE_ERR_ARG;
    return vae_encode_impl(cfg, blob, workspace, workspace_bytes, img, moments, B, stream, -1, nullptr, nullptr);
}

// Test aid: run the encode up to (and including) stage `stop_after` -- 0 conv_in, then one per res block / downsample of
// the down path in execution order, then mid.block_1, mid.attn_1, mid.block_2 -- and copy that stage's fp32
// zero-bordered NHWC map ([B, H+2, H+2, C]) to `dump`; hc_out (host) receives {H, C}.
extern "C" int uspace_vae_encode_tap(const uspace_vae_config* cfg, const void* blob, void* workspace, size_t workspace_bytes,
                                     const float* img, int B, int stop_after, float* dump, int* hc_out,
                                     uspace_stream_t stream) {
    if (!dump || !hc_out || stop_after < 0) return USPACE_ERR_ARG;
    hc_out[0] = hc_out[1] = 0;
    return vae_encode_impl(cfg, blob, workspace, workspace_bytes, img, nullptr, B, stream, stop_after, dump, hc_out);
}

extern "C" int uspace_vae_sample(const float* moments, const float* noise, float scale, float* z, int B, int h,
                                 uspace_stream_t stream) {
    if (!moments || !noise || !z || B <= 0 || h <= 0) return USPACE_ERR_ARG;
    hipLaunchKernelGGL(vae_sample_kernel, dim3(grid_for((long)B * 4 * h * h)), dim3(256), 0, (hipStream_t)stream, moments,
                       noise, scale, z, B, h * h);
    US_CHECK_LAUNCH();
    return USPACE_OK;
}
