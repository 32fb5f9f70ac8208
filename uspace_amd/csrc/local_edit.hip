// Local edits (uspace_amd/tools/local_edit.py, CNF.decode_local): the blend of the two branches of a paired solve and the two ways
// a mask is made -- from a label map (a face parser) and from the image x word attention maps of one evaluation.  All three are
// memory-bound and small next to a network evaluation; none uses atomics, every sum runs in one fixed order, and a sample's mask
// does not depend on the batch it sits in.
#include "common.h"

namespace {

template <int W> struct vec_t { using type = float; };
template <> struct vec_t<4> { using type = f32x4; };

inline unsigned grid_cap(long n) {
    const long g = (n + 255) / 256;
    return (unsigned)(g < 1 ? 1 : (g > 2048 ? 2048 : g));
}

// m <= 0 (and NaN): the source, bit for bit; m >= 1: the edited branch, bit for bit; between: one subtraction, one fused multiply-add
__device__ __forceinline__ float blend1(float s, float e, float m) {
    if (m >= 1.f) return e;
    if (!(m > 0.f)) return s;
    return __builtin_fmaf(m, e - s, s);
}

// pair [2B, C, cells] -> out rows [0, B) = the source rows, row B + b = blend(source b, edited b, mask[b]).  `out` may be `pair`:
// every element is read and written by the same thread, the reads first; then the source rows are left alone (copy == 0).
// Indices count vectors of W floats: row = C * cells / W, cw = cells / W, total = B * row.
template <int W>
__global__ __launch_bounds__(256) void pair_blend_kernel(const float* pair, const float* __restrict__ mask, float* out, long row, long cw,
                                                         long total, int copy) {
    using vec = typename vec_t<W>::type;
    const vec* src = (const vec*)pair;
    const vec* edt = src + total;
    vec* osrc = (vec*)out;
    vec* oedt = osrc + total;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long b = i / row;
        const long p = (i - b * row) % cw;
        const vec m = ((const vec*)mask)[b * cw + p];
        const vec s = src[i], e = edt[i];
        vec v;
        if constexpr (W == 4) {
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = blend1(s[k], e[k], m[k]);
        } else {
            v = blend1(s, e, m);
        }
        if (copy) osrc[i] = s;
        oedt[i] = v;
    }
}

constexpr int LABELS_MAX_S = 64;

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// One workgroup per sample (a mask is made once per edit, not once per evaluation).  Pass 1: a wave per cell counts the member
// pixels of its ch x cw pixels (integers), share = count / (ch * cw) goes to LDS.  Pass 2: a thread per cell takes the maximum of
// the shares over its (2 dilate + 1)^2 window, clipped at the border.
__global__ __launch_bounds__(256) void mask_from_labels_kernel(const uint8_t* __restrict__ labels, int H, int W, const uint8_t* __restrict__ member,
                                                               int S, int dilate, float thr, int soft, float* __restrict__ mask) {
    __shared__ float share[LABELS_MAX_S * LABELS_MAX_S];
    __shared__ uint8_t in_set[256];
    const int b = blockIdx.x;
    const int ch = H / S, cw = W / S, npx = ch * cw;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    in_set[threadIdx.x] = member[threadIdx.x];  // blockDim.x == 256
    __syncthreads();
    const uint8_t* lb = labels + (size_t)b * H * W;
    const float denom = (float)npx;
    for (int cell = wave; cell < S * S; cell += nwaves) {
        const int cy = cell / S, cx = cell - cy * S;
        const uint8_t* base = lb + (size_t)cy * ch * W + (size_t)cx * cw;
        int count = 0;
        for (int q = lane; q < npx; q += 64) {
            const int py = q / cw, px = q - py * cw;
            count += in_set[base[(size_t)py * W + px]] ? 1 : 0;
        }
        count = wave_sum_int(count);
        if (lane == 0) share[cell] = (float)count / denom;
    }
    __syncthreads();
    float* mb = mask + (size_t)b * S * S;
    for (int cell = threadIdx.x; cell < S * S; cell += blockDim.x) {
        const int cy = cell / S, cx = cell - cy * S;
        const int y0 = max(cy - dilate, 0), y1 = min(cy + dilate, S - 1);
        const int x0 = max(cx - dilate, 0), x1 = min(cx + dilate, S - 1);
        float v = 0.f;                          // shares are >= 0
        for (int y = y0; y <= y1; ++y)
            for (int x = x0; x <= x1; ++x) v = fmaxf(v, share[y * S + x]);
        mb[cell] = soft ? v : (v > thr ? 1.f : 0.f);
    }
}

constexpr int MAPS_MAX_G = 64;

// One workgroup per sample row.  A thread per token cell p sums a[p] = sum_blk w[blk] * (sum_j cols[j] * maps[blk, r, p, j]) in fp32,
// blocks ascending, columns ascending, one fused multiply-add per term; blocks of weight 0 and columns of weight 0 are left out
// (both are the same for the whole workgroup: no divergence, and with a few chosen words most of the maps are never read).
// Then the 3 x 3 maximum clipped at the border, the row's maximum (a maximum has no order), the division, the patch x patch spread.
__global__ __launch_bounds__(256) void mask_from_maps_kernel(const float* __restrict__ maps, int n_blocks, int R, int G, int nk,
                                                             const float* __restrict__ block_w, const float* __restrict__ cols, int patch,
                                                             float thr, int soft, float* __restrict__ mask) {
    __shared__ float a[MAPS_MAX_G * MAPS_MAX_G];
    __shared__ float pooled[MAPS_MAX_G * MAPS_MAX_G];
    __shared__ float wmax[4];
    const int r = blockIdx.x;
    const int np = G * G;
    const float* cr = cols + (size_t)r * nk;
    for (int p = threadIdx.x; p < np; p += blockDim.x) {
        float acc = 0.f;
        for (int blk = 0; blk < n_blocks; ++blk) {
            const float w = block_w[blk];
            if (w == 0.f) continue;
            const float* mp = maps + (((size_t)blk * R + r) * np + p) * nk;
            float inner = 0.f;
            for (int j = 0; j < nk; ++j) {
                const float c = cr[j];
                if (c != 0.f) inner = __builtin_fmaf(c, mp[j], inner);
            }
            acc = __builtin_fmaf(w, inner, acc);
        }
        a[p] = acc;
    }
    __syncthreads();
    float best = -INFINITY;
    for (int p = threadIdx.x; p < np; p += blockDim.x) {
        const int gy = p / G, gx = p - gy * G;
        const int y0 = max(gy - 1, 0), y1 = min(gy + 1, G - 1), x0 = max(gx - 1, 0), x1 = min(gx + 1, G - 1);
        float v = -INFINITY;
        for (int y = y0; y <= y1; ++y)
            for (int x = x0; x <= x1; ++x) v = fmaxf(v, a[y * G + x]);
        pooled[p] = v;
        best = fmaxf(best, v);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) best = fmaxf(best, __shfl_xor(best, o, 64));
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = best;
    __syncthreads();
    const float top = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
    const bool live = top > 0.f;                // a maximum of 0 (no chosen word, or no attention on it) or below: no edit anywhere
    const int side = G * patch;
    float* mr = mask + (size_t)r * side * side;
    for (int q = threadIdx.x; q < side * side; q += blockDim.x) {
        const int y = q / side, x = q - y * side;
        float v = 0.f;
        if (live) {
            v = pooled[(y / patch) * G + (x / patch)] / top;
            if (!soft) v = v > thr ? 1.f : 0.f;
        }
        mr[q] = v;
    }
}

}  // namespace

extern "C" int uspace_pair_blend(const float* pair, const float* mask, int B, int C, long cells, float* out, uspace_stream_t stream) {
    if (!pair || !mask || !out || B <= 0 || C <= 0 || cells <= 0) return USPACE_ERR_ARG;
    const long row = (long)C * cells, total = (long)B * row;
    // in place, or disjoint from the 2B rows read
    const uintptr_t p0 = (uintptr_t)pair, o0 = (uintptr_t)out, bytes = (uintptr_t)(2 * total) * sizeof(float);
    if (o0 != p0 && o0 < p0 + bytes && p0 < o0 + bytes) return USPACE_ERR_ARG;
    const int copy = out != pair;
    hipStream_t s = (hipStream_t)stream;
    if ((cells & 3) == 0 && !((p0 | o0 | (uintptr_t)mask) & 15)) {
        hipLaunchKernelGGL(pair_blend_kernel<4>, dim3(grid_cap(total >> 2)), dim3(256), 0, s, pair, mask, out, row >> 2, cells >> 2,
                           total >> 2, copy);
    } else {
        hipLaunchKernelGGL(pair_blend_kernel<1>, dim3(grid_cap(total)), dim3(256), 0, s, pair, mask, out, row, cells, total, copy);
    }
    US_CHECK_LAUNCH();
    return USPACE_OK;
}

extern "C" int uspace_mask_from_labels(const uint8_t* labels, int B, int H, int W, const uint8_t* member, int S, int dilate, float thr,
                                       int soft, float* mask, uspace_stream_t stream) {
    if (!labels || !member || !mask || B <= 0 || B > 65535 || S < 1 || S > LABELS_MAX_S || H < S || W < S || H > 16384 || W > 16384) return USPACE_ERR_ARG;
    if (H % S || W % S || dilate < 0 || dilate > 4) return USPACE_ERR_ARG;
    hipLaunchKernelGGL(mask_from_labels_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, labels, H, W, member,
                       S, dilate, thr, soft, mask);
    US_CHECK_LAUNCH();
    return USPACE_OK;
}

extern "C" int uspace_mask_from_maps(const float* maps, int n_blocks, int R, int G, int nk, const float* block_w, const float* cols,
                                     int patch, float thr, int soft, float* mask, uspace_stream_t stream) {
    if (!maps || !block_w || !cols || !mask || n_blocks <= 0 || R <= 0 || R > 65535 || G < 1 || G > MAPS_MAX_G || nk <= 0) return USPACE_ERR_ARG;
    if (patch < 1 || patch > 16) return USPACE_ERR_ARG;
    hipLaunchKernelGGL(mask_from_maps_kernel, dim3(R), dim3(256), 0, (hipStream_t)stream, maps, n_blocks, R, G, nk, block_w, cols, patch,
                       thr, soft, mask);
    US_CHECK_LAUNCH();
    return USPACE_OK;
}
