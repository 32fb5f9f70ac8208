// Inception Score on gfx950: the logits head of Inception-v3 (torchvision's fc, 2048 -> 1008 in the pytorch-fid file) over
// the pool features of csrc/inception.hip, and the fp64 statistics of the score.
//
// Logits: fp32 operands on v_mfma_f32_32x32x2_f32, operands straight from global memory (4 MFLOP per image next to the
// network's 11.4 GFLOP: correct and deterministic, not tuned).  The instruction is bit-for-bit a k-ordered fp32 fma chain,
// so logits[i, n] = fma(..fma(x[i,0] w[n,0], 0)..) over k = 0 .. K - 1, then + bias[n]: a row's logits do not depend on the
// batch it sits in.
//
// Score (Salimans et al. 2016), per split k of rows [k N / splits, (k + 1) N / splits) (integer division):
//   p_i = softmax(logits_i),  pbar = mean_i p_i,  score_k = exp(mean_i sum_c p_ic (log p_ic - log pbar_c)),  0 log 0 = 0.
// Everything is fp64 from the fp32 logits, and every sum has one fixed order that no launch parameter changes: a row's sums
// over classes are 64 lane-strided chains joined by a butterfly, a column's sum over a split's rows is a chain per block of
// kRowChunk rows and then a chain over the blocks, a split's sum over its rows again lane-strided chains and a butterfly.
// No atomics.
#include <math.h>

#include "common.h"

namespace {

// ---- logits.  Workgroup = 128 rows x 32 columns, one 32 x 32 accumulator per wave.  Lane l supplies A[i = l & 31][k = l >> 5]
// and B[k = l >> 5][j = l & 31]: per 16 k it loads the 16 consecutive values of its row of x and of its row of W (K % 16 == 0
// keeps them 64-byte aligned) and feeds element 2 kk + (l >> 5) to step kk.  Rows and columns beyond the matrix are clamped
// for the loads and never stored.
__global__ __launch_bounds__(256) void logits_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                     const float* __restrict__ bias, float* __restrict__ out, int B, int K, int C) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l32 = lane & 31, kh = lane >> 5;
    const int m0 = blockIdx.x * 128 + wave * 32, n0 = blockIdx.y * 32;
    if (m0 >= B) return;                                   // whole wave: no barrier follows
    const float* xa = x + (size_t)min(m0 + l32, B - 1) * K;
    const float* wb = w + (size_t)min(n0 + l32, C - 1) * K;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int k0 = 0; k0 < K; k0 += 16) {
        f32x4 a[4], b[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            a[q] = *(const f32x4*)(xa + k0 + 4 * q);
            b[q] = *(const f32x4*)(wb + k0 + 4 * q);
        }
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) {
            const float av = kh ? a[kk >> 1][2 * (kk & 1) + 1] : a[kk >> 1][2 * (kk & 1)];
            const float bv = kh ? b[kk >> 1][2 * (kk & 1) + 1] : b[kk >> 1][2 * (kk & 1)];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
        }
    }
    // C/D of the 32x32 MFMA: column = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
    const int n = n0 + l32;
    if (n >= C) return;
    const float bn = bias ? bias[n] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = m0 + (r & 3) + 8 * (r >> 2) + 4 * kh;
        if (m < B) out[(size_t)m * C + n] = bias ? acc[r] + bn : acc[r];
    }
}

// ---- score statistics
constexpr int kRowChunk = 256;      // rows per partial column sum (a constant of the summation order, not of the launch)

__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

__device__ __forceinline__ int split_lo(int k, int N, int splits) { return (int)((long)k * N / splits); }

// lse[i] = log sum_c exp(logits[i, c]); one wave per row
__global__ __launch_bounds__(256) void is_lse_kernel(const float* __restrict__ logits, double* __restrict__ lse, int N, int C) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= N) return;
    const float* p = logits + (size_t)row * C;
    double m = -INFINITY;
    for (int c = lane; c < C; c += 64) m = fmax(m, (double)p[c]);
    m = wave_max_f64(m);
    double s = 0.0;
    for (int c = lane; c < C; c += 64) s += exp((double)p[c] - m);
    s = wave_sum_f64(s);
    if (lane == 0) lse[row] = m + log(s);
}

// part[(k * chunks + j), c] = sum of p[i, c] over rows i of block j of split k, in row order; one thread per column
__global__ __launch_bounds__(128) void is_colsum_kernel(const float* __restrict__ logits, const double* __restrict__ lse,
                                                        double* __restrict__ part, int N, int C, int splits, int chunks) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    const int k = blockIdx.y / chunks, j = blockIdx.y - k * chunks;
    if (c >= C) return;
    const int lo = split_lo(k, N, splits) + j * kRowChunk;
    const int hi = min(lo + kRowChunk, split_lo(k + 1, N, splits));
    double s = 0.0;
    for (int i = lo; i < hi; ++i) s += exp((double)logits[(size_t)i * C + c] - lse[i]);
    part[(size_t)blockIdx.y * C + c] = s;
}

// logpbar[k, c] = log((sum_j part[(k, j), c]) / n_k), blocks in order; log 0 = -inf (no term of the score reads it: then every
// p[i, c] of the split is 0)
__global__ __launch_bounds__(128) void is_marginal_kernel(const double* __restrict__ part, double* __restrict__ logpbar, int N,
                                                          int C, int splits, int chunks) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x, k = blockIdx.y;
    if (c >= C) return;
    const int n = split_lo(k + 1, N, splits) - split_lo(k, N, splits);
    const int used = (n + kRowChunk - 1) / kRowChunk;
    double s = 0.0;
    for (int j = 0; j < used; ++j) s += part[((size_t)k * chunks + j) * C + c];
    logpbar[(size_t)k * C + c] = log(s / n);
}

// kl[i] = sum_c p_ic (log p_ic - log pbar_c) with log p_ic = logits[i, c] - lse[i]; terms with p_ic == 0 are skipped; one wave
// per row
__global__ __launch_bounds__(256) void is_kl_kernel(const float* __restrict__ logits, const double* __restrict__ lse,
                                                    const double* __restrict__ logpbar, double* __restrict__ kl, int N, int C,
                                                    int splits) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= N) return;
    // the split of this row: the largest k with k N / splits <= row
    int k = (int)(((long)row * splits) / N);
    while (k + 1 < splits && split_lo(k + 1, N, splits) <= row) ++k;
    while (k > 0 && split_lo(k, N, splits) > row) --k;
    const float* p = logits + (size_t)row * C;
    const double* lq = logpbar + (size_t)k * C;
    const double l = lse[row];
    double s = 0.0;
    for (int c = lane; c < C; c += 64) {
        const double lp = (double)p[c] - l;
        const double pr = exp(lp);
        if (pr > 0.0) s += pr * (lp - lq[c]);
    }
    s = wave_sum_f64(s);
    if (lane == 0) kl[row] = s;
}

// scores[k] = exp(mean of kl over the rows of split k); one wave per split
__global__ __launch_bounds__(64) void is_score_kernel(const double* __restrict__ kl, double* __restrict__ scores, int N,
                                                      int splits) {
    const int k = blockIdx.x, lane = threadIdx.x;
    const int lo = split_lo(k, N, splits), hi = split_lo(k + 1, N, splits);
    double s = 0.0;
    for (int i = lo + lane; i < hi; i += 64) s += kl[i];
    s = wave_sum_f64(s);
    if (lane == 0) scores[k] = exp(s / (hi - lo));
}

constexpr int kMaxRows = 1 << 24;

int score_chunks(int N, int splits) { return us_cdiv(us_cdiv(N, splits), kRowChunk); }

// (splits * chunks is a grid dimension)
bool score_args_ok(int N, int C, int splits) {
    if (N < 1 || N > kMaxRows || C < 1 || C > 65536 || splits < 1 || splits > N) return false;
    return (long)splits * score_chunks(N, splits) <= 65535;
}

}  // namespace

extern "C" int uspace_inception_logits(const float* pool, const float* weight, const float* bias, float* logits, int B, int K,
                                       int C, uspace_stream_t stream) {
    if (!pool || !weight || !logits || B < 1 || C < 1 || K < 16 || K % 16 != 0) return USPACE_ERR_ARG;
    if ((((uintptr_t)pool | (uintptr_t)weight) & 15) != 0) return USPACE_ERR_ARG;      // 16-byte loads
    if ((long)B * K >= (1L << 31) || (long)C * K >= (1L << 31) || (long)B * C >= (1L << 31) || us_cdiv(C, 32) > 65535)
        return USPACE_ERR_ARG;
    hipLaunchKernelGGL(logits_kernel, dim3(us_cdiv(B, 128), us_cdiv(C, 32)), dim3(256), 0, (hipStream_t)stream, pool, weight,
                       bias, logits, B, K, C);
    US_CHECK_LAUNCH();
    return USPACE_OK;
}

extern "C" size_t uspace_inception_score_workspace_bytes(int N, int C, int splits) {
    if (!score_args_ok(N, C, splits)) return 0;
    // lse [N], kl [N], logpbar [splits, C], part [splits * chunks, C]
    return (2 * (size_t)N + (size_t)splits * C + (size_t)splits * score_chunks(N, splits) * C) * sizeof(double);
}

extern "C" int uspace_inception_score_f64(const float* logits, int N, int C, int splits, void* workspace, size_t workspace_bytes,
                                          double* scores, uspace_stream_t stream) {
    if (!logits || !workspace || !scores || !score_args_ok(N, C, splits)) return USPACE_ERR_ARG;
    if (workspace_bytes < uspace_inception_score_workspace_bytes(N, C, splits)) return USPACE_ERR_WORKSPACE;
    const int chunks = score_chunks(N, splits);
    double* lse = (double*)workspace;
    double* kl = lse + N;
    double* logpbar = kl + N;
    double* part = logpbar + (size_t)splits * C;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(is_lse_kernel, dim3(us_cdiv(N, 4)), dim3(256), 0, st, logits, lse, N, C);
    US_CHECK_LAUNCH();
    hipLaunchKernelGGL(is_colsum_kernel, dim3(us_cdiv(C, 128), splits * chunks), dim3(128), 0, st, logits, lse, part, N, C,
                       splits, chunks);
    US_CHECK_LAUNCH();
    hipLaunchKernelGGL(is_marginal_kernel, dim3(us_cdiv(C, 128), splits), dim3(128), 0, st, part, logpbar, N, C, splits, chunks);
    US_CHECK_LAUNCH();
    hipLaunchKernelGGL(is_kl_kernel, dim3(us_cdiv(N, 4)), dim3(256), 0, st, logits, lse, logpbar, kl, N, C, splits);
    US_CHECK_LAUNCH();
    hipLaunchKernelGGL(is_score_kernel, dim3(splits), dim3(64), 0, st, kl, scores, N, splits);
    US_CHECK_LAUNCH();
    return USPACE_OK;
}
