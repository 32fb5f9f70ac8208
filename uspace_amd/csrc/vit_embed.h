// The front of a ViT image tower, shared by clip_vision.hip and dino.hip: patch rows for the patch-embedding GEMM, the padded patch
// weight, class token + position table, and the gather of one token row.  Kernels only; each tower keeps its own launches.
#pragma once
#include "common.h"

namespace {

// rows[b * N + gy * G + gx][k], k = (c, py, px) -> pixel_values[b, c, gy p + py, gx p + px] as bf16; columns K .. Kp - 1 are zero.
// One block per patch row.
__global__ __launch_bounds__(256) void patch_rows_kernel(const float* __restrict__ pv, bf16_t* __restrict__ rows, int S, int p, int G,
                                                         int K, int Kp) {
    const int row = blockIdx.x;
    const int N = G * G, b = row / N, i = row - b * N, gy = i / G, gx = i - gy * G;
    const int pp = p * p;
    bf16_t* dst = rows + (size_t)row * Kp;
    for (int k = threadIdx.x; k < Kp; k += 256) {
        float v = 0.0f;
        if (k < K) {
            const int c = k / pp, r = k - c * pp, py = r / p, px = r - py * p;
            v = pv[((size_t)(b * 3 + c) * S + gy * p + py) * S + gx * p + px];
        }
        dst[k] = f2bf(v);
    }
}

// x[b, 0] = cls + pos[0];  x[b, 1 + i] = patch[b, i] + pos[1 + i]  (HF CLIPVisionEmbeddings); one block per token row, fp32
__global__ __launch_bounds__(256) void assemble_tokens_kernel(const float* __restrict__ patch, const float* __restrict__ cls,
                                                              const float* __restrict__ pos, float* __restrict__ x, int T, int D) {
    const int row = blockIdx.x, b = row / T, t = row - b * T;
    const float* a = t == 0 ? cls : patch + ((size_t)b * (T - 1) + (t - 1)) * D;
    const float* pr = pos + (size_t)t * D;
    for (int d = threadIdx.x * 4; d < D; d += 1024) *(f32x4*)(x + (size_t)row * D + d) = *(const f32x4*)(a + d) + *(const f32x4*)(pr + d);
}

// out[b, :] = x[b, idx[b], :] of x [B, L, D]; idx == NULL: row 0 (the class token).  One block per sample; an index outside
// [0, L) is clamped (validated on the host).
__global__ __launch_bounds__(256) void gather_rows_kernel(const float* __restrict__ x, const int* __restrict__ idx, float* __restrict__ out,
                                                          int L, int D) {
    const int b = blockIdx.x;
    int r = idx ? idx[b] : 0;
    r = r < 0 ? 0 : (r >= L ? L - 1 : r);
    const float* src = x + ((size_t)b * L + r) * D;
    for (int d = threadIdx.x; d < D; d += 256) out[(size_t)b * D + d] = src[d];
}

// bf16 [D, K] dense (the staging area behind the table) -> [D, Kp] with zero pad columns (the table's region); one block per row
__global__ __launch_bounds__(256) void pad_patch_rows_kernel(const bf16_t* __restrict__ dense, bf16_t* __restrict__ padded, int K, int Kp) {
    const int d = blockIdx.x;
    for (int k = threadIdx.x; k < Kp; k += 256) padded[(size_t)d * Kp + k] = k < K ? dense[(size_t)d * K + k] : (bf16_t)0;
}

}  // namespace
