// Head-mean attention map of one block: the picture the reference draws from the [B, H, L, L] softmax of its editable attention
// path (tools/utils_t2i.py:141-193 vis_attention_map, called at :283 BEFORE the p2p edit of :286):
//     out[b, i, j] = (1/H) * sum_h softmax_k( q[b,h,q0+i] . k[b,h,k] / 8 )[k0+j]          fp32 [B, nq, nk]
// The flash-style attention_kernel (attention.hip) never holds P -- it rounds it to bf16 tile by tile and feeds it to the next MFMA --
// so the map has a kernel of its own, run only when a map is asked for.
//
// One workgroup = one wave owns a (batch, 16-query tile) and walks the heads h = 0 .. H-1 in order:
//   S^T = K . Q^T  with the fragment layout of attention_kernel (MFMA A = 16 K rows, B = the Q fragment held in registers):
//        a lane holds, for ONE query (lane & 15), keys 4 (lane >> 4) + 0..3 of every 16-key tile, so the row max and the row sum are
//        a register sweep plus two cross-lane steps;
//   P   = exp2(S c - max c) / rowsum stays fp32 (the map is a product, not an MFMA operand) and is added to the head sum the lane keeps
//        in registers for its (query, keys); 1/H is applied once at the end.
// No atomics, no second pass, one fixed summation order: a sample's map is bit-equal from run to run and whatever batch it sits in.
// The softmax runs over ALL L keys; the window only selects what is stored.  Padding keys (>= L) are masked to -inf exactly as in
// attention_kernel; their K rows and the query rows behind the window's end read row L-1 again (finite, never stored).
// K comes straight from global memory: with one query tile per workgroup every K row feeds exactly one MFMA fragment per head, so an
// LDS image of K (what attention_kernel stages for its 17-21 query tiles) would be written once and read once.
#include "common.h"

namespace {

constexpr int DH = 64;

template <int NT>
__global__ __launch_bounds__(64) void attention_map_kernel(const bf16_t* __restrict__ qkv, float* __restrict__ out, int L, int H,
                                                           int q0, int nq, int k0, int nk) {
    const int lane = threadIdx.x;
    const int fr = lane & 15;
    const int fq = lane >> 4;
    const int b = blockIdx.y;
    const int i0 = blockIdx.x * 16;                    // first window row of this tile
    const int C3 = 3 * H * DH;
    const bf16_t* base = qkv + (size_t)b * L * C3;
    const float c_exp = 0.125f * 1.4426950408889634f;  // head_dim^-0.5 * log2(e)
    const int t_last = (L - 1) >> 4;                   // last key tile holding valid keys

    int qrow = q0 + i0 + fr;
    qrow = qrow < L ? qrow : L - 1;

    f32x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};

#pragma unroll 1
    for (int h = 0; h < H; ++h) {
        const bf16_t* gq = base + (size_t)qrow * C3 + h * DH;
        const bf16_t* gk = base + (H + h) * DH;
        bf16x8 qf[2];
        qf[0] = *(const bf16x8*)(gq + fq * 8);
        qf[1] = *(const bf16x8*)(gq + 32 + fq * 8);

        // ---- S^T tiles: s[t][r] = <K[t*16 + 4*fq + r], Q[qrow]>
        f32x4 s[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            s[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (t <= t_last) {
                int kr = t * 16 + fr;
                kr = kr < L ? kr : L - 1;
                const bf16_t* pk = gk + (size_t)kr * C3;
                const bf16x8 ka = *(const bf16x8*)(pk + fq * 8);
                const bf16x8 kb = *(const bf16x8*)(pk + 32 + fq * 8);
                s[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ka, qf[0], s[t], 0, 0, 0);
                s[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kb, qf[1], s[t], 0, 0, 0);
            }
        }
        // ---- mask: only the last valid tile can hold keys >= L; tiles after it are all invalid
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            if (t == t_last) {
#pragma unroll
                for (int r = 0; r < 4; ++r) s[t][r] = (t * 16 + fq * 4 + r) < L ? s[t][r] : -INFINITY;
            } else if (t > t_last) {
                s[t] = (f32x4){-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            }
        }
        // ---- row max over all L keys (key 0 is always valid: finite)
        float mx = s[0][0];
#pragma unroll
        for (int t = 0; t < NT; ++t) mx = fmaxf(fmaxf(mx, fmaxf(s[t][0], s[t][1])), fmaxf(s[t][2], s[t][3]));
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float mc = mx * c_exp;
        // ---- P (fp32) and its row sum over all L keys, fixed order: the lane's keys tile by tile, then the four lanes of the query
        float sum = 0.f;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                s[t][r] = __builtin_amdgcn_exp2f(fmaf(s[t][r], c_exp, -mc));
                sum += s[t][r];
            }
        }
        sum += __shfl_xor(sum, 16, 64);
        sum += __shfl_xor(sum, 32, 64);
        const float inv = 1.0f / sum;
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] += s[t] * inv;
    }

    // ---- store the window: lane holds window row i0 + fr, keys t*16 + 4*fq + {0..3}
    const int i = i0 + fr;
    if (i < nq) {
        const float inv_h = 1.0f / (float)H;
        float* orow = out + ((size_t)b * nq + i) * nk;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = t * 16 + fq * 4 + r - k0;
                if (j >= 0 && j < nk) orow[j] = acc[t][r] * inv_h;
            }
        }
    }
}

template <int NT>
int launch_map(const bf16_t* qkv, float* out, int B, int L, int H, int q0, int nq, int k0, int nk, hipStream_t s) {
    hipLaunchKernelGGL((attention_map_kernel<NT>), dim3(us_cdiv(nq, 16), B), dim3(64), 0, s, qkv, out, L, H, q0, nq, k0, nk);
    US_CHECK_LAUNCH();
    return USPACE_OK;
}

}  // namespace

extern "C" int uspace_attention_map_bf16(const uint16_t* qkv, float* out, int B, int L, int H, int q0, int nq, int k0, int nk,
                                         uspace_stream_t stream) {
    if (!qkv || !out || B <= 0 || B > 65535 || L <= 0 || H <= 0) return USPACE_ERR_ARG;
    if (q0 < 0 || nq < 1 || q0 > L - nq || k0 < 0 || nk < 1 || k0 > L - nk) return USPACE_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const int nt = (L + 15) / 16;
    if (nt <= 6) return launch_map<6>(qkv, out, B, L, H, q0, nq, k0, nk, s);
    if (nt <= 10) return launch_map<10>(qkv, out, B, L, H, q0, nq, k0, nk, s);
    if (nt <= 17) return launch_map<17>(qkv, out, B, L, H, q0, nq, k0, nk, s);
    if (nt <= 21) return launch_map<21>(qkv, out, B, L, H, q0, nq, k0, nk, s);
    return USPACE_ERR_ARG;  // sequences longer than 336 tokens do not occur on this path
}
