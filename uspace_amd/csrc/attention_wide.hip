// Single-head, non-causal attention with a WIDE head (C = 64 / 128 / 256 / 512 channels: the mid-block AttnBlock of the VAE, one head
// over all channels), any number of tokens, bf16 operands on the gfx950 matrix cores, fp32 online softmax:
//   out[b, i, :] = softmax_j(q[b, i] . k[b, j] * scale) . v[b, j, :]
// q, k, v are three token-major [B * N, C] operands with one leading dimension (what three 1x1-conv GEMMs write); no transposed V.
// The arithmetic is attention_long.hip's restated for width C, and the LDS image, its swizzles, the LDS-DMA staging and the
// transposing V read are attention_tiles.h's: a C-wide K or V tile is C / 64 PANELS side by side, each the [rows][64] image of the
// head_dim-64 kernels, staged from the operand's columns 64 p .. 64 p + 63.
//
// Budget (MI355X: 160 KiB LDS per CU, 512 VGPR + AGPR per lane for a wave that has its SIMD to itself), at C = 512:
//   O^T accumulator of a 16-query tile  16 x 512 fp32 / 64 lanes = 128 registers per lane
//   Q fragment of the tile              16 x 512 bf16 / 64 lanes =  64 registers per lane, loaded once
//   one 32-key K or V tile              32 x 512 bf16            =  32 KiB;  K and V, double-buffered = 128 KiB
// so ONE 16-query tile per wave (two would need 384 registers before any operand), at most 4 waves per workgroup (one per SIMD:
// __launch_bounds__(256) gives every wave the whole 512-entry file), 32 keys per key tile (64 would be 256 KiB), one workgroup per CU
// at C = 512.  LDS = 256 C bytes: 16 / 32 / 64 / 128 KiB.  No instantiation may use scratch (tools/kernel_resources.py).
//
// A wave owns 16 consecutive queries of one image for the whole kernel: Q fragment, running maximum m, O^T and the row sum live in
// registers.  A workgroup is NW = 4, 2 or 1 such waves (the plan picks the largest that still gives every CU a workgroup); they share
// the staged tiles and nothing else, so NW is a launch parameter, not a template parameter, and a row's instructions are the same on
// every branch of the plan.  Per key tile j (buffer j & 1), after the one barrier:
//   S^T = K . Q^T          2 x C/32 MFMAs; a lane holds, for ONE query (lane & 15), keys 4 (lane >> 4) .. + 3 of both 16-key tiles
//   [the LDS-DMA of tile j + 1 is issued here, behind the K reads: it flies during the softmax; the backend makes the V reads below
//    wait for it, since it cannot tell the two buffers apart -- plain, not tuned: DESIGN.md section 4.2a.1]
//   keys >= N (last tile only) -> -inf, before the maximum
//   m' = max(m, max S);  alpha = 2^((m - m') c);  O, sum *= alpha          (c = scale log2 e; first tile: m = -inf, alpha = 0)
//   P  = 2^(S c - m' c), rounded to bf16 ONCE: the same rounded P feeds P.V and, against an all-ones tile, the row sum
//   O^T += V^T . P^T       C/16 MFMAs, V^T fragments by ds_read_b64_tr_b16
// and O / sum once at the end.  Every key tile holds at least one real key, so m' is finite from the first tile on; the LDS rows behind
// N repeat row N - 1 (finite), their P is 0.  A query row is never split across waves or workgroups, there are no atomics, and nothing
// is read before it is written: a row's bits depend on neither B nor the grid, and repeat from run to run.
#include <algorithm>

#include "attention_tiles.h"

namespace {

constexpr int WKT = 32;                              // keys per key tile
constexpr int WPANEL_BYTES = WKT * KROW_BYTES;       // one 64-column panel of a K or V tile: 4 KiB
constexpr int wide_tile_bytes(int C) { return (C / DH) * WPANEL_BYTES; }
constexpr int wide_lds_bytes(int C) { return 4 * wide_tile_bytes(C); }     // K[2], V[2]

template <int C>
__global__ __launch_bounds__(256) void attn_wide_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ k,
                                                        const bf16_t* __restrict__ v, int ld, bf16_t* __restrict__ out, int ld_out,
                                                        int N, int nqb, float c_exp) {
    constexpr int NP = C / DH;                         // panels
    constexpr int TILE = wide_tile_bytes(C);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* sK = smem;                                   // [2][NP][WKT][64] bf16, 16-B chunks swizzled (k_off)
    char* sV = smem + 2 * TILE;                        // [2][NP][WKT][64] bf16, 32-B chunks swizzled (v_off)

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nw = (int)blockDim.x >> 6;
    const int b = blockIdx.x / nqb, qb = blockIdx.x % nqb;
    const bf16_t* gq = q + (size_t)b * N * ld;
    const bf16_t* gk = k + (size_t)b * N * ld;
    const bf16_t* gv = v + (size_t)b * N * ld;

    const int fr = lane & 15;
    const int fq = lane >> 4;
    const int nkt = (N + WKT - 1) / WKT;

    // this wave's query tile (rows >= N read row N - 1 again and are not stored; a wave whose tile lies wholly behind N still stages)
    const int q_first = (qb * nw + wave) * 16;
    bf16x8 qf[2 * NP];
    {
        int qrow = q_first + fr;
        qrow = qrow < N ? qrow : N - 1;
#pragma unroll
        for (int c = 0; c < 2 * NP; ++c) qf[c] = *(const bf16x8*)(gq + (size_t)qrow * ld + c * 32 + fq * 8);
    }
    float m = -INFINITY;
    f32x4 o[4 * NP], osum = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int d = 0; d < 4 * NP; ++d) o[d] = (f32x4){0.f, 0.f, 0.f, 0.f};
    union { uint32_t w[4]; bf16x8 v; } ones;
    ones.w[0] = ones.w[1] = ones.w[2] = ones.w[3] = 0x3f803f80u;

    // key tile j -> buffer j & 1: per panel 4 blocks of 8 rows of K and of V, dealt round-robin to the waves
    auto stage = [&](int j) {
        const int buf = j & 1, key0 = j * WKT;
#pragma unroll 1
        for (int blk = wave; blk < NP * (WKT / 8); blk += nw) {
            const int p = blk / (WKT / 8), rb = (blk % (WKT / 8)) * 8;
            const int off = buf * TILE + p * WPANEL_BYTES + rb * KROW_BYTES;
            att_dma_k8(gk + p * DH, ld, key0 + rb, N, sK + off, lane);
            att_dma_v8(gv + p * DH, ld, key0 + rb, N, sV + off, lane);
        }
    };
    stage(0);

#pragma unroll 1
    for (int j = 0; j < nkt; ++j) {
        // This wave's share of tile j has landed (waited for explicitly: the other waves read it behind the barrier), and every wave
        // is done with tile j - 1, whose buffer tile j + 1 overwrites.
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        const bool more = j + 1 < nkt;                 // workgroup-uniform
        const char* kb = sK + (j & 1) * TILE;
        const char* vb = sV + (j & 1) * TILE;

        // ---- S^T tiles: s[t][r] = <K[key0 + t*16 + 4*fq + r], Q[q + fr]>
        f32x4 s[2];
        s[0] = s[1] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int p = 0; p < NP; ++p)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const bf16x8 kf = *(const bf16x8*)(kb + p * WPANEL_BYTES + k_off(t * 16 + fr, ks * 4 + fq));
                    s[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[p * 2 + ks], s[t], 0, 0, 0);
                }
        if (more) stage(j + 1);
        // ---- mask: only the last key tile holds keys >= N
        if (!more) {
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) s[t][r] = (j * WKT + t * 16 + fq * 4 + r) < N ? s[t][r] : -INFINITY;
        }
        // ---- running row maximum; the accumulated O and sum follow it
        float mx = fmaxf(fmaxf(fmaxf(s[0][0], s[0][1]), fmaxf(s[0][2], s[0][3])), fmaxf(fmaxf(s[1][0], s[1][1]), fmaxf(s[1][2], s[1][3])));
        mx = att_max_over_rows(mx);
        const float m_new = fmaxf(m, mx);
        const float alpha = __builtin_amdgcn_exp2f((m - m_new) * c_exp);
        m = m_new;
        const float mc = m_new * c_exp;
#pragma unroll
        for (int d = 0; d < 4 * NP; ++d) o[d] *= alpha;
        osum *= alpha;
        // ---- P = 2^(s*c - m*c), rounded to bf16 once; k-slot (fq, e): e < 4 -> tile 0 key 4fq + e, e >= 4 -> tile 1
        union { uint32_t w[4]; bf16x8 v; } pu;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) s[t][r] = __builtin_amdgcn_exp2f(fmaf(s[t][r], c_exp, -mc));
        pu.w[0] = pack_bf2(s[0][0], s[0][1]);
        pu.w[1] = pack_bf2(s[0][2], s[0][3]);
        pu.w[2] = pack_bf2(s[1][0], s[1][1]);
        pu.w[3] = pack_bf2(s[1][2], s[1][3]);
        // ---- O^T += V^T . P^T, sum += 1 . P^T
#pragma unroll
        for (int p = 0; p < NP; ++p)
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                union { uint2 h[2]; bf16x8 v; } vf;
                att_read_vt(vb + p * WPANEL_BYTES, fq, fr, dt, 0, vf.h[0], vf.h[1]);
                o[p * 4 + dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf.v, pu.v, o[p * 4 + dt], 0, 0, 0);
            }
        osum = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones.v, pu.v, osum, 0, 0, 0);
    }

    // ---- store: lane holds query q_first + fr, channels d*16 + 4*fq + {0..3}
    const int qi = q_first + fr;
    if (qi < N) {
        const float inv = 1.0f / osum[0];
        bf16_t* orow = out + ((size_t)b * N + qi) * ld_out;
#pragma unroll
        for (int d = 0; d < 4 * NP; ++d) {
            uint2 pk;
            pk.x = pack_bf2(o[d][0] * inv, o[d][1] * inv);
            pk.y = pack_bf2(o[d][2] * inv, o[d][3] * inv);
            *(uint2*)(orow + d * 16 + fq * 4) = pk;
        }
    }
}

// ---- host side.  wide_plan alone decides what a call launches, wide_launch alone launches; uspace_attention_wide_plan reports the plan.
struct WidePlan { int KT, QB, NW, nqb, grid, block, lds; };     // nqb: workgroups per image = ceil(N / QB)
struct WideArgs { const bf16_t *q, *k, *v; int ld; bf16_t* out; int ld_out, B, N; float scale; hipStream_t s; };

bool wide_width(int C) { return C == 64 || C == 128 || C == 256 || C == 512; }

int wide_plan(int B, int N, int C, WidePlan* p) {
    if (B <= 0 || N <= 0 || !wide_width(C)) return USPACE_ERR_ARG;
    // rows (B * N) and the grid are ints in the kernel; element offsets are size_t
    const long long maxi = 0x7fffffffLL;
    if ((long long)B * N > maxi) return USPACE_ERR_ARG;
    // The most waves per workgroup (they share every staged tile) that still gives each of the 256 CUs a workgroup; a single image
    // of 4 096 tokens takes one wave per workgroup, 256 workgroups.  (Reasoned, not measured: DESIGN.md section 4.2a.1.)
    int NW = 1;
    if ((long long)B * us_cdiv(N, 64) >= 256) NW = 4;
    else if ((long long)B * us_cdiv(N, 32) >= 256) NW = 2;
    const int QB = 16 * NW;
    const int nqb = us_cdiv(N, QB);
    const long long grid = (long long)B * nqb;
    if (grid > maxi) return USPACE_ERR_ARG;
    *p = WidePlan{WKT, QB, NW, nqb, (int)grid, 64 * NW, wide_lds_bytes(C)};
    return USPACE_OK;
}

// The launch recorder sees the wide form as an attention launch with US_REC_ATT_WIDE in its flags: M = B, N = tokens, K = C.
template <int C>
int wide_launch(const WidePlan& p, const WideArgs& a) {
    static std::atomic<uint64_t> opted_in{0};
    const auto kernel = attn_wide_kernel<C>;
    if (wide_lds_bytes(C) > 64 * 1024) US_TRY(us_opt_in_lds((const void*)kernel, wide_lds_bytes(C), opted_in));
    const int rec = us_rec_begin(US_REC_ATTENTION, US_REC_ATT_WIDE, a.B, a.N, C, a.s);
    hipLaunchKernelGGL(kernel, dim3(p.grid), dim3(p.block), p.lds, a.s, a.q, a.k, a.v, a.ld, a.out, a.ld_out, a.N, p.nqb,
                       a.scale * 1.4426950408889634f);
    us_rec_end(rec, a.s);
    US_CHECK_LAUNCH();
    return USPACE_OK;
}

}  // namespace

extern "C" int uspace_attention_wide_plan(int B, int N, int C, int* out) {
    WidePlan p;
    if (!out) return USPACE_ERR_ARG;
    US_TRY(wide_plan(B, N, C, &p));
    const int v[6] = {p.KT, p.QB, p.NW, p.grid, p.block, p.lds};
    std::copy(v, v + 6, out);
    return USPACE_OK;
}

extern "C" int uspace_attention_wide_bf16(const uint16_t* q, const uint16_t* k, const uint16_t* v, int ld, uint16_t* out, int ld_out,
                                          int B, int N, int C, float scale, uspace_stream_t stream) {
    WidePlan p;
    if (!q || !k || !v || !out) return USPACE_ERR_ARG;
    US_TRY(wide_plan(B, N, C, &p));
    // 16-byte operand reads (LDS-DMA, Q fragments) and 8-byte stores
    if (ld < C || ld_out < C || (ld & 7) || (ld_out & 3)) return USPACE_ERR_ARG;
    if ((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v) & 15) || ((uintptr_t)out & 7)) return USPACE_ERR_ARG;
    if (!(scale > 0.f) || !(scale < INFINITY)) return USPACE_ERR_ARG;
    const WideArgs a{q, k, v, ld, out, ld_out, B, N, scale, (hipStream_t)stream};
    switch (C) {
        case 64: return wide_launch<64>(p, a);
        case 128: return wide_launch<128>(p, a);
        case 256: return wide_launch<256>(p, a);
        default: return wide_launch<512>(p, a);
    }
}
