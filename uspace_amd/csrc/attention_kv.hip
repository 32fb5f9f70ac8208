// Attention with few resident keys and many queries (SegFormer's spatially reduced attention: the keys and values of a block are a
// map reduced by sr x sr, at most 336 rows, the queries every pixel -- 16 384 of them at 512^2 in stage 0, with ONE head).
// head_dim 64, bf16 operands on the matrix cores, fp32 softmax.  q and k | v are separate tensors with their own row strides.
//
// K and V of a (sample, head) are resident in LDS in the image and swizzles of attention_tiles.h, staged by LDS-DMA; the arithmetic
// of a query row is the resident kernel's (attention.hip, generic length): S^T = K . Q^T, fp32 row maximum, P = exp2(S c - max c)
// rounded once to bf16, O^T = V^T . P^T, the row sum from one more MFMA against an all-ones tile, one reciprocal.  What differs is
// who owns what: attention.hip gives one workgroup a whole (sample, head) and, for small batches, interleaves a head's query tiles
// over a few workgroups.  Here a head has up to a thousand query tiles, so they are cut into contiguous chunks of `chunk` tiles, one
// workgroup each, and every workgroup stages K and V once for its chunk.  A query row lives in one lane column of one wave's tile and
// never leaves it: its bits do not depend on the chunking, on the batch or on its place in either.
//
// The chunk rule (att_kv_plan) is reasoned, not measured: enough workgroups to give every CU its resident share (two 4-wave
// workgroups, one 8-wave workgroup), but no chunk below one query tile per wave: that is where the resident kernel's small-batch
// form stops splitting a head too (attention.hip, QS = ceil(NT / NW)), and below it a wave would stage up to 86 KB for nothing.
#include "attention_tiles.h"

namespace {

constexpr int kv_k_rows(int NT) { return NT * 16; }
constexpr int kv_v_rows(int NT) { return (NT + 1) / 2 * 32; }
constexpr int kv_lds_bytes(int NT) { return (kv_k_rows(NT) + kv_v_rows(NT)) * KROW_BYTES; }

// NT: 16-key tiles compiled for (keys >= Lk are masked, tiles beyond the last valid one skipped); NW: waves per workgroup.
template <int NT, int NW>
__global__ __launch_bounds__(64 * NW, 2) void attention_kv_kernel(const bf16_t* __restrict__ q, int ldq, const bf16_t* __restrict__ kv,
                                                                  int ldkv, bf16_t* __restrict__ out, int ldo, int Lq, int Lk, int H,
                                                                  int chunk, int nchunks) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NP = (NT + 1) / 2;
    constexpr int VROWS = kv_v_rows(NT);
    constexpr int KROWS = kv_k_rows(NT);
    char* sK = smem;
    char* sV = smem + KROWS * KROW_BYTES;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int bh = blockIdx.x / nchunks;
    const int ck = blockIdx.x % nchunks;
    const int b = bh / H, h = bh % H;
    const bf16_t* gq = q + (size_t)b * Lq * ldq + h * DH;
    const bf16_t* gk = kv + (size_t)b * Lk * ldkv + h * DH;
    const bf16_t* gv = gk + H * DH;

#pragma unroll
    for (int blk = 0; blk < (KROWS / 8 + NW - 1) / NW; ++blk) {
        const int rb = (blk * NW + wave) * 8;
        if (rb < KROWS) att_dma_k8(gk, ldkv, rb, Lk, sK + rb * KROW_BYTES, lane);
    }
#pragma unroll
    for (int blk = 0; blk < (VROWS / 8 + NW - 1) / NW; ++blk) {
        const int rb = (blk * NW + wave) * 8;
        if (rb < VROWS) att_dma_v8(gv, ldkv, rb, Lk, sV + rb * KROW_BYTES, lane);
    }

    const int fr = lane & 15;
    const int fq = lane >> 4;
    const float c_exp = 0.125f * 1.4426950408889634f;  // head_dim^-0.5 * log2(e)
    const int n_qt = (Lq + 15) >> 4;
    const int qt_end = (ck + 1) * chunk < n_qt ? (ck + 1) * chunk : n_qt;      // this workgroup's tiles: ck * chunk .. qt_end - 1
    const int t_last = (Lk - 1) >> 4;

    auto load_q = [&](int qt, bf16x8 (&qf)[2]) {
        int qrow = qt * 16 + fr;
        qrow = qrow < Lq ? qrow : Lq - 1;
        qf[0] = *(const bf16x8*)(gq + (size_t)qrow * ldq + fq * 8);
        qf[1] = *(const bf16x8*)(gq + (size_t)qrow * ldq + 32 + fq * 8);
    };
    bf16x8 qf[2], qn[2];
    const int qfirst = ck * chunk + wave;
    load_q(qfirst < qt_end ? qfirst : ck * chunk, qf);
    __syncthreads();   // (drains the LDS-DMA queue) K and V visible

#pragma unroll 1
    for (int qt = qfirst; qt < qt_end; qt += NW) {
        const int q0 = qt * 16;
        load_q(qt + NW < qt_end ? qt + NW : qt, qn);
        int lds_k = 0;
        asm volatile("" : "+v"(lds_k));      // keeps the K fragment reads inside the loop (attention.hip)

        f32x4 s[NT];
        {
            constexpr int TQ = 4, NQD = (NT + TQ - 1) / TQ;
            bf16x8 kb[2][TQ][2];
            auto load_kq = [&](int qd, bf16x8 (&dst)[TQ][2]) {
#pragma unroll
                for (int j = 0; j < TQ; ++j) {
                    const int t = qd * TQ + j;
                    if (t < NT && t <= t_last) {
                        dst[j][0] = *(const bf16x8*)(sK + lds_k + k_off(t * 16 + fr, fq));
                        dst[j][1] = *(const bf16x8*)(sK + lds_k + k_off(t * 16 + fr, 4 + fq));
                    }
                }
            };
#pragma unroll
            for (int t = 0; t < NT; ++t) s[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
            load_kq(0, kb[0]);
#pragma unroll
            for (int qd = 0; qd < NQD; ++qd) {
                if (qd + 1 < NQD) load_kq(qd + 1, kb[(qd + 1) & 1]);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                    for (int j = 0; j < TQ; ++j) {
                        const int t = qd * TQ + j;
                        if (t < NT && t <= t_last)
                            s[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kb[qd & 1][j][ks], qf[ks], s[t], 0, 0, 0);
                    }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            if (t == t_last) {
#pragma unroll
                for (int r = 0; r < 4; ++r) s[t][r] = (t * 16 + fq * 4 + r) < Lk ? s[t][r] : -INFINITY;
            } else if (t > t_last) {
                s[t] = (f32x4){-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            }
        }
        float mq[4] = {s[0][0], s[0][0], s[0][0], s[0][0]};
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            mq[(2 * t) & 3] = fmaxf(fmaxf(mq[(2 * t) & 3], s[t][0]), s[t][1]);
            mq[(2 * t + 1) & 3] = fmaxf(fmaxf(mq[(2 * t + 1) & 3], s[t][2]), s[t][3]);
        }
        float mx = fmaxf(fmaxf(mq[0], mq[1]), fmaxf(mq[2], mq[3]));
        mx = att_max_over_rows(mx);
        const float mc = mx * c_exp;
        auto exp_step = [&](int u) {
#pragma unroll
            for (int tt = 2 * u; tt < 2 * u + 2 && tt < NT; ++tt)
#pragma unroll
                for (int r = 0; r < 4; ++r) s[tt][r] = __builtin_amdgcn_exp2f(fmaf(s[tt][r], c_exp, -mc));
        };
        f32x4 o[4], osum = (f32x4){0.f, 0.f, 0.f, 0.f};
        union { uint32_t w[4]; bf16x8 v; } ones;
        ones.w[0] = ones.w[1] = ones.w[2] = ones.w[3] = 0x3f803f80u;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
        union VF { uint2 h[2]; bf16x8 v; };
        union PF { uint32_t w[4]; bf16x8 v; };
        VF vb[2][4];
        PF pb[2];
        auto load_v = [&](int u, VF (&dst)[4]) {
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) att_read_vt(sV, fq, fr, dt, u * (32 * KROW_BYTES), dst[dt].h[0], dst[dt].h[1]);
        };
        auto make_p = [&](int u) {
            exp_step(u);
            PF& pf = pb[u & 1];
            pf.w[0] = pack_bf2(s[2 * u][0], s[2 * u][1]);
            pf.w[1] = pack_bf2(s[2 * u][2], s[2 * u][3]);
            if (2 * u + 1 < NT) {
                pf.w[2] = pack_bf2(s[2 * u + 1][0], s[2 * u + 1][1]);
                pf.w[3] = pack_bf2(s[2 * u + 1][2], s[2 * u + 1][3]);
            } else {
                pf.w[2] = 0u;
                pf.w[3] = 0u;
            }
        };
        load_v(0, vb[0]);
        make_p(0);
#pragma unroll
        for (int u = 0; u < NP; ++u) {
            if (2 * u <= t_last) {
                const bool more = (u + 1 < NP) && (2 * (u + 1) <= t_last);
                if (more) load_v(u + 1, vb[(u + 1) & 1]);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int dt = 0; dt < 4; ++dt)
                    o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vb[u & 1][dt].v, pb[u & 1].v, o[dt], 0, 0, 0);
                osum = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones.v, pb[u & 1].v, osum, 0, 0, 0);
                if (more) make_p(u + 1);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        const float inv = 1.0f / osum[0];
        const int qi = q0 + fr;
        if (qi < Lq) {
            bf16_t* orow = out + ((size_t)b * Lq + qi) * ldo + h * DH;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                uint2 p;
                p.x = pack_bf2(o[dt][0] * inv, o[dt][1] * inv);
                p.y = pack_bf2(o[dt][2] * inv, o[dt][3] * inv);
                *(uint2*)(orow + dt * 16 + fq * 4) = p;
            }
        }
        qf[0] = qn[0];
        qf[1] = qn[1];
    }
}

struct KvPlan { int NT, NW, chunk, nchunks, grid, block, lds; };

int att_kv_plan(int B, int Lq, int Lk, int H, KvPlan* p) {
    if (B < 1 || Lq < 1 || Lk < 1 || H < 1 || Lk > 336) return USPACE_ERR_ARG;
    if ((long)B * H > (1L << 24) || Lq > (1 << 27)) return USPACE_ERR_ARG;
    const int nt = us_cdiv(Lk, 16);
    const int NT = nt <= 6 ? 6 : nt <= 10 ? 10 : nt <= 17 ? 17 : 21;     // the resident kernel's key-tile counts
    const int NW = NT > 17 ? 8 : 4;                                      // > 80 KB of LDS: one workgroup per CU, so 8 waves
    const long BH = (long)B * H;
    const int n_qt = us_cdiv(Lq, 16);
    // workgroups a full machine holds at once: 256 CUs x (two 4-wave workgroups | one 8-wave workgroup)
    const long slots = NW == 4 ? 512 : 256;
    const long per_head = (slots + BH - 1) / BH;                         // chunks per head that fill them (>= 1)
    int chunk = (int)((n_qt + per_head - 1) / per_head);
    if (chunk < NW) chunk = NW;                                          // at least one query tile per wave behind one staging
    chunk = us_cdiv(chunk, NW) * NW;                                     // whole rounds of the workgroup's waves
    const int nchunks = us_cdiv(n_qt, chunk);
    const long grid = BH * nchunks;
    if (grid >= (1L << 31)) return USPACE_ERR_ARG;
    *p = KvPlan{NT, NW, chunk, nchunks, (int)grid, 64 * NW, kv_lds_bytes(NT)};
    return USPACE_OK;
}

struct KvArgs { const bf16_t* q; int ldq; const bf16_t* kv; int ldkv; bf16_t* out; int ldo; int B, Lq, Lk, H; hipStream_t s; };

template <int NT, int NW>
int att_kv_launch(const KvPlan& p, const KvArgs& a) {
    static std::atomic<uint64_t> opted_in{0};
    const auto kernel = attention_kv_kernel<NT, NW>;
    US_TRY(us_opt_in_lds((const void*)kernel, 160 * 1024, opted_in));
    hipLaunchKernelGGL(kernel, dim3(p.grid), dim3(p.block), p.lds, a.s, a.q, a.ldq, a.kv, a.ldkv, a.out, a.ldo, a.Lq, a.Lk, a.H, p.chunk,
                       p.nchunks);
    US_CHECK_LAUNCH();
    return USPACE_OK;
}

}  // namespace

extern "C" int uspace_attention_kv_plan(int B, int Lq, int Lk, int H, int* out) {
    KvPlan p;
    if (!out) return USPACE_ERR_ARG;
    US_TRY(att_kv_plan(B, Lq, Lk, H, &p));
    const int v[7] = {p.NT, p.NW, p.chunk, p.nchunks, p.grid, p.block, p.lds};
    std::copy(v, v + 7, out);
    return USPACE_OK;
}

extern "C" int uspace_attention_kv_bf16(const uint16_t* q, int ldq, const uint16_t* kv, int ldkv, uint16_t* out, int ldo, int B, int Lq,
                                        int Lk, int H, uspace_stream_t stream) {
    KvPlan p;
    if (!q || !kv || !out) return USPACE_ERR_ARG;
    US_TRY(att_kv_plan(B, Lq, Lk, H, &p));
    // rows are read 16 bytes and written 8 bytes at a time
    if (ldq < H * DH || ldo < H * DH || ldkv < 2 * H * DH || ldq % 8 || ldkv % 8 || ldo % 4) return USPACE_ERR_ARG;
    if (((uintptr_t)q & 15) || ((uintptr_t)kv & 15) || ((uintptr_t)out & 7)) return USPACE_ERR_ARG;
    const KvArgs a{q, ldq, kv, ldkv, out, ldo, B, Lq, Lk, H, (hipStream_t)stream};
    if (p.NT == 6) return att_kv_launch<6, 4>(p, a);
    if (p.NT == 10) return att_kv_launch<10, 4>(p, a);
    if (p.NT == 17) return att_kv_launch<17, 4>(p, a);
    return att_kv_launch<21, 8>(p, a);
}
