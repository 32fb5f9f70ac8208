// Non-causal multi-head attention for sequences of any length (the 1 025 / 1 102 tokens of a U-ViT on 64 x 64 latents), head_dim 64,
// bf16 operands on the gfx950 matrix cores, fp32 online softmax.  The long form of attention.hip, which keeps a whole head's K and V
// in LDS and therefore stops at 336 tokens; the LDS image, its staging and the operand reads are that kernel's (attention_tiles.h).
//
// One workgroup (4 waves) owns QB = 64 or 128 consecutive queries of one (batch, head): a wave holds QT = 1 or 2 16-query tiles -- Q
// fragment, running maximum m, O^T accumulator and row sum -- in registers for the whole kernel.  K and V stream through two LDS
// buffers of KT = 64 keys each (2 x 16 KiB): while the waves compute on key tile j the LDS-DMA of tile j + 1 is in flight; one
// barrier per key tile.  Per key tile and query tile, in the resident kernel's operand layouts:
//   S^T = K . Q^T          -> a lane holds, for ONE query (lane & 15), 4 consecutive keys of each of the 4 16-key tiles
//   m'  = max(m, max S);  alpha = 2^((m - m') c);  O, sum *= alpha      (c = 64^-1/2 log2 e; first tile: m = -inf, alpha = 0)
//   P   = 2^(S c - m' c), rounded to bf16 ONCE: the same rounded P feeds P.V and, against an all-ones tile, the row sum
//   O^T += V^T . P^T      (V^T fragments by ds_read_b64_tr_b16; they and the K fragments are read once per key tile for all QT query tiles)
// and O / sum once at the end.  Keys >= L exist only in the last key tile and are masked to -inf before they enter the maximum; every
// key tile holds at least one real key, so m' is finite from the first tile on and no (-inf) - (-inf) occurs.  The LDS rows behind L
// repeat row L - 1 (finite), their P is 0.
// key_scale[B, L] multiplies P column-wise after normalisation: bf16(P ks) feeds P.V, bf16(P) the row sum, as in the resident kernel.
// A query row is never split: one wave walks all of its keys in order, no atomics, and the arithmetic of a row is the same for QT = 1
// and 2 -- a row's bits depend on neither B, H, the grid nor the plan's branch.
#include "attention_tiles.h"

namespace {

constexpr int LKT = 64;                          // keys per key tile
constexpr int LNW = 4;                           // waves per workgroup
constexpr int LTILE_BYTES = LKT * KROW_BYTES;    // one K or V buffer
// dynamic LDS: K[2][64 rows], V[2][64 rows], then one fp32 key scale per K row of both buffers (SCALED only)
constexpr int long_lds_bytes(bool scaled) { return 4 * LTILE_BYTES + (scaled ? 2 * LKT * 4 : 0); }

template <bool SCALED, int QT>
__global__ __launch_bounds__(64 * LNW, 2) void attn_stream_kernel(const bf16_t* __restrict__ qkv, const float* __restrict__ key_scale,
                                                                  bf16_t* __restrict__ out, int L, int H, int nqb) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* sK = smem;                                   // [2][LKT][64] bf16, 16-B chunks swizzled (k_off)
    char* sV = smem + 2 * LTILE_BYTES;                 // [2][LKT][64] bf16, 32-B chunks swizzled (v_off)
    float* sKs = (float*)(smem + 4 * LTILE_BYTES);     // [2][LKT] key scale (SCALED only)

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int bh = blockIdx.x / nqb, qb = blockIdx.x % nqb;
    const int b = bh / H, h = bh % H;
    const int C3 = 3 * H * DH;
    const bf16_t* base = qkv + (size_t)b * L * C3;
    const bf16_t* gq = base + h * DH;
    const bf16_t* gk = base + (H + h) * DH;
    const bf16_t* gv = base + (2 * H + h) * DH;
    const float* gks = SCALED ? key_scale + (size_t)b * L : nullptr;

    const int fr = lane & 15;
    const int fq = lane >> 4;
    const float c_exp = 0.125f * 1.4426950408889634f;  // head_dim^-0.5 * log2(e)
    const int nkt = (L + LKT - 1) / LKT;

    // this wave's query tiles (rows >= L read row L - 1 again and are not stored)
    const int q_first = ((qb * LNW + wave) * QT) * 16;
    bf16x8 qf[QT][2];
#pragma unroll
    for (int i = 0; i < QT; ++i) {
        int qrow = q_first + i * 16 + fr;
        qrow = qrow < L ? qrow : L - 1;
        qf[i][0] = *(const bf16x8*)(gq + (size_t)qrow * C3 + fq * 8);
        qf[i][1] = *(const bf16x8*)(gq + (size_t)qrow * C3 + 32 + fq * 8);
    }
    float m[QT];
    f32x4 o[QT][4], osum[QT];
#pragma unroll
    for (int i = 0; i < QT; ++i) {
        m[i] = -INFINITY;
        osum[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o[i][dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    union { uint32_t w[4]; bf16x8 v; } ones;
    ones.w[0] = ones.w[1] = ones.w[2] = ones.w[3] = 0x3f803f80u;

    // key tile j -> buffer j & 1: 8 blocks of 8 rows of K and of V, two of each per wave
    auto stage = [&](int j) {
        const int buf = j & 1, key0 = j * LKT;
#pragma unroll
        for (int blk = 0; blk < LKT / 8 / LNW; ++blk) {
            const int rb = (blk * LNW + wave) * 8;
            att_dma_k8(gk, C3, key0 + rb, L, sK + buf * LTILE_BYTES + rb * KROW_BYTES, lane);
            att_dma_v8(gv, C3, key0 + rb, L, sV + buf * LTILE_BYTES + rb * KROW_BYTES, lane);
        }
    };
    auto load_ks = [&](int j) {                        // the tile's key scale of this thread (tid < LKT), 0 behind L
        const int k = j * LKT + tid;
        return (tid < LKT && k < L) ? gks[k] : 0.f;
    };
    stage(0);
    if constexpr (SCALED) {
        if (tid < LKT) sKs[tid] = load_ks(0);
    }

#pragma unroll 1
    for (int j = 0; j < nkt; ++j) {
        // This wave's share of tile j has landed -- waited for explicitly: the backend places its own wait for an LDS-DMA in front of the
        // wave's next LDS read, which is BEHIND the barrier, where the other waves' shares are read as well -- and every wave is done with
        // tile j - 1, whose buffer tile j + 1 now overwrites.
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        const bool more = j + 1 < nkt;                 // workgroup-uniform
        const char* kb = sK + (j & 1) * LTILE_BYTES;
        const char* vb = sV + (j & 1) * LTILE_BYTES;
        const bool last = !more;

        // K and V^T fragments (and key scales) of the key tile, shared by the wave's query tiles.  Every LDS read of the tile is up here, in
        // front of the next tile's LDS-DMA: the backend cannot tell the two buffers apart and makes an LDS read behind an LDS-DMA wait for it.
        bf16x8 kf[4][2];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            kf[t][0] = *(const bf16x8*)(kb + k_off(t * 16 + fr, fq));
            kf[t][1] = *(const bf16x8*)(kb + k_off(t * 16 + fr, 4 + fq));
        }
        union VF { uint2 h[2]; bf16x8 v; };
        VF vf[2][4];
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) att_read_vt(vb, fq, fr, dt, u * (32 * KROW_BYTES), vf[u][dt].h[0], vf[u][dt].h[1]);
        f32x4 ksv[SCALED ? 4 : 1];
        if constexpr (SCALED) {
#pragma unroll
            for (int t = 0; t < 4; ++t) ksv[t] = *(const f32x4*)(sKs + (j & 1) * LKT + t * 16 + fq * 4);
        }
        float ks_next = 0.f;
        if (more) {
            stage(j + 1);
            if constexpr (SCALED) ks_next = load_ks(j + 1);
        }

#pragma unroll
        for (int i = 0; i < QT; ++i) {
            // ---- S^T tiles: s[t][r] = <K[key0 + t*16 + 4*fq + r], Q[q + fr]>
            f32x4 s[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) s[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int t = 0; t < 4; ++t) s[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[t][ks], qf[i][ks], s[t], 0, 0, 0);
            // ---- mask: only the last key tile holds keys >= L
            if (last) {
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) s[t][r] = (j * LKT + t * 16 + fq * 4 + r) < L ? s[t][r] : -INFINITY;
            }
            // ---- running row maximum; the accumulated O and sum follow it
            float mx = fmaxf(fmaxf(s[0][0], s[0][1]), fmaxf(s[0][2], s[0][3]));
#pragma unroll
            for (int t = 1; t < 4; ++t) mx = fmaxf(mx, fmaxf(fmaxf(s[t][0], s[t][1]), fmaxf(s[t][2], s[t][3])));
            mx = att_max_over_rows(mx);
            const float m_new = fmaxf(m[i], mx);
            const float alpha = __builtin_amdgcn_exp2f((m[i] - m_new) * c_exp);
            m[i] = m_new;
            const float mc = m_new * c_exp;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) o[i][dt] *= alpha;
            osum[i] *= alpha;
            // ---- P = 2^(s*c - m*c), rounded to bf16 once: pu feeds the row sum, pb (= pu without key scales) P.V
            union PF { uint32_t w[4]; bf16x8 v; };
            PF pu[2], pb[2];
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) s[t][r] = __builtin_amdgcn_exp2f(fmaf(s[t][r], c_exp, -mc));
            auto pack_p = [&](PF (&pf)[2]) {
#pragma unroll
                for (int u = 0; u < 2; ++u) {           // k-slot (fq, e) of step u: e < 4 -> tile 2u key 4fq + e, e >= 4 -> tile 2u + 1
                    pf[u].w[0] = pack_bf2(s[2 * u][0], s[2 * u][1]);
                    pf[u].w[1] = pack_bf2(s[2 * u][2], s[2 * u][3]);
                    pf[u].w[2] = pack_bf2(s[2 * u + 1][0], s[2 * u + 1][1]);
                    pf[u].w[3] = pack_bf2(s[2 * u + 1][2], s[2 * u + 1][3]);
                }
            };
            pack_p(pu);
            if constexpr (SCALED) {
#pragma unroll
                for (int t = 0; t < 4; ++t) s[t] *= ksv[t];
                pack_p(pb);
            }
            // ---- O^T += V^T . P^T, sum += 1 . P^T
#pragma unroll
            for (int u = 0; u < 2; ++u) {
#pragma unroll
                for (int dt = 0; dt < 4; ++dt)
                    o[i][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf[u][dt].v, SCALED ? pb[u].v : pu[u].v, o[i][dt], 0, 0, 0);
                osum[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones.v, pu[u].v, osum[i], 0, 0, 0);
            }
        }
        if constexpr (SCALED) {
            // (written here, not next to its load: a wait for that load in front of the tile's compute would also wait for the LDS-DMA issued before it)
            if (more && tid < LKT) sKs[((j + 1) & 1) * LKT + tid] = ks_next;
        }
    }

    // ---- store: lane holds query q + fr, head dims dt*16 + 4*fq + {0..3}
#pragma unroll
    for (int i = 0; i < QT; ++i) {
        const int q = q_first + i * 16 + fr;
        if (q < L) {
            const float inv = 1.0f / osum[i][0];
            bf16_t* orow = out + ((size_t)b * L + q) * (H * DH) + h * DH;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                uint2 p;
                p.x = pack_bf2(o[i][dt][0] * inv, o[i][dt][1] * inv);
                p.y = pack_bf2(o[i][dt][2] * inv, o[i][dt][3] * inv);
                *(uint2*)(orow + dt * 16 + fq * 4) = p;
            }
        }
    }
}

// ---- host side.  long_plan alone decides what a call launches, long_launch alone launches; uspace_attention_long_plan reports the plan.
struct LongPlan { int KT, QB, NW, nqb, grid, block, lds; };     // nqb: workgroups per (batch, head) = ceil(L / QB)
struct LongArgs { const bf16_t* qkv; const float* ks; bf16_t* out; int B, L, H; hipStream_t s; };

int long_plan(int B, int L, int H, bool scaled, LongPlan* p) {
    if (B <= 0 || L <= 0 || H <= 0) return USPACE_ERR_ARG;
    // rows (B * L) and columns (3 * H * 64) are ints in the kernel, B * H and the grid as well; element offsets are size_t
    const long long maxi = 0x7fffffffLL;
    if ((long long)B * L > maxi || (long long)H * (3 * DH) > maxi || (long long)B * H > maxi) return USPACE_ERR_ARG;
    const long long BH = (long long)B * H;
    // 128 queries per workgroup (two query tiles per wave share every K / V fragment read) once that still gives every CU its two
    // resident workgroups (256 CUs); below that 64, which splits a head along its queries only.  (The switch point is reasoned, not
    // measured: DESIGN.md section 4.2a.)
    const int QB = BH * us_cdiv(L, 128) >= 512 ? 128 : 64;
    const int nqb = us_cdiv(L, QB);
    const long long grid = BH * nqb;
    if (grid > maxi) return USPACE_ERR_ARG;
    *p = LongPlan{LKT, QB, LNW, nqb, (int)grid, 64 * LNW, long_lds_bytes(scaled)};
    return USPACE_OK;
}

// The launch recorder sees the long form as an attention launch with US_REC_ATT_LONG in its flags.
template <bool SCALED, int QT>
int long_launch(const LongPlan& p, const LongArgs& a) {
    const auto kernel = attn_stream_kernel<SCALED, QT>;     // 32.5 KiB of dynamic LDS: no large-LDS opt-in to make
    const int rec = us_rec_begin(US_REC_ATTENTION, US_REC_ATT_LONG | (SCALED ? US_REC_ATT_SCALED : 0), a.B * a.H, a.L, 64, a.s);
    hipLaunchKernelGGL(kernel, dim3(p.grid), dim3(p.block), p.lds, a.s, a.qkv, a.ks, a.out, a.L, a.H, p.nqb);
    us_rec_end(rec, a.s);
    US_CHECK_LAUNCH();
    return USPACE_OK;
}

}  // namespace

extern "C" int uspace_attention_long_plan(int B, int L, int H, int scaled, int* out) {
    LongPlan p;
    if (!out) return USPACE_ERR_ARG;
    US_TRY(long_plan(B, L, H, scaled != 0, &p));
    const int v[6] = {p.KT, p.QB, p.NW, p.grid, p.block, p.lds};
    std::copy(v, v + 6, out);
    return USPACE_OK;
}

extern "C" int uspace_attention_long_bf16(const uint16_t* qkv, const float* key_scale, uint16_t* out, int B, int L, int H,
                                          uspace_stream_t stream) {
    LongPlan p;
    if (!qkv || !out) return USPACE_ERR_ARG;
    US_TRY(long_plan(B, L, H, key_scale != nullptr, &p));
    const LongArgs a{qkv, key_scale, out, B, L, H, (hipStream_t)stream};
    if (key_scale) return p.QB == 128 ? long_launch<true, 2>(p, a) : long_launch<true, 1>(p, a);
    return p.QB == 128 ? long_launch<false, 2>(p, a) : long_launch<false, 1>(p, a);
}

// The attention of a block: the resident kernel wherever its plan takes the length (att_plan of attention.hip is the one place that
// knows the limit), the streaming kernel beyond
int us_attention_any(const uint16_t* qkv, const float* key_scale, uint16_t* out, int B, int L, int H, uspace_stream_t stream) {
    int plan[8];
    if (uspace_attention_plan(B, L, H, key_scale != nullptr, plan) == USPACE_OK)
        return uspace_attention_bf16(qkv, key_scale, out, B, L, H, stream);
    return uspace_attention_long_bf16(qkv, key_scale, out, B, L, H, stream);
}
