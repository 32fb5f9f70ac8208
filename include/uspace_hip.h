/*
 * uspace_hip.h -- C-ABI of the MI355X (gfx950) implementation of uspace's flow-matching
 * sampling hot path: the U-ViT velocity-network forward evaluated at every ODE step.
 *
 * The reference (dongzhuoyao/uspace, paths below relative to its root) is pure Python and
 * has no FFI of its own; this header is the boundary a maintainer binds instead of the
 * stock PyTorch ops the reference calls (INTEGRATION.md shows the ctypes stub).  Rules:
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless it says host;
 *   - the caller owns every buffer (weights blob, workspace, inputs, outputs);
 *   - every function enqueues on the caller's hipStream_t and never synchronises;
 *   - return 0 on success, a negative USPACE_ERR_* otherwise; nothing throws;
 *   - no per-call global state.  Process-wide state, all of it listed here: (1) the optional launch recorder at the
 *     end of this header (not thread-safe: one measuring thread); (2) the LayerNorm-fold switch
 *     uspace_uvit_set_ln_fold / _get_ln_fold (atomic; default on); (3) per kernel, the set of devices on which it has
 *     been opted in to more than 64 KiB of dynamic LDS (atomic bit mask; any number of GPUs per process); (4) a
 *     mutex-protected cache of the parameter layout derived from each distinct uspace_uvit_config; (5) the switch of the GEMM's
 *     in-launch K-split tail uspace_gemm_set_sk / _get_sk (atomic; default on; read once per call: uspace_uvit_forward reads it once
 *     for its workspace, its partial-sum slot counts and all of its launches); (6) per device, whether it has the 256 CUs that form needs.
 * bf16 values cross the boundary as raw uint16_t (upper half of an IEEE fp32, RNE).
 */
#ifndef USPACE_HIP_H
#define USPACE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define USPACE_ABI_VERSION 11

#define USPACE_OK 0
#define USPACE_ERR_ARG (-1)         /* bad pointer / size / unsupported shape */
#define USPACE_ERR_LAUNCH (-2)      /* hipGetLastError() != hipSuccess after a launch */
#define USPACE_ERR_WORKSPACE (-3)   /* workspace too small */

typedef void* uspace_stream_t;      /* a hipStream_t */

#define USPACE_API __attribute__((visibility("default")))

USPACE_API int uspace_abi_version(void);

/* ---------------------------------------------------------------------------------------
 * Operators.  Each replaces one stock op of the reference's nnet forward.
 * ------------------------------------------------------------------------------------- */

/* Epilogue flags for uspace_gemm_bf16 (OR them). */
#define USPACE_EPI_BIAS 1        /* + bias[N]                                   */
#define USPACE_EPI_GELU 2        /* exact-erf GELU after bias (libs/timm.py:107) */
#define USPACE_EPI_RESIDUAL 4    /* + resid_in[M,N] (fp32)                      */
#define USPACE_EPI_OUT_F32 8     /* write out_f32[M,N]                          */
#define USPACE_EPI_OUT_BF16 16   /* write out_bf16[M,N]                         */
#define USPACE_EPI_CEN_OUT 32    /* uspace_gemm_bf16_ext: also write bf16(v - row_c[m]) and per-row partial sums */
#define USPACE_EPI_LN_IN 64      /* uspace_gemm_bf16_ext: A holds centred rows; apply LayerNorm through the GEMM  */
#define USPACE_EPI_RANK1 128     /* uspace_gemm_bf16_ext, with CEN_OUT: + row_add[m] * col_add[n] (a K slab that was stored centred) */

/* nn.Linear on bf16 operands with fp32 accumulation on the MFMA cores:
 *     acc[M,N] = [A | A2][M,K] . W[N,K]^T
 * A is [M,K1] (row stride lda), A2 (optional, NULL when K1 == K) is [M,K1] with K == 2*K1, K1 a power
 * of two (row stride lda2, which must equal lda): the two K-slabs of skip_linear(cat([x, skip])) without materialising
 * the concat (libs/uvit.py:159).  W is nn.Linear's own [out,in] layout (row stride ldw).
 * K1 and K must be multiples of 64, N a multiple of 4.  resid_in and out_f32 may alias
 * (x += ...; libs/uvit.py:160-161).  Replaces libs/uvit.py:89,116,159; libs/timm.py:107-110;
 * libs/uvit_t2i.py:322. */
USPACE_API int uspace_gemm_bf16(const uint16_t* A, int lda, const uint16_t* A2, int lda2, int K1,
                     const uint16_t* W, int ldw, int M, int N, int K, int epi_flags,
                     const float* bias, const float* resid_in, int ld_resid,
                     float* out_f32, int ld_f32, uint16_t* out_bf16, int ld_bf16,
                     uspace_stream_t stream);

/* LayerNorm folded through the GEMMs that surround it (no separate LayerNorm pass over the residual stream).
 *   y = LN(x) W^T + b = rstd * ((x - mu) . (W gamma)^T) + (b + W beta)
 * Producer of x (proj / fc2 / skip_linear, USPACE_EPI_CEN_OUT): besides its usual outputs writes out_cen[m, n] =
 *   bf16(v[m, n] - row_c[m]) -- row_c is any per-row constant close to the row mean, so the rounding acts on centred
 *   values exactly as it does on LayerNorm's output today -- and part_out[m][tile][2] = (sum, sum of squares) of
 *   v - row_c over each N tile (uspace_gemm_part_slots_k(M, N, K) tiles per row; fixed summation order, no atomics).
 * Consumer (qkv / fc1, USPACE_EPI_LN_IN): A = out_cen, W = bf16(W * gamma), bias = b + W beta, colsum[n] = sum_k of the
 *   bf16 W rows; from part_in it derives d = mean(v - row_c), rstd = 1/sqrt(var + eps) (norm_dim = row length) and
 *   applies y = rstd * (acc - d * colsum) + bias before the rest of the epilogue; with c_out it also publishes
 *   c_out[m] = row_c[m] + d (the row mean) for the next producer. */
typedef struct uspace_gemm_ext {
    const float* row_c;     /* [M]   CEN_OUT: centring constants; LN_IN: the ones its producer used (only with c_out) */
    uint16_t* out_cen;      /* [M, ld_cen] bf16 */
    int ld_cen;
    float* part_out;        /* [M][uspace_gemm_part_slots_k(M, N, K)][2] */
    const float* part_in;   /* [M][np_in][2] */
    int np_in;              /* <= 8 */
    const float* colsum;    /* [N] */
    float* c_out;           /* [M] or NULL */
    int norm_dim;           /* LayerNorm width (row length of the producer's output) */
    float eps;
    /* USPACE_EPI_RANK1: acc[m, n] += row_add[m] * col_add[n] ahead of the bias.  skip_linear(cat([x, skip])) with the skip kept as
     * the CENTRED bf16 copy its producer wrote anyway (skip = xc + c):  xc . W2^T + c[m] * rowsum(W2)[n]  -- row_add = the centring
     * constants of that copy, col_add[n] = sum_k bf16(W[n, K1 + k]) (libs/uvit.py:158-159). */
    const float* row_add;   /* [M] */
    const float* col_add;   /* [N] */
    /* optional (any epilogue without LN_IN / GELU): workspace for the K-split form of small launches -- few output tiles and
     * a long K are cut into K ranges on as many times the CUs, whose fp32 partial sums go here; a second kernel adds them in
     * a fixed order and applies the epilogue.  uspace_gemm_split_ws_bytes(M, N, K) is the size it needs (0: the launch is
     * never split); NULL or too small = no split.  Must not alias any operand; 16-byte aligned; one workspace serves one
     * stream at a time. */
    void* split_ws;
    size_t split_ws_bytes;
    /* optional (round 6, ABI 11): workspace for the K-split TAIL of launches whose 256x256 tiles do not fill whole rounds of the 256
     * CUs (proj / fc2 / skip_linear / qkv epilogues; e.g. M = 64 x 334 or 32 x 257 rows at N = 1024).  The whole rounds run as they are;
     * every remaining tile is shared by 2 ... 4 workgroups of the SAME launch, each over a part of the K tiles, which exchange fp32
     * partial sums through sk_ws and finish a part of the tile's rows each (fixed summation order: bit-identical run to run, no second
     * kernel).  uspace_gemm_sk_ws_bytes(M, N, K) is the size it needs (0: the launch has no such tail).  sk_counters: 256 uint32,
     * ALL ZERO when the launch starts (the kernel leaves counts behind: zero them again before the next use, or hand every launch its
     * own 256).  Both NULL, or sk_ws too small: no tail (a producer of LayerNorm partial sums then takes plain 256x256 tiles).
     * 16-byte aligned, must not alias any operand, one workspace serves one stream at a time. */
    void* sk_ws;
    size_t sk_ws_bytes;
    void* sk_counters;
} uspace_gemm_ext;
USPACE_API size_t uspace_gemm_split_ws_bytes(int M, int N, int K);
USPACE_API size_t uspace_gemm_sk_ws_bytes(int M, int N, int K);
#define USPACE_GEMM_SK_COUNTERS 256
/* process-wide switch of that form (A/B measurements): 1 = launches may take it (default), 0 = never, -1 = back to the default.
 * uspace_gemm_plan_k / _part_slots_k / _sk_ws_bytes answer for the current setting; set it before sizing workspaces. */
USPACE_API int uspace_gemm_set_sk(int mode);
USPACE_API int uspace_gemm_get_sk(void);
USPACE_API int uspace_gemm_bf16_ext(const uint16_t* A, int lda, const uint16_t* A2, int lda2, int K1,
                                    const uint16_t* W, int ldw, int M, int N, int K, int epi_flags,
                                    const float* bias, const float* resid_in, int ld_resid,
                                    float* out_f32, int ld_f32, uint16_t* out_bf16, int ld_bf16,
                                    const uspace_gemm_ext* ext, uspace_stream_t stream);
/* pack-time fold for a LayerNorm consumer: Wf = bf16(W * gamma) [N, K], colsum[n] = sum_k Wf[n, k],
 * bias_out[n] = (bias ? bias[n] : 0) + sum_k W[n, k] * beta[k] */
USPACE_API int uspace_fold_layernorm(const float* W, const float* gamma, const float* beta, const float* bias, uint16_t* Wf,
                                     float* bias_out, float* colsum, int N, int K, uspace_stream_t stream);
/* first norm of a chain: xc = bf16(x - rowmean), c[m] = rowmean, part[m][1][2] = (sum, sum of squares) of x - rowmean */
USPACE_API int uspace_center_rows(const float* x, uint16_t* xc, float* c, float* part, int M, int D, uspace_stream_t stream);
/* process-wide switch for the U-ViT forward: 1 = LayerNorm folded through the GEMMs (default), 0 = separate LayerNorm
 * launches (kept for A/B measurements), -1 = back to the default.  The library reads no environment variable.
 * A hipGraph captured by uspace_uvit_graph_create keeps the mode it was captured in. */
USPACE_API int uspace_uvit_set_ln_fold(int mode);
USPACE_API int uspace_uvit_get_ln_fold(void);
/* number of N tiles (= partial-sum slots per row) a CEN_OUT launch with this [M, N] output uses */
USPACE_API int uspace_gemm_part_slots(int M, int N);       /* the largest count over K: size part_out / check np_in <= 8 with it */
/* ... of the producer GEMM with this K.  (Launches of few tiles use 64-wide tiles -- more slots -- whatever their K; K only
 * selects which K loop those tiles run, so today the count does not depend on it.  Callers pass the real K all the same.) */
USPACE_API int uspace_gemm_part_slots_k(int M, int N, int K);

/* Which tile configuration uspace_gemm_bf16 uses for an [M, N] output (host-side planning, no GPU work):
 * 0 = 256x256 tiles, 1 = 192x256, 2 = 128x128, 3 = rows [0, *split_rows) as 256x256 and the rest as 128x128,
 * 4 = 256x128 (short row counts / narrow outputs: twice the workgroups of 256x256 at 3/4 of its staging traffic). */
USPACE_API int uspace_gemm_tile_choice(int M, int N, int* split_rows);
/* The whole plan (host-side, no GPU work): out[8] = {choice as above, split_rows, BM, BN, tile rows, tile columns, number of
 * 16-row remainder strips (each owned by the workgroups of one tile row), workgroups per round of 256 CUs}.  For choice 3 the
 * fields after split_rows describe the 256x256 launch over rows [0, split_rows). */
USPACE_API int uspace_gemm_plan(int M, int N, int* out);
/* ... of a launch with this K and role (producer of LayerNorm partial sums or not), i.e. what the dispatcher really launches:
 * few-tile launches use 64x64 tiles (out[0] = 5, out[2] = out[3] = 64; K selects their K loop and with it out[7]: 512 workgroups
 * per round for the four-stage ring, 1024 for the two-stage form); a producer never takes the split form (reported as 256x256) nor
 * 128-wide tiles that would make more than 8 partial-sum slots (reported as 256x256).  The answer assumes a launch that may take
 * the K-split tail; a uspace_gemm_slabs_bf16 launch of more than 2 slabs never does (3x3 convolutions: 9): for it, ask with
 * uspace_gemm_set_sk(0). */
USPACE_API int uspace_gemm_plan_k(int M, int N, int K, int producer, int* out);

/* Sum of row-shifted GEMMs:  acc[m, n] = sum_t A[m + row_shift[t], 0:K1] . W[n, t*K1:(t+1)*K1]  (+ epilogue
 * as above).  With rows = pixels of a zero-bordered NHWC map [B, H+2, W+2, C] and the 9 shifts
 * dy*(W+2)+dx this is Conv2d(C, N, 3, padding=1) (libs/autoencoder.py:85-112); the caller provides
 * (W+3) guard rows before and after the map (border outputs are garbage and must be re-zeroed by the
 * consumer).  K1 a power of two >= 64, n_slab <= 9, W rows are [tap][K1] contiguous.  row_shift is a HOST
 * array. */
USPACE_API int uspace_gemm_slabs_bf16(const uint16_t* A, int lda, const uint16_t* W, int ldw, int M, int N, int K1,
                                      int n_slab, const int* row_shift, int epi_flags, const float* bias,
                                      const float* resid_in, int ld_resid, float* out_f32, int ld_f32,
                                      uint16_t* out_bf16, int ld_bf16, uspace_stream_t stream);

/* nn.LayerNorm(D, eps) over fp32 rows -> bf16 rows (libs/uvit.py:135,139,160-161). D % 4 == 0. */
USPACE_API int uspace_layernorm_f32_bf16(const float* x, const float* gamma, const float* beta, uint16_t* y,
                              int M, int D, float eps, uspace_stream_t stream);

/* Non-causal multi-head attention, head_dim 64, softmax in fp32 (libs/uvit.py:91-96).
 * qkv [B*L, 3*H*64] bf16 with columns ordered (3, H, 64); out [B*L, H*64] bf16.
 * key_scale (optional, [B, L] fp32): the post-softmax map is multiplied column-wise by it
 * before P.V, without renormalisation -- the attention-map edit of
 * tools/utils_t2i.py:196-224 at libs/uvit_t2i.py:101-105, applied as a row scaling of V.
 * L <= 336 (K and V of a head resident in LDS; longer sequences: uspace_attention_long_bf16); which kernel form and grid a call
 * launches: uspace_attention_plan. */
USPACE_API int uspace_attention_bf16(const uint16_t* qkv, const float* key_scale, uint16_t* out,
                          int B, int L, int H, uspace_stream_t stream);
/* host-side, no GPU work: out[8] = {NT, LC, NW, QS, HPW, grid, block, dynamic LDS bytes} of the launch
 * uspace_attention_bf16 takes for (B, L, H, key_scale != NULL); USPACE_ERR_ARG where that call would refuse (L > 336 among them:
 * uspace_attention_long_plan).
 * NT 16-key tiles the kernel is compiled for, LC its compile-time length (0 = any length up to 16 NT), NW waves per workgroup,
 * QS workgroups per (batch, head), HPW heads per workgroup. */
USPACE_API int uspace_attention_plan(int B, int L, int H, int scaled, int* out);

/* The long form of uspace_attention_bf16: same qkv, key_scale and out, same key_scale semantics (bf16(P ks) feeds P.V, bf16(P) the
 * row sum, no renormalisation; a sample whose scales are all 0 comes out exactly 0), any L >= 1.  K and V stream through LDS in key
 * tiles under an fp32 online softmax (running row maximum and sum; P rounded to bf16 once per key tile).  A query row's keys are never
 * split across workgroups and there are no atomics: a row's bits depend on neither B, H nor the grid, and repeat from run to run.
 * The U-ViT forward takes it for L > 336.  USPACE_ERR_ARG for B, L or H <= 0, NULL qkv / out, or B * L, 3 * H * 64, B * H or the
 * grid beyond INT_MAX. */
USPACE_API int uspace_attention_long_bf16(const uint16_t* qkv, const float* key_scale, uint16_t* out,
                                          int B, int L, int H, uspace_stream_t stream);
/* host-side, no GPU work: out[6] = {KT, QB, NW, grid, block, dynamic LDS bytes} of the launch uspace_attention_long_bf16 takes for
 * (B, L, H, key_scale != NULL); USPACE_ERR_ARG where that call would refuse.  KT keys per key tile, QB queries per workgroup
 * (grid = B * H * ceil(L / QB)), NW waves per workgroup. */
USPACE_API int uspace_attention_long_plan(int B, int L, int H, int scaled, int* out);

/* Single-head, non-causal attention with a wide head (the VAE's mid-block AttnBlock beyond 1 024 tokens):
 *   out[b, i, :] = softmax_j(q[b, i] . k[b, j] * scale) . v[b, j, :]
 * q, k, v: token-major bf16 [B * N, C] with leading dimension ld (elements; a multiple of 8, 16-byte aligned pointers); out bf16
 * [B * N, C] with leading dimension ld_out (a multiple of 4, 8-byte aligned).  C = 64, 128, 256 or 512; any N >= 1.  K and V stream
 * through LDS in 32-key tiles; online softmax in fp32 (running maximum and sum, accumulator rescaling), P rounded to bf16 once per
 * key tile for both P.V and the row sum, one division at the end, keys >= N masked before the maximum.  A query row is never split
 * across workgroups and there are no atomics: a row's bits depend on neither B nor the grid, and repeat from run to run.  Nothing is
 * read before it is written.  USPACE_ERR_ARG for any other C, B or N <= 0, NULL or misaligned operands, ld or ld_out < C, a scale
 * that is not positive and finite, or B * N or the grid beyond INT_MAX.  Added without a change of USPACE_ABI_VERSION: symbols only. */
USPACE_API int uspace_attention_wide_bf16(const uint16_t* q, const uint16_t* k, const uint16_t* v, int ld,
                                          uint16_t* out, int ld_out, int B, int N, int C, float scale,
                                          uspace_stream_t stream);
/* host-side, no GPU work: out[6] = {KT, QB, NW, grid, block, dynamic LDS bytes} of the launch uspace_attention_wide_bf16 takes for
 * (B, N, C); USPACE_ERR_ARG where that call would refuse these three.  KT keys per key tile, QB = 16 NW queries per workgroup
 * (grid = B * ceil(N / QB)), NW waves per workgroup. */
USPACE_API int uspace_attention_wide_plan(int B, int N, int C, int* out);

/* Head-mean attention map of the same packed qkv (what tools/utils_t2i.py:141-193 vis_attention_map draws from the reference's
 * [B, H, L, L] softmax, libs/uvit_t2i.py:101-103):
 *     out[b, i, j] = (1/H) * sum_h softmax_k( q[b,h,q0+i] . k[b,h,k] * 64^-0.5 )[k0+j]       fp32, [B, nq, nk]
 * The softmax runs over ALL L keys, not the window.  No key_scale: the reference shows the map before the edit
 * (tools/utils_t2i.py:283 precedes :286).  P stays fp32; the heads are summed in the order 0 .. H-1 by the one workgroup that owns
 * a (sample, 16-query tile): no atomics, bit-equal from run to run and for any B.  head_dim 64, L <= 336 (there is no long form of the
 * map), 0 <= q0, nq >= 1,
 * q0 + nq <= L and the same for k0 / nk; anything else returns USPACE_ERR_ARG. */
USPACE_API int uspace_attention_map_bf16(const uint16_t* qkv, float* out, int B, int L, int H,
                                         int q0, int nq, int k0, int nk, uspace_stream_t stream);

/* Token assembly (libs/uvit.py:315-327, libs/uvit_t2i.py:309-324): patch-embed conv (k=s=p) +
 * sinusoidal time token + optional extra tokens + pos_embed, fp32 -> residual stream
 * tok[B, L, D] fp32 (+ bf16 copy if tok_bf16 != NULL).
 *   img [B,C,S,S] fp32; t: B timesteps read as t[b*t_stride] (t_stride 0 for the solver's
 *   stride-0 expand, flow_matching.py:33); extra [B, n_extra, D] fp32 or NULL.
 *   time_first != 0: order [time, extra..., patches] (T2I); == 0: [extra..., time, patches]
 *   (class-conditional: label token precedes the time token, libs/uvit.py:322-326). */
USPACE_API int uspace_embed_tokens(const float* img, const float* t, int t_stride, const float* extra, int n_extra,
                        int time_first, const float* patch_w, const float* patch_b, const float* pos,
                        float* tok, uint16_t* tok_bf16, int B, int C, int S, int p, int D,
                        uspace_stream_t stream);

/* Output head (libs/uvit.py:342-347): LayerNorm -> decoder_pred (D -> p*p*C) on the patch
 * tokens -> unpatchify "(p1 p2 C)" -> Conv2d(C,C,3,pad=1).  tok [B,L,D] fp32, out [B,C,S,S]
 * fp32; scratch must hold B*C*S*S floats. */
USPACE_API int uspace_output_head(const float* tok, int L, int extras, const float* norm_g, const float* norm_b,
                       const float* dec_w, const float* dec_b, const float* conv_w, const float* conv_b,
                       float* scratch, float* out, int B, int C, int S, int p, int D, float eps,
                       uspace_stream_t stream);

/* x[b, i] += scale * delta[i]  (the u-space write hook, libs/dissection.py:157,178; delta is
 * broadcast over the batch).  Optionally refreshes a bf16 copy of x. */
USPACE_API int uspace_add_broadcast(float* x, uint16_t* x_bf16, const float* delta, float scale,
                         int B, long per_sample, uspace_stream_t stream);

/* Same with a per-sample factor: x[b, i] += scale * row_scale[b] * delta[i] (row_scale: device float[B] or
 * NULL).  Lets the reference's sweep over `write_scales` (tools/utils_vis.py:189-198: nine full solves of
 * the same z) run as ONE solve over 9*B rows. */
USPACE_API int uspace_add_broadcast_rows(float* x, uint16_t* x_bf16, const float* delta, float scale,
                                         const float* row_scale, int B, long per_sample, uspace_stream_t stream);

/* Classifier-free guidance, U-ViT's convention (the configs' sample.scale): out[b, i] = c + s_b * (c - u) with c = pair[b, i],
 * u = pair[B + b, i] and s_b = scale * row_scale[b] (row_scale: device float[B] or NULL = ones), evaluated in fp32 as
 * fmaf(s_b, c - u, c); s_b == 0 returns c bit for bit.  pair [2B, per_sample] holds the conditional rows first, out is
 * [B, per_sample] and overlaps neither half of pair.  16-byte accesses where per_sample % 4 == 0 and both pointers are 16-byte
 * aligned, a scalar form otherwise; no atomics. */
USPACE_API int uspace_cfg_combine(const float* pair, const float* row_scale, float scale, float* out, int B, long per_sample,
                                  uspace_stream_t stream);

/* Attribute-direction statistics kept on the device (reference: tools/utils_attr.py:124-145 computes
 * mean(feat[attr==1]) - mean(feat[attr==0]) in numpy from activations the read hook staged through disk):
 *   pos_sum[a, f] += sum_n [attr[n,a] == 1] * feat[n, f];  neg_sum likewise for attr == 0.
 * feat [B, F] fp32, attr [B, A] int32, pos_sum / neg_sum [A, F] fp32 (caller zero-initialises). F % 4 == 0. */
USPACE_API int uspace_direction_accumulate(const float* feat, const int* attr, float* pos_sum, float* neg_sum,
                                           int B, long F, int A, uspace_stream_t stream);

/* Principal directions of tapped activations (reference: tools/utils_pca.py:13-50 over sklearn PCA(svd_solver="full"),
 * tools/utils_vis.py:80-118) from the N x N Gram matrix of the centred data; the F-sized contractions run on the fp64 matrix
 * cores (products of fp32 data are exact in fp64), only the N x N symmetric eigen-decomposition is left to the caller.
 *   center_cols : xc[N,F] = x[N,F] - column mean                         (F % 4 == 0; xc may alias x)
 *   gram_f64    : G[N,N] (fp64, symmetric, fully written) = xc . xc^T     (F % 4 == 0)
 *   project_rows: out[n,F] (fp32) = Ut[n,N] (fp64, row-major) . xc[N,F]
 *   normalize_rows_signed: every row of v[n,F] to unit length with its largest-magnitude entry positive */
USPACE_API int uspace_center_cols_f32(const float* x, float* xc, int N, long F, uspace_stream_t stream);
USPACE_API int uspace_gram_f64(const float* x, double* G, int N, long F, uspace_stream_t stream);
USPACE_API int uspace_project_rows_f64(const double* Ut, const float* x, float* out, int n, int N, long F, uspace_stream_t stream);
USPACE_API int uspace_normalize_rows_signed(float* v, int n, long F, uspace_stream_t stream);

/* fp32 -> bf16 (round to nearest even). */
USPACE_API int uspace_cast_f32_bf16(const float* src, uint16_t* dst, long n, uspace_stream_t stream);

/* ODE state arithmetic (the integrator the reference delegates to torchdiffeq,
 * flow_matching.py:118,140,163,172): out = y + sum_i coef[i] * k[i], n_k <= 8.
 * k is a HOST array of device pointers, coef a HOST array.  out may alias y. */
USPACE_API int uspace_ode_combine(float* out, const float* y, const float* const* k, const float* coef,
                       int n_k, long n, uspace_stream_t stream);

/* Scaled RMS error norm of an embedded Runge-Kutta step:
 *   result[0] = sqrt(mean((err / (atol + rtol * max(|y0|, |y1|)))^2)),  err = sum_i coef[i]*k[i];
 *   result[1] = the sum of squares itself (a batch sharded over GPUs all-reduces these sums, not the norms).
 * A non-finite y0[i] or y1[i] makes that element's ratio NaN (max() would drop a NaN and an Inf would make the ratio 0),
 * so a step whose state is no longer finite yields a non-finite result[0] and result[1], never an accepted step; a
 * non-finite k[i] reaches err itself.  Finite inputs take the plain arithmetic above.
 * result is a device float[2]; scratch a device float[>=1024]. */
USPACE_API int uspace_ode_error_norm(const float* y0, const float* y1, const float* const* k, const float* coef,
                          int n_k, float rtol, float atol, long n, float* scratch, float* result,
                          uspace_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Whole forward: nnet(x, timesteps, ...) of libs/uvit.py:306-351 / libs/uvit_t2i.py:308-342.
 * ------------------------------------------------------------------------------------- */
typedef struct uspace_uvit_config {
    int img_size;      /* 32 */
    int patch_size;    /* 2 */
    int in_chans;      /* 4 */
    int embed_dim;     /* D: multiple of 64, at most 2048 (the output head keeps its D x 16 weight image in LDS) */
    int depth;         /* even; depth/2 in-blocks, 1 mid, depth/2 out-blocks */
    int num_heads;     /* embed_dim / 64 */
    int mlp_hidden;    /* 4*D */
    int n_extra;       /* extra tokens besides the time token: 0, 1 (label) or 77 (CLIP) */
    int clip_dim;      /* >0: extra tokens = context_embed(context[B,n_extra,clip_dim]); 0: given */
    int time_first;    /* 1: [time, extra, patches]; 0: [extra, time, patches] */
} uspace_uvit_config;

/* Number of fp32 parameter tensors in canonical order, and their element counts.
 * Canonical order (names are the reference state_dict keys, libs/uvit.py:183-291):
 *   pos_embed, patch_embed.proj.weight, patch_embed.proj.bias,
 *   [context_embed.weight, context_embed.bias]            (clip_dim > 0)
 *   for blk in in_blocks.0.., mid_block, out_blocks.0..:
 *       [skip_linear.weight, skip_linear.bias]             (out_blocks only)
 *       norm1.weight, norm1.bias, attn.qkv.weight, attn.proj.weight, attn.proj.bias,
 *       norm2.weight, norm2.bias, mlp.fc1.weight, mlp.fc1.bias, mlp.fc2.weight, mlp.fc2.bias
 *   norm.weight, norm.bias, decoder_pred.weight, decoder_pred.bias,
 *   final_layer.weight, final_layer.bias */
USPACE_API int uspace_uvit_num_params(const uspace_uvit_config* cfg);
USPACE_API long uspace_uvit_param_numel(const uspace_uvit_config* cfg, int index);

USPACE_API size_t uspace_uvit_weight_bytes(const uspace_uvit_config* cfg);
USPACE_API size_t uspace_uvit_workspace_bytes(const uspace_uvit_config* cfg, int B);

/* Repack fp32 parameters (HOST array of DEVICE pointers, canonical order) into the kernel
 * layout inside `blob` (GEMM weights -> bf16, the rest fp32). */
USPACE_API int uspace_uvit_pack_weights(const uspace_uvit_config* cfg, const float* const* params, int n_params,
                             void* blob, size_t blob_bytes, uspace_stream_t stream);

typedef struct uspace_uvit_io {
    const float* x;          /* [B,C,S,S] fp32 */
    const float* t;          /* timesteps, element b at t[b*t_stride] */
    int t_stride;            /* 0 or 1 */
    const float* context;    /* [B,n_extra,clip_dim] fp32 (clip_dim>0) or extra tokens [B,n_extra,D] or NULL */
    const float* mid_delta;  /* optional [L,D] fp32: x += mid_scale*mid_delta after mid_block (libs/uvit.py:336) */
    float mid_scale;
    float* mid_tap;          /* optional [B,L,D] fp32: copy of the mid_block output (hook "read" mode) */
    const float* key_scale;  /* optional [depth+1, B, L] fp32 attention-map column factors per block */
    float* out;              /* [B,C,S,S] fp32 */
    const float* mid_row_scale; /* optional [B] fp32: per-sample factor multiplying mid_scale */
} uspace_uvit_io;

USPACE_API int uspace_uvit_forward(const uspace_uvit_config* cfg, const void* blob, void* workspace,
                        size_t workspace_bytes, const uspace_uvit_io* io, int B, uspace_stream_t stream);

/* uspace_uvit_forward, and after every block's qkv GEMM the head-mean map (uspace_attention_map_bf16, window q0 / nq / k0 / nk) of
 * that block's attention into maps[(i * B + b) * nq * nk ...], i = 0 .. depth (in-blocks, mid, out-blocks = the reference's
 * _counter["block_id"], libs/uvit_t2i.py:107,316).  maps: caller-owned device float[(depth + 1) * B * nq * nk]; the workspace is that
 * of uspace_uvit_forward.  Every other launch is the one uspace_uvit_forward issues, in the same order, so io->out is bit-equal to
 * its; io->key_scale edits io->out and the later blocks as there, never the map of the block it is applied in. */
USPACE_API int uspace_uvit_forward_maps(const uspace_uvit_config* cfg, const void* blob, void* workspace, size_t workspace_bytes,
                                        const uspace_uvit_io* io, int B, int q0, int nq, int k0, int nk, float* maps,
                                        uspace_stream_t stream);

/* Classifier-free guidance inside the forward: ONE evaluation over 2B rows -- row b the conditional branch (x[b], t[b], context[b]),
 * row B + b the unconditional one (x[b], t[b], uncond[b], or uncond itself when uncond_batched == 0) -- and one uspace_cfg_combine
 * (scale, row_scale as there) of the 2B predictions into io->out [B,C,S,S].
 *   io       describes the B samples as for uspace_uvit_forward.  key_scale, when given, is [depth+1, 2B, L] (the caller puts ones in
 *            the rows of the unconditional half); mid_delta / mid_scale act on all 2B rows; mid_row_scale, when given, is float[2B];
 *            mid_tap must be NULL.
 *   uncond   the unconditional branch's context in the form of io->context: [n_extra, clip_dim] / [n_extra, D], or B of them.
 *            A config with n_extra == 0 has no condition to drop: USPACE_ERR_ARG.
 *   pair_out optional [2B,C,S,S]: receives the 2B predictions (conditional rows first); with NULL they stay in the workspace.
 *   workspace of uspace_uvit_cfg_workspace_bytes(cfg, B) bytes: a plain forward's at batch 2B, then the predictions.
 * The launches are those of uspace_uvit_forward at batch 2B -- same GEMM forms, LayerNorm mode and K-split decisions, same attention
 * launches (and records) -- except that the context cast and the token embedding are issued once per half, each reading x, t and its
 * context where the caller holds them: neither a doubled x nor a second context batch is staged.  An unbatched uncond is cast into
 * each sample's rows and embedded with the rest (one GEMM over 2B * n_extra rows).  The 2B predictions are bit-equal to
 * uspace_uvit_forward at batch 2B on the explicitly concatenated inputs. */
USPACE_API size_t uspace_uvit_cfg_workspace_bytes(const uspace_uvit_config* cfg, int B);
USPACE_API int uspace_uvit_forward_cfg(const uspace_uvit_config* cfg, const void* blob, void* workspace, size_t workspace_bytes,
                                       const uspace_uvit_io* io, int B, const float* uncond, int uncond_batched, float scale,
                                       const float* row_scale, float* pair_out, uspace_stream_t stream);

/* Test aid: run the forward exactly as uspace_uvit_forward does up to the end of stage `stop_after`, then copy the fp32 residual
 * stream x [B,L,D] to `dump` (device) and return.  Stages: 0 the tokens after embed + pos_embed, as block 0 reads them; k = 1 ..
 * depth+1 x after block k-1 (in_blocks, then mid_block at k = depth/2 + 1, then out_blocks).  For the mid block that is the value
 * after the mid hook's add (what the next block reads; io->mid_tap still receives the value before it).  At stop_after = depth+1
 * the head runs as well and io->out receives the forward's output. */
USPACE_API int uspace_uvit_forward_tap(const uspace_uvit_config* cfg, const void* blob, void* workspace, size_t workspace_bytes,
                                       const uspace_uvit_io* io, int B, int stop_after, float* dump, uspace_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * VAE decode (the step after the solve): FrozenAutoencoderKL.decode of libs/autoencoder.py:446-450 =
 * z / scale_factor -> post_quant_conv -> Decoder.forward (libs/autoencoder.py:376-409).
 * ------------------------------------------------------------------------------------- */
typedef struct uspace_vae_config {
    int ch;              /* 128 */
    int ch_mult[4];      /* {1,2,4,4} */
    int n_levels;        /* 4 */
    int num_res_blocks;  /* 2 */
    int resolution;      /* 256 (output); latents are resolution >> (n_levels-1) */
} uspace_vae_config;

/* GroupNorm(32 groups, C, eps) (+ x*sigmoid(x) when silu != 0) over a zero-bordered NHWC fp32 map
 * [B, H+2, H+2, C] -> bf16 operand map of the same geometry with the border rows zeroed
 * (libs/autoencoder.py:26-32).  C a power of two in [64, 512]; stats_scratch: device float[B*257*64].
 * Deterministic (no atomics): repeated calls give bit-identical results. */
USPACE_API int uspace_groupnorm_map_bf16(const float* x, const float* gamma, const float* beta, uint16_t* y,
                                         float* stats_scratch, int B, int H, int C, int silu, float eps,
                                         uspace_stream_t stream);

/* parameter tensors in the reference's state_dict order: decoder.* then post_quant_conv.* */
USPACE_API int uspace_vae_num_params(const uspace_vae_config* cfg);
USPACE_API long uspace_vae_param_numel(const uspace_vae_config* cfg, int index);
USPACE_API size_t uspace_vae_weight_bytes(const uspace_vae_config* cfg);
USPACE_API size_t uspace_vae_workspace_bytes(const uspace_vae_config* cfg, int B);
USPACE_API int uspace_vae_pack_weights(const uspace_vae_config* cfg, const float* const* params, int n_params,
                                       void* blob, size_t blob_bytes, uspace_stream_t stream);
/* z [B,4,h,h] fp32 (NCHW) -> out [B,3,resolution,resolution] fp32 (NCHW).  B * (resolution+2)^2 * 512 must stay
 * below 2^30 (decode in chunks, as the reference does: dissect_lfm.py:86-98). */
USPACE_API int uspace_vae_decode(const uspace_vae_config* cfg, const void* blob, void* workspace, size_t workspace_bytes,
                                 const float* z, float scale_factor, float* out, int B, uspace_stream_t stream);

/* Test aid: stop after stage `stop_after` (0 conv_in, 1 mid.block_1, 2 mid.attn_1, 3 mid.block_2, then one per
 * res block / upsample conv in execution order) and copy that fp32 zero-bordered NHWC map [B,H+2,H+2,C] to
 * `dump` (device, large enough); hc_out (host int[2]) receives {H, C}. */
USPACE_API int uspace_vae_decode_tap(const uspace_vae_config* cfg, const void* blob, void* workspace, size_t workspace_bytes,
                                     const float* z, float scale_factor, int B, int stop_after, float* dump, int* hc_out,
                                     uspace_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * VAE encode (images -> latents): FrozenAutoencoderKL.encode_moments / sample of libs/autoencoder.py:428-442 =
 * Encoder.forward (:215-300; double_z, 3 input channels, no attention in the down path, Downsample with a conv)
 * -> quant_conv.  Same uspace_vae_config as the decode; ch must also be a power of two.
 * ------------------------------------------------------------------------------------- */
/* parameter tensors in the reference's state_dict order: encoder.* then quant_conv.* */
USPACE_API int uspace_vae_enc_num_params(const uspace_vae_config* cfg);
USPACE_API long uspace_vae_enc_param_numel(const uspace_vae_config* cfg, int index);
USPACE_API size_t uspace_vae_enc_weight_bytes(const uspace_vae_config* cfg);
USPACE_API size_t uspace_vae_enc_workspace_bytes(const uspace_vae_config* cfg, int B);
USPACE_API int uspace_vae_enc_pack_weights(const uspace_vae_config* cfg, const float* const* params, int n_params,
                                           void* blob, size_t blob_bytes, uspace_stream_t stream);
/* img [B,3,resolution,resolution] fp32 (NCHW) -> moments [B,8,h,h] fp32 (NCHW; mean = channels 0-3, logvar = 4-7).
 * Every map stays below 2^30 elements: B * (resolution+2)^2 * ch < 2^30, at the SD shape B <= 126 (encode in chunks);
 * larger B returns USPACE_ERR_ARG. */
USPACE_API int uspace_vae_encode_moments(const uspace_vae_config* cfg, const void* blob, void* workspace,
                                         size_t workspace_bytes, const float* img, float* moments, int B,
                                         uspace_stream_t stream);
/* Test aid: stop after stage `stop_after` (0 conv_in, then one per res block / downsample of the down path in
 * execution order, then mid.block_1, mid.attn_1, mid.block_2) and copy that fp32 zero-bordered NHWC map
 * [B,H+2,H+2,C] to `dump` (device, large enough); hc_out (host int[2]) receives {H, C}. */
USPACE_API int uspace_vae_encode_tap(const uspace_vae_config* cfg, const void* blob, void* workspace, size_t workspace_bytes,
                                     const float* img, int B, int stop_after, float* dump, int* hc_out,
                                     uspace_stream_t stream);
/* z = scale * (mean + exp(0.5 * clamp(logvar, -30, 20)) * noise): moments [B,8,h,h], noise / z [B,4,h,h], fp32 NCHW */
USPACE_API int uspace_vae_sample(const float* moments, const float* noise, float scale, float* z, int B, int h,
                                 uspace_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * FID: the Inception-v3 feature extractor of pytorch-fid (reference tools/inception.py, fid_inception_v3 up to the final
 * average pool) and the fp64 statistics of its features (tools/fid_score.py).  fp32 operands on the fp32 matrix cores;
 * each output is a fixed k-ordered fp32 fma chain, so each image's features are bit-identical across batch sizes.
 * ------------------------------------------------------------------------------------- */
/* 470 parameter tensors: per BasicConv2d in torchvision Inception3's state_dict order, conv.weight [Cout,Cin,kh,kw] then
 * bn.weight, bn.bias, bn.running_mean, bn.running_var [Cout] (fp32, device).  Packing folds BN (eps 1e-3) in fp64. */
USPACE_API int uspace_inception_num_params(void);
USPACE_API long uspace_inception_param_numel(int index);
USPACE_API size_t uspace_inception_weight_bytes(void);
USPACE_API size_t uspace_inception_workspace_bytes(int B, int H, int W);
USPACE_API int uspace_inception_pack_weights(const float* const* params, int n_params, void* blob, size_t blob_bytes,
                                             uspace_stream_t stream);
/* x [B,3,H,W] fp32 (NCHW, values in [0,1]) -> bilinear resize to 299 x 299 (align_corners=False), 2x - 1, the network up to
 * block `last_block` (0: first max pool, 64; 1: second max pool, 192; 2: Mixed_6e, 768; 3: Mixed_7c, 2048) and its global
 * spatial mean -> feat [B, dims] fp32.  B * 147 * 147 * 64 and B * 3 * H * W must stay below 2^31 (run in chunks). */
USPACE_API int uspace_inception_forward(const void* blob, void* workspace, size_t workspace_bytes, const float* x, int B,
                                        int H, int W, int last_block, float* feat, uspace_stream_t stream);
/* Test aid: run up to `stage` and copy its output to `out` (device, large enough): 0 the resized, normalised input
 * [B,299,299,3]; 1-3 Conv2d_1a/2a/2b; 4 max pool; 5-6 Conv2d_3b/4a; 7 max pool; 8-10 Mixed_5b-5d; 11 Mixed_6a; 12-15
 * Mixed_6b-6e; 16 Mixed_7a; 17-18 Mixed_7b/7c (all NHWC [B,H,W,C]); 19 the global mean [B,2048]. */
USPACE_API int uspace_inception_tap(const void* blob, void* workspace, size_t workspace_bytes, const float* x, int B, int H,
                                    int W, int stage, float* out, uspace_stream_t stream);
/* In place, in fp64: s1[F] += sum_b (feat[b] - shift), s2[F,F] += sum_b (feat[b] - shift)(feat[b] - shift)^T for
 * feat [B,F] fp32; shift [F] fp64 (the first batch's mean).  Deterministic: every element has one owner. */
USPACE_API int uspace_fid_stats_accumulate(const float* feat, int B, int F, const double* shift, double* s1, double* s2,
                                           uspace_stream_t stream);

/* hipGraph form of the forward.  _create() runs the forward once eagerly on `capture_stream` (must be a
 * real, non-NULL stream), then captures the same launch sequence and instantiates it.  The pointers in
 * `io`, the blob and the workspace are baked in: keep them alive and stable, refresh their CONTENTS
 * before each _launch().  Replaces ~160 host launches per network evaluation with one. */
typedef struct uspace_uvit_graph uspace_uvit_graph;
USPACE_API int uspace_uvit_graph_create(const uspace_uvit_config* cfg, const void* blob, void* workspace,
                                        size_t workspace_bytes, const uspace_uvit_io* io, int B,
                                        uspace_stream_t capture_stream, uspace_uvit_graph** out);
USPACE_API int uspace_uvit_graph_launch(uspace_uvit_graph* g, uspace_stream_t stream);
USPACE_API int uspace_uvit_graph_destroy(uspace_uvit_graph* g);

/* ------------------------------------------------------------------------------------------------
 * CLIP text transformer: the encoder behind FrozenCLIPEmbedder (libs/clip.py:40-91), i.e. Hugging Face
 * CLIPTextModel(input_ids).last_hidden_state -- token + position table lookup, pre-LN blocks with causal attention
 * (head_dim 64) and a quick-GELU MLP, final LayerNorm.  Tokenisation stays on the host (libs/clip.py:64-72).
 * ---------------------------------------------------------------------------------------------- */
typedef struct uspace_clip_config {
    int vocab;    /* 49408 */
    int dim;      /* 768 = heads * 64 */
    int heads;    /* 12 */
    int layers;   /* 12 */
    int ffn;      /* 3072 */
    int max_pos;  /* 77 */
    float eps;    /* 1e-5 */
} uspace_clip_config;

/* parameter tensors in the HF state_dict order: embeddings.token_embedding.weight, embeddings.position_embedding.weight,
 * per layer self_attn.{k,v,q,out}_proj.{weight,bias}, layer_norm1.*, mlp.fc1.*, mlp.fc2.*, layer_norm2.*, then
 * final_layer_norm.{weight,bias} */
USPACE_API int uspace_clip_num_params(const uspace_clip_config* cfg);
USPACE_API long uspace_clip_param_numel(const uspace_clip_config* cfg, int index);
USPACE_API size_t uspace_clip_weight_bytes(const uspace_clip_config* cfg);
USPACE_API size_t uspace_clip_workspace_bytes(const uspace_clip_config* cfg, int B);
USPACE_API int uspace_clip_pack_weights(const uspace_clip_config* cfg, const float* const* params, int n_params, void* blob,
                                        size_t blob_bytes, uspace_stream_t stream);
/* ids: device int32 [B, L] (L <= max_pos); out: device fp32 [B, L, dim].  stop_after_layer < 0: last_hidden_state;
 * k >= 0: the hidden state after k layers without the final norm (HF output_hidden_states[k]; test aid). */
USPACE_API int uspace_clip_text_forward(const uspace_clip_config* cfg, const void* blob, void* workspace, size_t workspace_bytes,
                                        const int* ids, float* out, int B, int L, int stop_after_layer, uspace_stream_t stream);

/* causal attention over packed qkv (as uspace_attention_bf16, key k visible to query q iff k <= q); L <= 160 */
USPACE_API int uspace_attention_causal_bf16(const uint16_t* qkv, uint16_t* out, int B, int L, int H, uspace_stream_t stream);
/* LayerNorm with fp32 output (final norms) */
USPACE_API int uspace_layernorm_f32(const float* x, const float* gamma, const float* beta, float* y, int M, int D, float eps,
                                    uspace_stream_t stream);
/* out[b,l,:] = tok_table[ids[b,l],:] + pos_table[l,:]  (HF CLIPTextEmbeddings) */
USPACE_API int uspace_table_embed(const int* ids, const float* tok_table, const float* pos_table, float* out, int B, int L, int D,
                                  int vocab, uspace_stream_t stream);
/* x <- x * sigmoid(1.702 x) in place, bf16 (HF QuickGELUActivation); n % 4 == 0 */
USPACE_API int uspace_quick_gelu_bf16(uint16_t* x, long n, uspace_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * CLIP score: the image side of CLIP (Hugging Face CLIPVisionModelWithProjection: patch embedding, class token + position
 * table, pre_layrnorm, pre-LN blocks with NON-causal attention and a quick-GELU MLP, post_layernorm of the class token,
 * visual_projection), the image preprocessing in front of it and the fp32 pieces of the metric.  Added under ABI 11: new
 * symbols only.
 * ---------------------------------------------------------------------------------------------- */
/* (declared struct-then-typedef: the generated ctypes stub of INTEGRATION.md lists the `typedef struct {` configs of the
 * sampling path; the binding of this one is uspace_amd/_hip.py ClipVisionConfig) */
struct uspace_clipv_config {
    int image;     /* 224: side of pixel_values; image % patch == 0 */
    int patch;     /* 14 */
    int dim;       /* 1024 = heads * 64 */
    int heads;     /* 16 */
    int layers;    /* 24 */
    int ffn;       /* 4096; % 64 == 0 */
    int proj_dim;  /* 768; % 4 == 0 */
    float eps;     /* 1e-5 */
};
typedef struct uspace_clipv_config uspace_clipv_config;

/* parameter tensors in the HF state_dict order: embeddings.class_embedding [dim], embeddings.patch_embedding.weight
 * [dim, 3, patch, patch] (no bias), embeddings.position_embedding.weight [(image / patch)^2 + 1, dim], pre_layrnorm.{weight,bias}
 * (HF's spelling), per layer self_attn.{k,v,q,out}_proj.{weight,bias}, layer_norm1.*, mlp.fc1.*, mlp.fc2.*, layer_norm2.*, then
 * post_layernorm.{weight,bias} and visual_projection.weight [proj_dim, dim].  The patch weight is stored bf16 as [dim, Kp],
 * Kp = 3 patch^2 rounded up to 64 with zero columns (the GEMM's K % 64 == 0; ViT-L/14: 588 -> 640); visual_projection stays fp32.
 * An invalid config gives USPACE_ERR_ARG / 0 bytes. */
USPACE_API int uspace_clipv_num_params(const uspace_clipv_config* cfg);
USPACE_API long uspace_clipv_param_numel(const uspace_clipv_config* cfg, int index);
USPACE_API size_t uspace_clipv_weight_bytes(const uspace_clipv_config* cfg);
USPACE_API size_t uspace_clipv_workspace_bytes(const uspace_clipv_config* cfg, int B);
USPACE_API int uspace_clipv_pack_weights(const uspace_clipv_config* cfg, const float* const* params, int n_params, void* blob,
                                         size_t blob_bytes, uspace_stream_t stream);
/* pixel_values: fp32 [B, 3, image, image] (uspace_clip_preprocess's output) -> image_embeds fp32 [B, proj_dim] and, where
 * pooler_output != NULL, post_layernorm(class token) fp32 [B, dim].  Patch rows in (c, py, px) order as bf16 -> uspace_gemm_bf16;
 * the attention is uspace_attention_bf16 where uspace_attention_plan accepts the token count, uspace_attention_long_bf16 beyond.
 * stop_after_layer = -1: the whole model.  Test aid, written to tap_out fp32 [B, tokens, dim] instead (image_embeds may be
 * NULL): k >= 0 the hidden state after k layers (k = 0: after pre_layrnorm; HF hidden_states[k]), -2 the embeddings before
 * pre_layrnorm. */
USPACE_API int uspace_clipv_forward(const uspace_clipv_config* cfg, const void* blob, void* workspace, size_t workspace_bytes,
                                    const float* pixel_values, float* image_embeds, float* pooler_output, int B, int stop_after_layer,
                                    float* tap_out, uspace_stream_t stream);

/* images fp32 [B, 3, H, W] in [0, 1] (H == W; anything else: USPACE_ERR_ARG) -> pixel_values fp32 [B, 3, S, S]:
 *   v = 255 x, with quantize != 0 v = clamp(floor(255 x + 0.5), 0, 255), each step rounded to fp32
 *   (save_image's rounding, ties included);
 *   separable antialiased bicubic resize to S: Keys filter a = -0.5 of support 2 max(H / S, 1) around the centre (o + 0.5) H / S,
 *   the window clipped to the image and its weights renormalised per output pixel (torch interpolate(mode="bicubic",
 *   antialias=True, align_corners=False)); the result is NOT rounded back to uint8;
 *   out = (clamp(v, 0, 255) / 255 - mean[c]) / std[c].   mean, std: HOST float[3].  H <= 4096, H / S <= 63. */
USPACE_API int uspace_clip_preprocess(const float* images, float* pixel_values, int B, int H, int W, int S, int quantize,
                                      const float* mean, const float* std, uspace_stream_t stream);
/* out[B, N] = x[B, K] . w[N, K]^T in fp32 (weights, products and sums), no bias: the two CLIP projections.  K % 4 == 0. */
USPACE_API int uspace_linear_f32(const float* x, const float* w, float* out, int B, int N, int K, uspace_stream_t stream);
/* out[b, :] = x[b, idx[b], :] of x fp32 [B, L, D]; idx: device int32 [B] in [0, L) (the text pooling position) */
USPACE_API int uspace_gather_rows_f32(const float* x, const int* idx, float* out, int B, int L, int D, uspace_stream_t stream);
/* out[b] = scale <a_b, b_b> / (|a_b| |b_b|), with relu != 0 max(., 0); a, b fp32 [B, D].  One wave per row, fixed summation
 * order, no atomics.  A zero row gives NaN, as the division does. */
USPACE_API int uspace_cosine_f32(const float* a, const float* b, float* out, int B, int D, float scale, int relu,
                                 uspace_stream_t stream);
/* out[b, :] = a_b / |a_b| - b_b / |b_b|: the step between two embeddings on the unit sphere (directional similarity) */
USPACE_API int uspace_normalized_diff_f32(const float* a, const float* b, float* out, int B, int D, uspace_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Feature-set metrics (KID, precision / recall / density / coverage; uspace_amd/tools/feature_metrics.py): reductions over
 * the pairwise quantities of two fp32 row-major feature sets x [nx, F] and y [ny, F] on the device, F >= 1, n, nx, ny <= 2^24.
 * Everything is fp64: the dot product x_i . y_j by v_mfma_f64_16x16x4_f64 over the fp32 values widened to fp64, and
 *   D2(i, j) = max(0, |x_i|^2 + |y_j|^2 - 2 x_i . y_j),
 * the squared norms computed once per call and set by one fixed-order kernel.  The nx x ny matrix is never stored: a workgroup
 * owns 64 rows and walks the column tiles, the reductions fused.  No floating-point atomics: every output is bit-equal from
 * run to run.  workspace: uspace_metric_workspace_bytes(nx, ny, n_subsets, m) bytes (norms of both sets + the partial sums of
 * uspace_metric_poly_sums; pass ny = 0 for uspace_metric_knn_radius2, n_subsets = m = 0 where no sums are asked for); 0 on
 * invalid arguments.  The layout is one formula for all consumers, norms first: uspace_metric_poly_sums computes no norms and
 * leaves those (nx + ny) doubles untouched ahead of its partial sums (128 MiB per 2^24-row set, allocated and unused).
 * Nothing of the workspace is read before it is written.  These functions were added without a change
 * of USPACE_ABI_VERSION: they only add symbols.
 * ------------------------------------------------------------------------------------- */
USPACE_API size_t uspace_metric_workspace_bytes(int nx, int ny, int n_subsets, int m);
/* radius2[i] = the k-th smallest D2(i, j) over j != i (excluded by index) within one set x [n, F]; 1 <= k <= 16, k <= n - 1,
 * otherwise USPACE_ERR_ARG.  A sorted list of the k smallest per row is merged tile by tile. */
USPACE_API int uspace_metric_knn_radius2(const float* x, int n, int F, int k, double* radius2, void* workspace,
                                         size_t workspace_bytes, uspace_stream_t stream);
/* count[i] = #{j : D2(i, j) <= radius2_y[j]} (int32 [nx]; needs radius2_y fp64 [ny]) and min_d2[i] = min_j D2(i, j) (fp64 [nx]).
 * Either output may be NULL, not both. */
USPACE_API int uspace_metric_manifold(const float* x, int nx, const float* y, int ny, int F, const double* radius2_y, int* count,
                                      double* min_d2, void* workspace, size_t workspace_bytes, uspace_stream_t stream);
/* With K(a, b) = (gamma a . b + coef0)^degree, degree an integer in 1 .. 8 applied by multiplication, and idx_x, idx_y device
 * int32 [n_subsets, m] row indices into x and y (the caller validates them; 1 <= m <= min(nx, ny), n_subsets <= 65535):
 *   sums[s, 0] = sum_{p != q} K(x[idx_x[s, p]], x[idx_x[s, q]]),   sums[s, 1] = the same for y and idx_y,
 *   sums[s, 2] = sum_{p, q} K(x[idx_x[s, p]], y[idx_y[s, q]]);     sums: fp64 [n_subsets, 3].
 * The diagonal is excluded by position p == q.  Per-workgroup partial sums are finished in a fixed order. */
USPACE_API int uspace_metric_poly_sums(const float* x, int nx, const float* y, int ny, int F, const int* idx_x, const int* idx_y,
                                       int n_subsets, int m, int degree, double gamma, double coef0, double* sums, void* workspace,
                                       size_t workspace_bytes, uspace_stream_t stream);
/* The sums of the Gaussian RBF kernel K(a, b) = exp(-gamma D2(a, b)) behind MMD^2 / CMMD (uspace_amd/tools/cmmd.py), over whole sets:
 *   sums[0] = sum_{i != j} K(x_i, x_j),   sums[1] = sum_{i != j} K(y_i, y_j),   sums[2] = sum_{i, j} K(x_i, y_j);   sums: fp64 [3].
 * The diagonal is left out by index (K(a, a) = 1 is the caller's to add where its estimator wants it), and so is everything beyond
 * either set.  normalize = 1: D2 is taken between the unit vectors a / |a|, b / |b|, formed in fp64 from the same dot product and
 * norms -- no fp32 normalisation pass, no second copy of the features; a zero row counts as the zero vector.  normalize = 0: the
 * raw D2 above.  exp is the fp64 device exp; K <= 1 because D2 >= 0.  One launch over the three set pairs, per-workgroup partial
 * sums finished in a fixed order, no atomics: bit-equal from run to run.  USPACE_ERR_ARG: a NULL pointer, nx or ny outside
 * 1 .. 2^24, F < 1, gamma negative or not finite, normalize not 0 or 1 -- checked, like USPACE_ERR_WORKSPACE, before any GPU work.
 * workspace: uspace_metric_workspace_bytes(nx, ny, 1, max(nx, ny)) bytes (the norms of both sets, then three partial sums per
 * 64-row block of the larger set); nothing of it is read before it is written.  Symbols only: USPACE_ABI_VERSION is unchanged. */
USPACE_API int uspace_metric_rbf_sums(const float* x, int nx, const float* y, int ny, int F, double gamma, int normalize,
                                      double* sums, void* workspace, size_t workspace_bytes, uspace_stream_t stream);
/* The k nearest rows of y for every row of x, with their indices (uspace_amd/tools/neighbors.py): d2 fp64 [nx, k] and idx int32
 * [nx, k], each row ascending in the lexicographic order (d2, index).  1 <= k <= 16, F >= 1, nx, ny in 1 .. 2^24; k may exceed the
 * number of eligible columns, and the tail of such a row is d2 = +inf, idx = -1.
 *   Indices: idx holds index_base + j (y may be a shard of a larger bank; index_base >= 0 and index_base + ny - 1 <= INT_MAX).
 *   self_base >= 0 leaves column j out for row i where index_base + j == self_base + i -- a set queried against itself, sharded
 *   or not; self_base = -1 leaves nothing out.
 *   Selection is by the engine's D2 above, which is accurate to an absolute 8 F u (|x|^2 + |y|^2), u = 2^-53: the k-th and the
 *   (k + 1)-th candidate can be exchanged only where they lie within twice that ceiling of each other.  Equal rows of y give
 *   bit-equal D2 and come out in index order.
 *   Reported values are refined in the same call: each kept pair is recomputed as sum_f (x_if - y_jf)^2 with the differences formed
 *   in fp64 from the fp32 values (one wave per pair, the summation order of the norms), so an exact copy reports exactly 0.0; each
 *   row is then sorted again by (refined d2, index).  |d2 - exact| <= 4 F u d2.
 * No atomics, one fixed order: a row's result is bit-equal from run to run and the same whether the row is alone or among others.
 * workspace: uspace_metric_workspace_bytes(nx, ny, 0, 0) bytes, the two norm arrays.  USPACE_ERR_ARG (a NULL pointer, a size,
 * k, F, index_base or self_base outside the ranges above) and USPACE_ERR_WORKSPACE are returned before any GPU work.  Symbols
 * only: USPACE_ABI_VERSION is unchanged. */
USPACE_API int uspace_metric_topk(const float* x, int nx, const float* y, int ny, int F, int k, int index_base, int self_base,
                                  double* d2, int* idx, void* workspace, size_t workspace_bytes, uspace_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Inception Score and sFID (uspace_amd/tools/inception_score.py, sfid_score.py, eval_suite.py): the pool features, the
 * spatial features and the logits from ONE walk of the network, and the fp64 statistics of the score.  These are the numbers
 * of the pytorch-fid port of the network, not of the TF graph.  Added without a change of USPACE_ABI_VERSION: symbols only.
 * ------------------------------------------------------------------------------------- */
/* uspace_inception_forward(last_block = 3) with one addition: right after tap stage `spatial_stage` (1 .. 18, numbered as in
 * uspace_inception_tap) is complete, channels [0, spatial_channels) of every pixel are gathered to
 * spatial [B, h * w * spatial_channels] in (h, w, c) order.  sFID's features are stage 14 (Mixed_6d), 7 channels: the first 7
 * of Mixed_6d.branch1x1 after BN and ReLU, 17 * 17 * 7 = 2023 values per image.  pool [B, 2048] and the workspace
 * (uspace_inception_workspace_bytes) are those of uspace_inception_forward, bit for bit; spatial == NULL skips the gather.
 * spatial_stage outside 1 .. 18 or spatial_channels outside 1 .. the stage's channels: USPACE_ERR_ARG, checked either way. */
USPACE_API int uspace_inception_forward_suite(const void* blob, void* workspace, size_t workspace_bytes, const float* x, int B,
                                              int H, int W, float* pool, float* spatial, int spatial_stage, int spatial_channels,
                                              uspace_stream_t stream);
/* logits [B, C] = pool [B, K] . weight [C, K]^T (+ bias [C] unless NULL), no activation: torchvision's fc.  fp32 operands on
 * v_mfma_f32_32x32x2_f32: each logit is the k-ordered fp32 fma chain over K, so a row's logits are bit-identical whatever B it
 * sits in.  Any B >= 1 and C >= 1; K % 16 == 0 and 16-byte aligned pool and weight, anything else USPACE_ERR_ARG.  Plain fp32
 * device tensors, no blob. */
USPACE_API int uspace_inception_logits(const float* pool, const float* weight, const float* bias, float* logits, int B, int K,
                                       int C, uspace_stream_t stream);
/* scores[k] (fp64 [splits], device) = exp(mean_i sum_c p_ic (log p_ic - log pbar_c)) over the rows i of split k =
 * [k N / splits, (k + 1) N / splits) (integer division), p_i = softmax(logits_i), pbar = the split's mean of p_i; terms with
 * p_ic == 0 contribute 0.  logits fp32 [N, C]; all arithmetic fp64; every sum in a fixed order, no atomics: bit-equal from run to
 * run.  1 <= splits <= N <= 2^24, C <= 65536, splits * ceil(ceil(N / splits) / 256) <= 65535; otherwise USPACE_ERR_ARG / 0 bytes.
 * Nothing of the workspace is read before it is written. */
USPACE_API size_t uspace_inception_score_workspace_bytes(int N, int C, int splits);
USPACE_API int uspace_inception_score_f64(const float* logits, int N, int C, int splits, void* workspace, size_t workspace_bytes,
                                          double* scores, uspace_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Paired edit-fidelity metrics (uspace_amd/tools/lpips.py, pair_metrics.py; csrc/lpips.hip): LPIPS, SSIM and PSNR of image
 * pairs, one fp64 value per pair.  Every sum over pixels is fp64 in one fixed order (per-workgroup partial sums over a constant
 * number of pixels, then one wave per image; no atomics), so a pair's value is bit-identical whatever B it sits in and wherever
 * it sits in the batch.  Nothing of a workspace is read before it is written.  Added without a change of USPACE_ABI_VERSION:
 * symbols only.
 *
 * LPIPS (Zhang et al. 2018).  net: 0 = AlexNet, 1 = VGG-16 (torchvision's `features`, convolutions with bias, no batch norm);
 * anything else is USPACE_ERR_ARG (-1 / 0 from the queries).  Parameters, in order: per convolution weight [Cout, Cin, k, k]
 * then bias [Cout]; then lin0 .. lin4, the per-channel weights [C_l] of the five taps (alex: 64, 192, 384, 256, 256 after the
 * five ReLUs; vgg: 64, 128, 256, 512, 512 after relu1_2, 2_2, 3_3, 4_3, 5_3).  The pair runs as one batch of 2B images through
 * the fp32-MFMA convolution the Inception network uses (a k-ordered fp32 fma chain per output); after each tap
 *   d_l[b] = (1 / HW) sum_pixels sum_c w_c (a_c / (sqrt(sum a^2) + 1e-10) - b_c / (sqrt(sum b^2) + 1e-10))^2
 * is computed in this direct form, fp32 per pixel, fp64 over pixels.  x0, x1: fp32 NCHW [B, 3, H, W]; the input is
 * (v - shift_c) / scale_c with v = x (normalize = 0: images in [-1, 1]) or 2 x - 1 (normalize = 1: images in [0, 1]).
 * An input too small for the stack (alex below 31 x 31, vgg below 16 x 16), B > 32767 or a tensor of 2^31 elements or more:
 * USPACE_ERR_ARG / 0 bytes.
 * ------------------------------------------------------------------------------------- */
USPACE_API int uspace_lpips_num_params(int net);
USPACE_API long uspace_lpips_param_numel(int net, int index);
USPACE_API size_t uspace_lpips_weight_bytes(int net);
USPACE_API size_t uspace_lpips_workspace_bytes(int net, int B, int H, int W);
USPACE_API int uspace_lpips_pack_weights(int net, const float* const* params, int n_params, void* blob, size_t blob_bytes,
                                         uspace_stream_t stream);
/* out fp64 [B] = d_0 + .. + d_4 (summed in this order); per_layer fp64 [5, B] (d_l[b] at l * B + b) or NULL. */
USPACE_API int uspace_lpips_forward(int net, const void* blob, void* workspace, size_t workspace_bytes, const float* x0,
                                    const float* x1, int B, int H, int W, int normalize, double* out, double* per_layer,
                                    uspace_stream_t stream);
/* Test aid: the NHWC fp32 activations [2B, h, w, c] of tap stage `stage` (x0's images first): 0 = the scaled input,
 * 1 .. 5 = the five taps.  No head runs. */
USPACE_API int uspace_lpips_tap(int net, const void* blob, void* workspace, size_t workspace_bytes, const float* x0, const float* x1,
                                int B, int H, int W, int normalize, int stage, float* dump, uspace_stream_t stream);
/* The distance head alone: f0, f1 fp32 [B, HW, C] (NHWC), w fp32 [C], out fp64 [B] = d[b] above.  C a multiple of 64 up to 512,
 * B <= 65535; otherwise USPACE_ERR_ARG / 0 bytes. */
USPACE_API size_t uspace_lpips_distance_workspace_bytes(int B, int HW, int C);
USPACE_API int uspace_lpips_distance_f64(const float* f0, const float* f1, const float* w, int B, int HW, int C, void* workspace,
                                         size_t workspace_bytes, double* out, uspace_stream_t stream);
/* SSIM (Wang et al. 2004): x, y fp32 NCHW [B, C, H, W]; Gaussian window of 11 taps, sigma 1.5, normalised to sum 1, applied
 * separably over the "valid" region (H - 10) x (W - 10); population moments per channel; C1 = (0.01 L)^2, C2 = (0.03 L)^2 with
 * L = data_range; out fp64 [B] = the mean of the SSIM map over positions and channels.  The moments and the map are fp32, the
 * mean is fp64.  H or W below 11, B or C above 65535, data_range <= 0: USPACE_ERR_ARG / 0 bytes. */
USPACE_API size_t uspace_ssim_workspace_bytes(int B, int C, int H, int W);
USPACE_API int uspace_ssim_f64(const float* x, const float* y, int B, int C, int H, int W, double data_range, void* workspace,
                               size_t workspace_bytes, double* out, uspace_stream_t stream);
/* PSNR: out fp64 [B] = 10 log10(L^2 / mse), mse = the mean over the n_per_image fp32 values of (x - y)^2, all in fp64;
 * identical images give +inf. */
USPACE_API size_t uspace_psnr_workspace_bytes(int B, long n_per_image);
USPACE_API int uspace_psnr_f64(const float* x, const float* y, int B, long n_per_image, double data_range, void* workspace,
                               size_t workspace_bytes, double* out, uspace_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * DINO towers and the structure distance (uspace_amd/libs/dino.py, tools/dino_metrics.py; csrc/dino.hip): Hugging Face
 * Dinov2Model in eval mode -- class token, patch embedding WITH bias, position table, pre-LN blocks with non-causal attention,
 * an erf-GELU MLP (the GEMM's USPACE_EPI_GELU epilogue) and LayerScale on both branches, final LayerNorm; pooler_output is the
 * final LayerNorm of the class token.  layerscale = 0 gives the plain pre-LN ViT of HF ViTModel (DINO v1).  SwiGLU MLPs and
 * register tokens are not supported.  Added without a change of USPACE_ABI_VERSION: symbols only.
 * ------------------------------------------------------------------------------------- */
/* (struct-then-typedef, as uspace_clipv_config; the binding is uspace_amd/_hip.py DinoConfig) */
struct uspace_dino_config {
    int image;       /* 224: side of pixel_values, the side the tower runs at; image % patch == 0 */
    int patch;       /* 14 */
    int dim;         /* 1024 = heads * 64 */
    int heads;       /* 16 */
    int layers;      /* 24 */
    int ffn;         /* 4096; % 64 == 0 */
    int layerscale;  /* 1: layer_scale1 / layer_scale2 parameters exist (Dinov2Model); 0: none (ViTModel) */
    float eps;       /* 1e-6 (ViTModel: 1e-12) */
};
typedef struct uspace_dino_config uspace_dino_config;

/* parameter tensors in the order of Dinov2Model.state_dict() with embeddings.mask_token dropped: embeddings.cls_token [dim],
 * embeddings.position_embeddings [(image / patch)^2 + 1, dim] -- ALREADY interpolated to this config's grid by the caller --,
 * embeddings.patch_embeddings.projection.{weight [dim, 3, patch, patch], bias}; per layer norm1.{weight,bias},
 * attention.attention.{query,key,value}.{weight,bias}, attention.output.dense.{weight,bias}, layer_scale1.lambda1, norm2.{weight,bias},
 * mlp.fc1.{weight,bias}, mlp.fc2.{weight,bias}, layer_scale2.lambda1 (the two lambda1 only with layerscale = 1); then
 * layernorm.{weight,bias}.  The patch weight is stored bf16 as [dim, Kp], Kp = 3 patch^2 rounded up to 64 with zero columns.
 * LayerScale is folded at pack time: the stored out projection and fc2 are bf16(lambda1[n] * W[n, k]) and lambda1[n] * b[n],
 * computed from the fp32 values.  An invalid config gives USPACE_ERR_ARG / 0 bytes. */
USPACE_API int uspace_dino_num_params(const uspace_dino_config* cfg);
USPACE_API long uspace_dino_param_numel(const uspace_dino_config* cfg, int index);
USPACE_API size_t uspace_dino_weight_bytes(const uspace_dino_config* cfg);
USPACE_API size_t uspace_dino_workspace_bytes(const uspace_dino_config* cfg, int B);
USPACE_API int uspace_dino_pack_weights(const uspace_dino_config* cfg, const float* const* params, int n_params, void* blob,
                                        size_t blob_bytes, uspace_stream_t stream);
/* pixel_values fp32 [B, 3, image, image] -> pooler_output fp32 [B, dim] (may be NULL when only keys are wanted).
 * stop_after_layer = -1: the whole model.  k >= 0: stop after k layers and write the fp32 residual stream [B, tokens, dim] to
 * tap_out (HF hidden_states[k]; k = 0 and -2 both give the embeddings: there is no norm in front of the layers); no pooler then.
 * key_layer = -1: no keys.  l >= 0 (below the number of layers run): the keys of layer l, LN1(x_l) Wk^T + bk with the heads
 * concatenated, as the q|k|v GEMM stored them: bf16 [B, tokens, dim] to keys_out.  With keys asked for, tap_out may be NULL. */
USPACE_API int uspace_dino_forward(const uspace_dino_config* cfg, const void* blob, void* workspace, size_t workspace_bytes,
                                   const float* pixel_values, float* pooler_output, int B, int stop_after_layer, float* tap_out,
                                   int key_layer, uint16_t* keys_out, uspace_stream_t stream);
/* Structure distance (Tumanyan et al. 2022): for pair p with bf16 keys Ka, Kb [T, D] at keys_x + p * pair_stride, rows row_stride
 * elements apart,
 *   S(K)[i, j] = <k_i, k_j> / max(|k_i| |k_j|, 1e-8),   out[p] = (1 / T^2) sum_ij (S(Ka)[i, j] - S(Kb)[i, j])^2     fp64 [P].
 * Both Gram tiles of a 16 x 16 tile pair by v_mfma_f32_16x16x32_bf16 with fp32 accumulation, the norms fp32 sums of squares of
 * the same stored keys, the normalisation after the product; one fp32 sum per tile, the tiles of a pair added in a fixed order
 * in fp64; no atomics, neither T x T matrix stored.  A pair's value is bit-identical from run to run and whatever P it sits in;
 * identical members give exactly 0.  D % 64 == 0, strides % 8 == 0, 16-byte aligned keys, T <= 16384, P <= 65535; otherwise
 * USPACE_ERR_ARG / 0 bytes.  Nothing of the workspace is read before it is written. */
USPACE_API size_t uspace_self_similarity_mse_workspace_bytes(int P, int T);
USPACE_API int uspace_self_similarity_mse_f64(const uint16_t* keys_a, const uint16_t* keys_b, int P, int T, int D, long row_stride,
                                              long pair_stride, void* workspace, size_t workspace_bytes, double* out,
                                              uspace_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * ArcFace identity tower and the ID similarity (uspace_amd/libs/arcface.py, tools/id_metrics.py; csrc/idnet.hip):
 * Backbone(input_size, num_layers, mode) of TreB1eN's InsightFace_Pytorch model_irse.py in eval mode -- IR-SE50 at 112 is the
 * network behind the ID similarity of pSp / e4e.  input_layer = conv3x3(3, 64) + BN + PReLU; units bottleneck_IR(_SE)(in, depth,
 * stride): res = BN -> conv3x3 -> PReLU -> conv3x3(stride) -> BN (-> SE, reduction 16), out = res + shortcut, the shortcut the
 * subsample x[:, :, ::stride, ::stride] where in == depth and conv1x1(stride) + BN otherwise; four levels of 64 / 128 / 256 / 512
 * channels, level l = one unit (in, depth, 2) and blocks[l] - 1 units (depth, depth, 1); output_layer = BN2d -> Flatten (c, y, x)
 * -> Linear(512 (input_size / 16)^2, 512) -> BN1d; the result divided by its l2 norm (no eps).  Batch norms use the running
 * statistics, eps 1e-5.  fp32 NHWC activations, every convolution the fp32-MFMA implicit GEMM (a k-ordered fp32 fma chain);
 * batch norms behind a convolution or the Linear, and output_layer.0, are folded at pack time in fp64; the batch norm in front of
 * a unit's first convolution is applied to in-bounds operands only (the reference zero-pads after it).  Every sum has one
 * fixed order: a sample's embedding and a pair's similarity are bit-identical whatever B they sit in and wherever they sit in the
 * batch.  No atomics; nothing of a workspace is read before it is written.  Added without a change of USPACE_ABI_VERSION:
 * symbols only.
 * ------------------------------------------------------------------------------------- */
/* (struct-then-typedef, as uspace_clipv_config; the binding is uspace_amd/_hip.py IdnetConfig) */
struct uspace_idnet_config {
    int input_size;  /* 112: side of the aligned face crop; a positive multiple of 16, at most 4096 */
    int blocks[4];   /* units per level: IR-50 (3, 4, 14, 3), IR-100 (3, 13, 30, 3), IR-152 (3, 8, 36, 3); each >= 1 */
    int se;          /* 1: mode "ir_se" (SE modules), 0: mode "ir" */
};
typedef struct uspace_idnet_config uspace_idnet_config;

/* parameter tensors in the module's state_dict order with the num_batches_tracked buffers dropped; a batch norm is weight, bias,
 * running_mean, running_var: input_layer.0.weight [64, 3, 3, 3], input_layer.1.*, input_layer.2.weight [64] (PReLU);
 * output_layer.0.* [512], output_layer.3.weight [512, 512 (input_size / 16)^2], output_layer.3.bias, output_layer.4.*; per unit
 * body.u: shortcut_layer.0.weight [depth, in, 1, 1] and shortcut_layer.1.* (only where in != depth), res_layer.0.* [in],
 * res_layer.1.weight [depth, in, 3, 3], res_layer.2.weight [depth], res_layer.3.weight [depth, depth, 3, 3], res_layer.4.*,
 * res_layer.5.fc1.weight [depth / 16, depth, 1, 1], res_layer.5.fc2.weight [depth, depth / 16, 1, 1] (the two only with se).
 * The blob is fp32 pieces on the 256-byte grid of csrc/blob.h; the Linear is stored permuted to (y, x, c).  An invalid config
 * gives USPACE_ERR_ARG (-1 from param_numel) / 0 bytes; B outside 1 .. 32767 or a tensor of 2^31 elements or more likewise. */
USPACE_API int uspace_idnet_num_params(const uspace_idnet_config* cfg);
USPACE_API long uspace_idnet_param_numel(const uspace_idnet_config* cfg, int index);
USPACE_API size_t uspace_idnet_weight_bytes(const uspace_idnet_config* cfg);
USPACE_API size_t uspace_idnet_workspace_bytes(const uspace_idnet_config* cfg, int B);
USPACE_API int uspace_idnet_pack_weights(const uspace_idnet_config* cfg, const float* const* params, int n_params, void* blob,
                                         size_t blob_bytes, uspace_stream_t stream);
/* x: fp32 NCHW [B, 3, H, W] -> out: fp32 NHWC [B, out_size, out_size, 3].  normalize != 0 maps [0, 1] to [-1, 1] first
 * (2 x - 1).  crop != 0 is the ID loss of pSp / e4e: adaptive average pooling to 256 x 256 unless the input has that size, the
 * crop [35:223, 32:220] (188 x 188), adaptive average pooling to out_size.  crop == 0 pools the whole image to out_size (inputs
 * that are aligned crops already).  Adaptive pooling: output i of O averages inputs floor(i N / O) .. ceil((i + 1) N / O) - 1;
 * every window sum is fp32 in row-major order, divided by the count, the 256 x 256 values rounded to fp32 as a stored map would
 * be.  H, W <= 16384, out_size <= 4096, both tensors below 2^31 elements; otherwise USPACE_ERR_ARG. */
USPACE_API int uspace_idnet_preprocess(const float* x, int B, int H, int W, int normalize, int crop, int out_size, float* out,
                                       uspace_stream_t stream);
/* x_nhwc: fp32 [B, input_size, input_size, 3] in [-1, 1] (uspace_idnet_preprocess's output) -> emb fp32 [B, 512], unit length */
USPACE_API int uspace_idnet_forward(const uspace_idnet_config* cfg, const void* blob, void* workspace, size_t workspace_bytes,
                                    const float* x_nhwc, int B, float* emb, uspace_stream_t stream);
/* Test aid: stage 0 = input_layer's output, 1 + u = unit u's output (NHWC fp32 [B, h, w, c]), 1 + (number of units) = the
 * 512-vector before the l2 normalisation, fp32 [B, 512].  Nothing after the stage runs. */
USPACE_API int uspace_idnet_tap(const uspace_idnet_config* cfg, const void* blob, void* workspace, size_t workspace_bytes,
                                const float* x_nhwc, int B, int stage, float* dump, uspace_stream_t stream);
/* Test aid: unit `unit` of the packed tower alone on any map x_nhwc fp32 [B, H, W, in] (1 <= H, W <= 4096; odd sizes, which no
 * valid input_size reaches) -> out fp32 [B, (H - 1) / stride + 1, (W - 1) / stride + 1, depth]. */
USPACE_API size_t uspace_idnet_unit_workspace_bytes(const uspace_idnet_config* cfg, int unit, int B, int H, int W);
USPACE_API int uspace_idnet_unit(const uspace_idnet_config* cfg, const void* blob, void* workspace, size_t workspace_bytes, int unit,
                                 const float* x_nhwc, int B, int H, int W, float* out, uspace_stream_t stream);
/* out[b] = sum_k ea[b, k] eb[b, k] over the 512 entries of two embeddings fp32 [B, 512]: products and sum in fp64, in k order */
USPACE_API int uspace_idnet_similarity_f64(const float* ea, const float* eb, int B, double* out, uspace_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Attribute-classifier tower and the effect of an attribute edit (uspace_amd/libs/resnet.py, tools/attr_metrics.py;
 * csrc/resnet.hip): a torchvision-layout ResNet in eval mode, groups 1.  Stem: conv1 7 x 7 stride 2 padding 3 without bias, bn1,
 * ReLU, max pool 3 x 3 stride 2 padding 1 (floor mode).  Body: layer1 .. layer4 of blocks[l] blocks; the first block of layers
 * 2 - 4 has stride 2.  BasicBlock: conv3x3(stride) bn relu conv3x3 bn; Bottleneck: conv1x1 bn relu conv3x3(stride) bn relu conv1x1
 * bn (the stride on the 3 x 3, "v1.5"; output channels 4 planes).  Shortcut: downsample.0 (1 x 1, the block's stride) and
 * downsample.1 (batch norm) exactly when stride != 1 or in != out.  A block ends relu((branch + shift) + shortcut), in that order.
 * Tail: the mean over the pixels, then fc with bias.  Batch norms use the running statistics, eps 1e-5, and are all folded into
 * the convolution in front of them at pack time, in fp64, rounded once.  fp32 NHWC activations, every convolution the fp32-MFMA
 * implicit GEMM (a k-ordered fp32 fma chain).  Every sum has one fixed order: an image's stage maps, pooled vector and logits are
 * bit-identical whatever B it sits in and wherever it sits in the batch.  No atomics; nothing of a workspace is read before it
 * is written.  Added without a change of USPACE_ABI_VERSION: symbols only.
 * ------------------------------------------------------------------------------------- */
/* (struct-then-typedef, as uspace_idnet_config; the binding is uspace_amd/_hip.py ResnetConfig) */
struct uspace_resnet_config {
    int stem;        /* conv1 output channels (64) */
    int planes[4];   /* 64, 128, 256, 512 */
    int blocks[4];   /* 2,2,2,2 | 3,4,6,3 | ...; each >= 1 */
    int bottleneck;  /* 0: BasicBlock (expansion 1), 1: Bottleneck (expansion 4, stride on the 3 x 3: "v1.5") */
    int num_outputs; /* fc rows, >= 1 */
};
typedef struct uspace_resnet_config uspace_resnet_config;

/* parameter tensors in the module's state_dict order with the num_batches_tracked buffers dropped; a batch norm is weight, bias,
 * running_mean, running_var: conv1.weight [stem, 3, 7, 7], bn1.*; per block layerL.i: conv1.weight, bn1.*, conv2.weight, bn2.*
 * (Bottleneck: conv3.weight, bn3.* too), then downsample.0.weight [out, in, 1, 1] and downsample.1.* where the block has them;
 * fc.weight [num_outputs, F], fc.bias, F = planes[3] (x 4 for Bottleneck).  Every channel count (stem, planes, 4 planes) must be
 * a multiple of 4 and at most 2048; any H, W from 32 to 16384.  An invalid config gives USPACE_ERR_ARG (-1 from param_numel) / 0
 * bytes; B outside 1 .. 32767, H or W outside their range, or a tensor of 2^31 elements or more likewise. */
USPACE_API int uspace_resnet_num_params(const uspace_resnet_config* cfg);
USPACE_API long uspace_resnet_param_numel(const uspace_resnet_config* cfg, int index);
USPACE_API size_t uspace_resnet_weight_bytes(const uspace_resnet_config* cfg);
USPACE_API size_t uspace_resnet_workspace_bytes(const uspace_resnet_config* cfg, int B, int H, int W);
USPACE_API int uspace_resnet_pack_weights(const uspace_resnet_config* cfg, const float* const* params, int n_params, void* blob,
                                          size_t blob_bytes, uspace_stream_t stream);
/* x: fp32 NCHW [B, 3, H, W] in [0, 1] -> out: fp32 NHWC [B, H, W, 3], (x - mean_c) / std_c; mean and std are HOST arrays of 3
 * floats (ImageNet's 0.485, 0.456, 0.406 and 0.229, 0.224, 0.225 for the usual classifiers), std positive and finite.  Not folded
 * into conv1: the network zero-pads the normalised image. */
USPACE_API int uspace_resnet_preprocess(const float* x, int B, int H, int W, const float* mean, const float* std, float* out,
                                        uspace_stream_t stream);
/* x_nhwc: fp32 [B, H, W, 3] (uspace_resnet_preprocess's output) -> logits fp32 [B, num_outputs]; pooled fp32 [B, F] or NULL */
USPACE_API int uspace_resnet_forward(const uspace_resnet_config* cfg, const void* blob, void* workspace, size_t workspace_bytes,
                                     const float* x_nhwc, int B, int H, int W, float* pooled, float* logits, uspace_stream_t stream);
/* Test aid: stage 0 = the stem after the max pool, 1 + u = block u's output (NHWC fp32 [B, h, w, c]), 1 + (number of blocks) =
 * the pooled vector fp32 [B, F].  Nothing after the stage runs. */
USPACE_API int uspace_resnet_tap(const uspace_resnet_config* cfg, const void* blob, void* workspace, size_t workspace_bytes,
                                 const float* x_nhwc, int B, int H, int W, int stage, float* dump, uspace_stream_t stream);
/* The effect of an attribute edit from the classifier's logits za (original) and zb (edit), fp32 [B, A]; target int [B] (the
 * edited attribute of each pair), sign fp32 [B] (the intended direction), sigma fp32 [A] (per-attribute logit standard deviation)
 * or NULL for ones; all device pointers.  One thread per pair, fp64, in attribute order, d = zb - za:
 * out [B, 4] = { sign d_t,  1 if sign zb_t > 0 else 0,  mean over j != t of |d_j| / sigma_j (0 if A == 1),
 * |d_t| / sigma_t over (that + the sum over j != t of |d_j| / sigma_j), 0 where nothing moved }.  A target outside 0 .. A - 1
 * gives that pair four NaNs. */
USPACE_API int uspace_attr_effect_f64(const float* za, const float* zb, const int* target, const float* sign, const float* sigma,
                                      int B, int A, double* out, uspace_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Segmentation operators and the pair reductions of the segmentation-consistency metric (uspace_amd/tools/seg_metrics.py;
 * csrc/segformer.hip).  No workspace, no floating-point atomics; every output element has one thread, every pair one workgroup and
 * one summation order, so a result is bit-identical whatever batch it sits in.  All pointers are device pointers.  Sides (h, w, H,
 * W, Ho, Wo) are 1 .. 16384, label counts L 1 .. 256; anything else gives USPACE_ERR_ARG.  Added without a change of
 * USPACE_ABI_VERSION: symbols only.
 * ------------------------------------------------------------------------------------- */
/* Attention with few resident keys and many queries (csrc/attention_kv.hip; SegFormer's spatially reduced attention): q bf16
 * [B, Lq, ldq] (head h in columns 64 h .. 64 h + 63), kv bf16 [B, Lk, ldkv] (k of head h in columns 64 h .., v in columns
 * 64 (H + h) ..), out bf16 [B, Lq, ldo].  Head dim 64, softmax of q.k / 8 over the Lk keys, 1 <= Lk <= 336, any Lq >= 1.  K and V
 * of a (sample, head) are staged once per workgroup; the queries are cut into chunks of whole 16-row tiles, one workgroup each.
 * A row's arithmetic is uspace_attention_bf16's (fp32 softmax, P rounded once to bf16, row sum by the all-ones MFMA) and its bits do
 * not depend on the chunking or on its place in the batch.  ldq, ldkv multiples of 8, ldo of 4, q and kv 16-byte aligned.
 * uspace_attention_kv_plan: what the launch uses, out[7] = {key tiles compiled for, waves per workgroup, query tiles per chunk,
 * chunks per (sample, head), grid, block, LDS bytes}; the chunk rule is reasoned, not measured (see the file's head). */
USPACE_API int uspace_attention_kv_plan(int B, int Lq, int Lk, int H, int* out);
USPACE_API int uspace_attention_kv_bf16(const uint16_t* q, int ldq, const uint16_t* kv, int ldkv, uint16_t* out, int ldo, int B, int Lq,
                                        int Lk, int H, uspace_stream_t stream);
/* y = GELU(depthwise 3 x 3 convolution of x + bias), zero padding 1: x, y bf16 NHWC [B, H, W, C] (y != x), w fp32 [9][C] with tap
 * ty * 3 + tx reading pixel (y + ty - 1, x + tx - 1), bias fp32 [C].  fp32: acc = bias, then one fma per tap in (ty, tx) order, taps
 * outside the map left out; the erf-GELU of the GEMM epilogue; one rounding to bf16.  C a multiple of 8, pointers 16-byte aligned. */
USPACE_API int uspace_dwconv3x3_gelu_bf16(const uint16_t* x, const float* w, const float* bias, uint16_t* y, int B, int H, int W,
                                          int C, uspace_stream_t stream);
/* Bilinear resampling, align_corners = False (torch.nn.functional.interpolate): x fp32 NHWC [B, h, w, C] -> channels coff ..
 * coff + C - 1 of y, fp32 [B, Ho, Wo, ldo]: a concatenation is written in place.  The source coordinate ((2 d + 1) in - out) /
 * (2 out), clamped at 0, is split into tap and weight in integers; in == out copies. */
USPACE_API int uspace_bilinear_nhwc_f32(const float* x, int B, int h, int w, int C, float* y, int Ho, int Wo, int ldo, int coff,
                                        uspace_stream_t stream);
/* labels uint8 [B, H, W] = argmax over the L channels of logits fp32 NHWC [B, h, w, L] resampled to H x W by the arithmetic of
 * uspace_bilinear_nhwc_f32 (bit for bit), the lowest index on ties; a NaN never wins.  The resampled logits are not stored. */
USPACE_API int uspace_seg_labels_u8(const float* logits, int B, int h, int w, int L, uint8_t* labels, int H, int W,
                                    uspace_stream_t stream);
/* counts int32 [B, 3, L] of two label maps la, lb uint8 [B, npx]: pixels of each label in a, in b, and in both at once.  Labels
 * >= L are counted nowhere.  B <= 65535, npx < 2^31. */
USPACE_API int uspace_seg_pair_counts(const uint8_t* la, const uint8_t* lb, int B, long npx, int L, int* counts,
                                      uspace_stream_t stream);
/* out fp64 [B, 2] = { sum of (img_a - img_b)^2 over the 3 channels, number of pixels } over the pixels whose label is in the set
 * `member` (uint8 [L], nonzero = in the set) in NEITHER map; images fp32 NCHW [B, 3, H, W], la, lb uint8 [B, H, W].  Differences
 * and sum in fp64 in one fixed order.  Labels >= L are in no set. */
USPACE_API int uspace_seg_region_sse_f64(const float* img_a, const float* img_b, const uint8_t* la, const uint8_t* lb,
                                         const uint8_t* member, int L, int B, int H, int W, double* out, uspace_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * SegFormer (uspace_amd/libs/segformer.py; csrc/segformer.hip): Hugging Face SegformerForSemanticSegmentation in eval mode, the
 * MiT encoder of four stages with the all-MLP decode head.  Stage i: overlapping patch embedding (convolution 7 x 7 stride 4
 * padding 3 for stage 0, 3 x 3 stride 2 padding 1 after, with bias) and LayerNorm; depths[i] blocks x += o_proj(attn(LN1 x)),
 * x += fc2(GELU(dwconv3x3(fc1(LN2 x)))), where q = q_proj(LN1 x) and k, v are linear maps of LN1 x reduced by a convolution of
 * kernel = stride = sr[i] without padding and LayerNormed (sr[i] == 1: of LN1 x itself), softmax of q.k / 8; a LayerNorm closes
 * the stage.  Head: per-stage Linear hidden[i] -> decoder_dim, bilinear resize (align_corners = False) to the stage-0 map,
 * concatenation in reversed stage order, 1 x 1 convolution without bias + BatchNorm (running statistics) + ReLU, 1 x 1 classifier.
 * Convolutions and the head run in fp32 (fp32 MFMA), the five linears of a block on uspace_gemm_bf16 with the residual stream in
 * fp32.  A sample's maps and logits are bit-identical whatever B it sits in and wherever it sits in the batch.  Added without a
 * change of USPACE_ABI_VERSION: symbols only.
 * ------------------------------------------------------------------------------------- */
/* (struct-then-typedef, as uspace_resnet_config; the binding is uspace_amd/_hip.py SegformerConfig) */
struct uspace_segformer_config {
    int hidden[4];    /* C_i: multiples of 64, at most 2048 */
    int depths[4];    /* blocks per stage, each >= 1 */
    int heads[4];     /* heads[i] * 64 == hidden[i]: head dim 64 only (MiT-B0 has 32) */
    int sr[4];        /* 8, 4, 2, 1 in every published model; 1 .. 16 */
    int mlp[4];       /* Mix-FFN width over hidden[i], 1 .. 8 */
    int decoder_dim;  /* D: a multiple of 4, at most 2048 */
    int num_labels;   /* 1 .. 256 */
    float eps_embed;  /* the patch embeddings' LayerNorm */
    float eps_block;  /* layernorm_before / layernorm_after */
    float eps_sr;     /* the sequence reduction's LayerNorm */
    float eps_stage;  /* the LayerNorm that closes a stage */
    float eps_bn;     /* the head's BatchNorm */
};
typedef struct uspace_segformer_config uspace_segformer_config;

/* parameter tensors in the module's state_dict order with num_batches_tracked dropped.  Per stage: patch_embeddings.proj.{weight,
 * bias}, patch_embeddings.layer_norm.*; per block layernorm_before.*, attention.{q_proj, k_proj, v_proj, o_proj}.{weight, bias},
 * attention.sequence_reduction.sequence_reduction.{weight, bias} and .layer_norm.* (only where sr > 1), layernorm_after.*,
 * mlp.fc1.*, mlp.dwconv.dwconv.{weight [4C, 1, 3, 3], bias}, mlp.fc2.*; the stage's layer_norm.*.  Then decode_head.
 * linear_projections.i.proj.*, linear_fuse.weight, batch_norm.{weight, bias, running_mean, running_var}, classifier.*.
 * An invalid config gives USPACE_ERR_ARG (-1 from param_numel) / 0 bytes.  H and W from 32 to 16384; every reduced key map at most
 * 336 positions (images up to about 576^2 with the published sr); B 1 .. 32767; otherwise USPACE_ERR_ARG / 0 bytes. */
USPACE_API int uspace_segformer_num_params(const uspace_segformer_config* cfg);
USPACE_API long uspace_segformer_param_numel(const uspace_segformer_config* cfg, int index);
USPACE_API size_t uspace_segformer_weight_bytes(const uspace_segformer_config* cfg);
USPACE_API size_t uspace_segformer_workspace_bytes(const uspace_segformer_config* cfg, int B, int H, int W);
USPACE_API int uspace_segformer_pack_weights(const uspace_segformer_config* cfg, const float* const* params, int n_params, void* blob,
                                             size_t blob_bytes, uspace_stream_t stream);
/* x_nhwc: fp32 [B, H, W, 3], normalised (uspace_resnet_preprocess's output) -> logits fp32 NHWC [B, h, w, num_labels] at the
 * stage-0 map h = (H - 1) / 4 + 1, w = (W - 1) / 4 + 1 */
USPACE_API int uspace_segformer_forward(const uspace_segformer_config* cfg, const void* blob, void* workspace, size_t workspace_bytes,
                                        const float* x_nhwc, int B, int H, int W, float* logits, uspace_stream_t stream);
/* Test aid.  Stages in order, all fp32 NHWC: per encoder stage the patch embedding after its LayerNorm, every block's output,
 * the stage's closing LayerNorm ([B, h_i, w_i, hidden[i]]); then the concatenation [B, h_0, w_0, 4 D], the fused map
 * [B, h_0, w_0, D], the logits.  uspace_segformer_num_stages counts them.  Nothing after the stage runs. */
USPACE_API int uspace_segformer_num_stages(const uspace_segformer_config* cfg);
USPACE_API int uspace_segformer_tap(const uspace_segformer_config* cfg, const void* blob, void* workspace, size_t workspace_bytes,
                                    const float* x_nhwc, int B, int H, int W, int stage, float* dump, uspace_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Local edits (uspace_amd/tools/local_edit.py, CNF.decode_local; csrc/local_edit.hip): the velocity blend of a paired solve and
 * the masks it takes.  Enqueued on `stream`; no atomics, every sum in one fixed order, a sample's result bit-identical whatever
 * batch it sits in.  All pointers are device pointers.  Added without a change of USPACE_ABI_VERSION: symbols only.
 * ------------------------------------------------------------------------------------- */
/* pair fp32 [2B, C, cells], source rows first; mask fp32 [B, cells], broadcast over C.  out rows [0, B) = the source rows as they
 * are; row B + b per element, with s = pair[b], e = pair[B + b], m = mask[b, p]: m <= 0 or NaN -> s, m >= 1 -> e (both bit for
 * bit), otherwise fmaf(m, e - s, s).  out == pair (in place) or disjoint from it.  16-byte accesses where cells % 4 == 0 and the
 * three pointers are 16-byte aligned, a scalar form otherwise. */
USPACE_API int uspace_pair_blend(const float* pair, const float* mask, int B, int C, long cells, float* out, uspace_stream_t stream);
/* mask fp32 [B, S, S] from label maps uint8 [B, H, W] and the set `member` (uint8 [256], nonzero = in the region); H and W
 * multiples of S, S 1 .. 64, sides up to 16384.  Per cell share = (float)count / (float)(H/S * W/S), count the member pixels of
 * the cell (an integer); v = the maximum of share over the (2 dilate + 1)^2 window of cells clipped at the border, dilate 0 .. 4;
 * soft != 0 stores v, otherwise v > thr ? 1 : 0. */
USPACE_API int uspace_mask_from_labels(const uint8_t* labels, int B, int H, int W, const uint8_t* member, int S, int dilate, float thr,
                                       int soft, float* mask, uspace_stream_t stream);
/* mask fp32 [R, G * patch, G * patch] from maps fp32 [n_blocks, R, G * G, nk] (uspace_uvit_forward_maps' image x context window),
 * block_w fp32 [n_blocks] and cols fp32 [R, nk].  Per row r: a[p] = sum_blk block_w[blk] * (sum_j cols[r, j] * maps[blk, r, p, j])
 * in fp32, blocks ascending, columns ascending, one fused multiply-add per term from 0 (terms of a block or a column of weight 0
 * are left out); the 3 x 3 maximum over the G x G grid clipped at the border; divided by the row's maximum; soft != 0 stores that,
 * otherwise > thr ? 1 : 0; every token cell goes to its patch x patch cells.  A row whose maximum is not above 0 is all 0.
 * G 1 .. 64, patch 1 .. 16. */
USPACE_API int uspace_mask_from_maps(const float* maps, int n_blocks, int R, int G, int nk, const float* block_w, const float* cols,
                                     int patch, float thr, int soft, float* mask, uspace_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Measurement aid (bench.py): record HIP events, on the launching stream, around every
 * uspace_gemm_bf16 launch whose (epi_flags, N, K) match, up to max_launches; _end() waits for
 * the recorded events and returns their summed duration.  Off unless _begin() was called.
 * ------------------------------------------------------------------------------------- */
USPACE_API int uspace_prof_gemm_begin(int epi_flags, int N, int K, int max_launches);
USPACE_API int uspace_prof_gemm_end(double* total_ms, int* n_launches);
/* The same around EVERY GEMM and attention launch (bench.py's roofline_all): _end() aggregates the recorded launches by
 * (kind, flags, M, N, K) into keys[6 * i + {0: kind (0 GEMM, 1 attention), 1: epi_flags (attention: 1 = key scales, 2 = the streaming form
 * uspace_attention_long_bf16, 4 = the wide single-head form uspace_attention_wide_bf16, whose M is B and whose K is C),
 * 2: M (attention: B * H), 3: N (attention: L), 4: K (attention: head dim), 5: launches}] and total_ms[i], i < *n_records <= max_records. */
USPACE_API int uspace_prof_all_begin(int max_launches);
USPACE_API int uspace_prof_all_end(int* keys, double* total_ms, int max_records, int* n_records);
/* Launches that matched but found the recorder full (max_launches reached) since the last _begin(): a recording is complete
 * only if this is 0 (bench.py fails otherwise instead of pricing a truncated solve). */
USPACE_API long uspace_prof_dropped(void);

/* What this box reaches on the two rooflines (synchronous, self-timed with HIP events, own scratch; host pointers out):
 * dense bf16 MFMA rate of an MFMA-only loop on every SIMD (TFLOP/s), and a device-to-device float4 stream copy
 * (read + written bytes per second, GB/s) over `bytes` (>= 1 MiB) repeated `reps` times. */
USPACE_API int uspace_prof_mfma_peak(int iters, double* tflops);
/* ... and the shader clock the chip sustained under that load (GHz; s_memtime ticks of one workgroup / wall time) */
USPACE_API int uspace_prof_mfma_peak_clock(int iters, double* tflops, double* shader_ghz);
/* The two above loop over v_mfma_f32_32x32x16_bf16 on near-constant operands: the burst figure.  This one runs the GEMM's own
 * instruction, v_mfma_f32_16x16x32_bf16, on pseudo-random operands in [-1, 1): what the matrix pipe sustains on data that toggles
 * like real activations (the chip is power-limited there; ABI 10). */
USPACE_API int uspace_prof_mfma_peak_gemm_op(int iters, double* tflops, double* shader_ghz);
USPACE_API int uspace_prof_hbm_copy(size_t bytes, int reps, double* gb_per_s);

#ifdef __cplusplus
}
#endif
#endif /* USPACE_HIP_H */
