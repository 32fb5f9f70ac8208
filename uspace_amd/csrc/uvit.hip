// Whole-forward orchestration of the U-ViT velocity network on one MI355X:
//   nnet(x, timesteps, ...) of the reference (libs/uvit.py:306-351, libs/uvit_t2i.py:308-342)
// as a fixed sequence of gfx950 kernels on the caller's stream.  No allocation, no sync:
// the caller provides the packed-weights blob and a workspace sized by
// uspace_uvit_workspace_bytes(); the sequence is hipGraph-capturable.
#include <atomic>
#include <cstring>
#include <memory>
#include <mutex>
#include <vector>

#include "blob.h"

namespace {

struct BlockIdx {
    int skip_w = -1, skip_b = -1;
    int n1w, n1b, qkv, projw, projb, n2w, n2b, fc1w, fc1b, fc2w, fc2b;
    // derived at pack time for the LayerNorm-folded path (not parameters): gamma-folded weights, beta-folded biases,
    // column sums of the folded bf16 weights
    int qkv_f, qkv_fb, qkv_cs, fc1_f, fc1_fb, fc1_cs;
    int skip_cs2 = -1;   // out-blocks: row sums of bf16(skip_linear.weight[:, D:]) -- the skip slab is stored centred (uspace_uvit_forward)
};

struct Model {
    ParamTable lay;
    int pos, pw, pb, cw = -1, cb = -1;
    std::vector<BlockIdx> blk;
    int ng, nb, dw, db, convw, convb;
    int head_img;        // derived: the output head's weight image (rowops.hip head_weight_image)
    int L, extras, npatch, nblocks;
};

bool valid_cfg(const uspace_uvit_config* c) {
    if (!c) return false;
    if (c->img_size <= 0 || c->patch_size <= 0 || c->img_size % c->patch_size) return false;
    if (c->in_chans <= 0 || c->in_chans * c->patch_size * c->patch_size > 16) return false;
    if (c->embed_dim <= 0 || c->embed_dim % 64 || c->num_heads * 64 != c->embed_dim) return false;
    if (c->embed_dim > 2048) return false;           // the output head keeps its weight image in LDS (rowops.hip, us_head_pack)
    if (c->depth <= 0 || (c->depth & 1)) return false;
    if (c->mlp_hidden <= 0 || c->mlp_hidden % 64) return false;
    if (c->n_extra < 0 || c->clip_dim < 0 || (c->clip_dim % 64)) return false;
    if (c->clip_dim > 0 && c->n_extra == 0) return false;
    return true;
}

// Canonical parameter order (documented in include/uspace_hip.h).
Model build_model(const uspace_uvit_config& c) {
    Model m;
    const long D = c.embed_dim, Hd = c.mlp_hidden;
    const int g = c.img_size / c.patch_size;
    m.npatch = g * g;
    m.extras = 1 + c.n_extra;
    m.L = m.extras + m.npatch;
    m.pos = m.lay.add((long)m.L * D, P_F32);
    m.pw = m.lay.add(D * c.in_chans * c.patch_size * c.patch_size, P_F32);
    m.pb = m.lay.add(D, P_F32);
    if (c.clip_dim > 0) {
        m.cw = m.lay.add(D * c.clip_dim, P_BF16);
        m.cb = m.lay.add(D, P_F32);
    }
    const int half = c.depth / 2;
    m.nblocks = c.depth + 1;
    for (int i = 0; i < m.nblocks; ++i) {
        BlockIdx b;
        if (i > half) {
            b.skip_w = m.lay.add(D * 2 * D, P_BF16);
            b.skip_b = m.lay.add(D, P_F32);
        }
        b.n1w = m.lay.add(D, P_F32);
        b.n1b = m.lay.add(D, P_F32);
        b.qkv = m.lay.add(3 * D * D, P_BF16);
        b.projw = m.lay.add(D * D, P_BF16);
        b.projb = m.lay.add(D, P_F32);
        b.n2w = m.lay.add(D, P_F32);
        b.n2b = m.lay.add(D, P_F32);
        b.fc1w = m.lay.add(Hd * D, P_BF16);
        b.fc1b = m.lay.add(Hd, P_F32);
        b.fc2w = m.lay.add(D * Hd, P_BF16);
        b.fc2b = m.lay.add(D, P_F32);
        m.blk.push_back(b);
    }
    m.ng = m.lay.add(D, P_F32);
    m.nb = m.lay.add(D, P_F32);
    const long PD = (long)c.patch_size * c.patch_size * c.in_chans;
    m.dw = m.lay.add(PD * D, P_F32);
    m.db = m.lay.add(PD, P_F32);
    m.convw = m.lay.add((long)c.in_chans * c.in_chans * 9, P_F32);
    m.convb = m.lay.add(c.in_chans, P_F32);
    m.lay.derived = true;   // from here on: tensors uspace_uvit_pack_weights computes
    for (BlockIdx& b : m.blk) {
        b.qkv_f = m.lay.add(3 * D * D, P_BF16);
        b.qkv_fb = m.lay.add(3 * D, P_F32);
        b.qkv_cs = m.lay.add(3 * D, P_F32);
        b.fc1_f = m.lay.add(Hd * D, P_BF16);
        b.fc1_fb = m.lay.add(Hd, P_F32);
        b.fc1_cs = m.lay.add(Hd, P_F32);
        if (b.skip_w >= 0) b.skip_cs2 = m.lay.add(D, P_F32);
    }
    m.head_img = m.lay.add((long)us_head_image_floats((int)D), P_F32);
    return m;
}

struct Workspace {
    size_t x, xb, h, qkv, f, skips, ctx_bf, ctx_f32, head, xc, part, cbuf, cskip, splitk, splitk_bytes, sk, sk_bytes, skcnt, skcnt_bytes, total;
};
// GEMM launches of one forward that may take the in-launch K-split tail: each gets its own 256 arrival counters, zeroed by ONE
// memset at the start of the forward (include/uspace_hip.h, uspace_gemm_ext.sk_counters)
inline int sk_launches(const uspace_uvit_config& c) { return 5 * (c.depth + 1) + c.depth / 2 + 2; }

// sk_on: the K-split tail switch (uspace_gemm_set_sk) as the caller read it
Workspace plan_workspace(const uspace_uvit_config& c, const Model& m, int B, bool sk_on) {
    Workspace w;
    const size_t M = (size_t)B * m.L, D = c.embed_dim;
    Arena a;
    w.x = a.take(M * D * 4);
    w.xb = a.take(M * D * 2);
    w.h = a.take(M * D * 2);
    w.qkv = a.take(M * 3 * D * 2);
    w.f = a.take(M * (size_t)c.mlp_hidden * 2);
    w.skips = a.take((size_t)(c.depth / 2) * M * D * 2);
    w.ctx_bf = a.take(c.clip_dim > 0 ? (size_t)B * c.n_extra * c.clip_dim * 2 : 0);
    w.ctx_f32 = a.take(c.clip_dim > 0 ? (size_t)B * c.n_extra * D * 4 : 0);
    w.head = a.take((size_t)B * c.in_chans * c.img_size * c.img_size * 4);
    w.xc = a.take(M * D * 2);                          // LayerNorm folding: centred bf16 copy of the residual stream
    w.part = a.take(M * (size_t)us_cdiv((int)D, 64) * 2 * 4);    // per-row partial sums, one slot per producer N tile (64 columns at the least)
    w.cbuf = a.take(M * 4);                            // per-row centring constants (row means at the last norm)
    w.cskip = a.take((size_t)(c.depth / 2) * M * 4);   // ... of the centred copies kept on the long-skip stack, one per in-block
    // fp32 partial sums of the K-split form the GEMM uses for small batches (proj, skip_linear, fc2: N = D)
    w.splitk_bytes = std::max(std::max(uspace_gemm_split_ws_bytes((int)M, (int)D, (int)D), uspace_gemm_split_ws_bytes((int)M, (int)D, 2 * (int)D)),
                              uspace_gemm_split_ws_bytes((int)M, (int)D, c.mlp_hidden));
    w.splitk = a.take(w.splitk_bytes);
    // partial-sum slabs of the in-launch K-split tail (qkv; proj, skip_linear, fc2: N = D) and the launches' arrival counters
    auto sk_ws = [&](size_t n, size_t k) { return us_gemm_sk_ws_bytes((int)M, (int)n, (int)k, sk_on); };
    w.sk_bytes = std::max(std::max(sk_ws(D, D), sk_ws(D, 2 * D)), std::max(sk_ws(D, c.mlp_hidden), sk_ws(3 * D, D)));
    w.sk_bytes = std::max(w.sk_bytes, sk_ws(c.mlp_hidden, D));
    w.sk = a.take(w.sk_bytes);
    w.skcnt_bytes = w.sk_bytes ? (size_t)sk_launches(c) * USPACE_GEMM_SK_COUNTERS * 4 : 0;
    w.skcnt = a.take(w.skcnt_bytes);
    w.total = a.off;
    return w;
}

}  // namespace

extern "C" int uspace_uvit_num_params(const uspace_uvit_config* cfg) {
    if (!valid_cfg(cfg)) return USPACE_ERR_ARG;
    return build_model(*cfg).lay.n_params;
}

extern "C" long uspace_uvit_param_numel(const uspace_uvit_config* cfg, int index) {
    if (!valid_cfg(cfg)) return USPACE_ERR_ARG;
    return build_model(*cfg).lay.numel(index);
}

extern "C" size_t uspace_uvit_weight_bytes(const uspace_uvit_config* cfg) {
    if (!valid_cfg(cfg)) return 0;
    return build_model(*cfg).lay.bytes();
}

extern "C" size_t uspace_uvit_workspace_bytes(const uspace_uvit_config* cfg, int B) {
    if (!valid_cfg(cfg) || B <= 0) return 0;
    const Model m = build_model(*cfg);
    return plan_workspace(*cfg, m, B, uspace_gemm_get_sk() != 0).total;
}

extern "C" int uspace_uvit_pack_weights(const uspace_uvit_config* cfg, const float* const* params, int n_params,
                                        void* blob, size_t blob_bytes, uspace_stream_t stream) {
    if (!valid_cfg(cfg)) return USPACE_ERR_ARG;
    const Model m = build_model(*cfg);
    US_TRY(us_pack_table(m.lay, params, n_params, blob, blob_bytes, stream));
    hipStream_t s = (hipStream_t)stream;
    // LayerNorm folding: W' = bf16(W * gamma), bias' = bias + W beta, column sums of W' (qkv has no bias of its own)
    const int D = cfg->embed_dim, Hd = cfg->mlp_hidden;
    auto at = [&](int idx) { return (char*)blob + m.lay.p[idx].offset; };
    for (const BlockIdx& b : m.blk) {
        US_TRY(uspace_fold_layernorm(params[b.qkv], params[b.n1w], params[b.n1b], nullptr, (uint16_t*)at(b.qkv_f),
                                     (float*)at(b.qkv_fb), (float*)at(b.qkv_cs), 3 * D, D, stream));
        US_TRY(uspace_fold_layernorm(params[b.fc1w], params[b.n2w], params[b.n2b], params[b.fc1b], (uint16_t*)at(b.fc1_f),
                                     (float*)at(b.fc1_fb), (float*)at(b.fc1_cs), Hd, D, stream));
        if (b.skip_cs2 >= 0) US_TRY(us_rowsum_bf16(params[b.skip_w], 2 * D, D, D, (float*)at(b.skip_cs2), D, s));
    }
    return us_head_pack(params[m.ng], params[m.nb], params[m.dw], params[m.db], cfg->patch_size * cfg->patch_size * cfg->in_chans, D,
                        (float*)at(m.head_img), s);
}

namespace {
// Process-wide switch (documented in the header's global-state note): LayerNorm folded through the GEMMs (default) or
// separate LayerNorm launches.  No environment variable is read here; the Python binding forwards USPACE_LN_FOLD.
std::atomic<int> g_ln_fold{1};

// Derived per-configuration layout (parameter offsets in the blob): built once per distinct configuration.
std::mutex g_model_mu;
std::vector<std::pair<uspace_uvit_config, std::shared_ptr<const Model>>> g_models;
std::shared_ptr<const Model> model_for(const uspace_uvit_config& c) {
    std::lock_guard<std::mutex> lock(g_model_mu);
    for (const auto& e : g_models)
        if (memcmp(&e.first, &c, sizeof(c)) == 0) return e.second;
    if (g_models.size() >= 16) g_models.erase(g_models.begin());
    g_models.emplace_back(c, std::make_shared<const Model>(build_model(c)));
    return g_models.back().second;
}
}  // namespace

extern "C" int uspace_uvit_set_ln_fold(int mode) {
    if (mode < -1 || mode > 1) return USPACE_ERR_ARG;
    g_ln_fold.store(mode < 0 ? 1 : mode);
    return USPACE_OK;
}

extern "C" int uspace_uvit_get_ln_fold(void) { return g_ln_fold.load(); }

namespace {
// The forward; stop_after >= 0 (uspace_uvit_forward_tap) copies the residual stream x to `dump` after stage stop_after and
// returns there (the last stage, depth + 1, runs the head first).  stop_after = -1 is the product forward: the launch sequence
// is the same for every stop_after up to the stop.  maps != NULL (uspace_uvit_forward_maps): one more launch per block, the head-mean
// attention map of the window mw = {q0, nq, k0, nk} right after the block's qkv GEMM; with maps == NULL the launch sequence is
// the product forward's.
// pair != NULL (uspace_uvit_forward_cfg): io describes Bs samples and the forward runs over B = 2 Bs rows -- row b is (x[b], t[b],
// context[b]), row Bs + b is (x[b], t[b], uncond[b or 0]) -- with the launch sequence of a plain forward at batch 2 Bs, except that the
// context cast and the token embedding are issued per half, each reading its own rows in place; the head writes pair->pred
// ([2 Bs, C, S, S]) instead of io->out.
struct MapWindow { int q0, nq, k0, nk; };
struct PairArgs { const float* uncond; bool batched; float* pred; };
struct ForwardOpts {             // what the exported forms add to the product forward; each fills only what it uses
    int stop_after = -1;
    float* dump = nullptr;
    float* maps = nullptr;
    MapWindow mw{0, 0, 0, 0};
    const PairArgs* pair = nullptr;
};
int forward_impl(const uspace_uvit_config* cfg, const void* blob, void* workspace, size_t workspace_bytes, const uspace_uvit_io* io,
                 int Bs, uspace_stream_t stream, const ForwardOpts& opt) {
    if (!valid_cfg(cfg) || !blob || !workspace || !io || Bs <= 0) return USPACE_ERR_ARG;
    const int stop_after = opt.stop_after;
    float* const dump = opt.dump;
    float* const maps = opt.maps;
    const MapWindow mw = opt.mw;
    const PairArgs* const pair = opt.pair;
    const int B = pair ? 2 * Bs : Bs;
    if (stop_after >= 0 && (!dump || stop_after > cfg->depth + 1)) return USPACE_ERR_ARG;
    if (!io->x || !io->t || !io->out) return USPACE_ERR_ARG;
    if (cfg->n_extra > 0 && !io->context) return USPACE_ERR_ARG;
    const uspace_uvit_config& c = *cfg;
    const std::shared_ptr<const Model> mp = model_for(c);
    const Model& m = *mp;
    // the K-split tail switch, read once: the workspace, the slot counts the consumers are told and every launch follow this reading
    const bool sk_on = uspace_gemm_get_sk() != 0;
    const Workspace w = plan_workspace(c, m, B, sk_on);
    if (workspace_bytes < w.total) return USPACE_ERR_WORKSPACE;

    const int D = c.embed_dim, Hd = c.mlp_hidden, L = m.L, H = c.num_heads;
    const int M = B * L;
    if (maps && (mw.q0 < 0 || mw.nq < 1 || mw.q0 > L - mw.nq || mw.k0 < 0 || mw.nk < 1 || mw.k0 > L - mw.nk)) return USPACE_ERR_ARG;
    const size_t map_stride = maps ? (size_t)B * mw.nq * mw.nk : 0;      // floats per block
    const char* wb = (const char*)blob;
    char* ws = (char*)workspace;
    auto PF = [&](int idx) { return (const float*)(wb + m.lay.p[idx].offset); };
    auto PH = [&](int idx) { return (const uint16_t*)(wb + m.lay.p[idx].offset); };
    float* x = (float*)(ws + w.x);
    uint16_t* xb = (uint16_t*)(ws + w.xb);
    uint16_t* h = (uint16_t*)(ws + w.h);
    uint16_t* qkv = (uint16_t*)(ws + w.qkv);
    uint16_t* f = (uint16_t*)(ws + w.f);
    uint16_t* skips = (uint16_t*)(ws + w.skips);
    uint16_t* xc = (uint16_t*)(ws + w.xc);
    float* part = (float*)(ws + w.part);
    float* cbuf = (float*)(ws + w.cbuf);
    uspace_gemm_ext plain{};                          // no LayerNorm folding, only the K-split workspaces
    plain.split_ws = w.splitk_bytes ? ws + w.splitk : nullptr;
    plain.split_ws_bytes = w.splitk_bytes;
    // in-launch K-split tail: one slab workspace (launches of a stream run one after the other), a fresh set of zeroed counters per launch
    int sk_next = 0;
    if (w.sk_bytes) {
        if (hipMemsetAsync(ws + w.skcnt, 0, w.skcnt_bytes, (hipStream_t)stream) != hipSuccess) return USPACE_ERR_LAUNCH;
        plain.sk_ws = ws + w.sk;
        plain.sk_ws_bytes = w.sk_bytes;
    }
    const int sk_max = sk_launches(c);
    auto with_sk = [&](uspace_gemm_ext e) {           // e with this launch's counters
        if (w.sk_bytes && sk_next < sk_max) {
            e.sk_ws = ws + w.sk;
            e.sk_ws_bytes = w.sk_bytes;
            e.sk_counters = ws + w.skcnt + (size_t)(sk_next++) * USPACE_GEMM_SK_COUNTERS * 4;
        } else {
            e.sk_ws = nullptr; e.sk_ws_bytes = 0; e.sk_counters = nullptr;
        }
        return e;
    };
    uspace_gemm_ext sk_tmp;                           // (the call reads it before it returns)
    auto sk_ptr = [&](const uspace_gemm_ext& e) { sk_tmp = with_sk(e); return (const uspace_gemm_ext*)&sk_tmp; };
    const bool fold = g_ln_fold.load() != 0 && us_gemm_part_slots_k(M, D, 64, sk_on) <= 8;   // consumers read <= 8 partial slots per row
    const size_t MD = (size_t)M * D;

    constexpr int B_ = USPACE_EPI_BIAS, G_ = USPACE_EPI_GELU, R_ = USPACE_EPI_RESIDUAL, F_ = USPACE_EPI_OUT_F32,
                  H_ = USPACE_EPI_OUT_BF16;

    // ---- tokens: [time | extra | patches] (+pos)  (libs/uvit.py:315-327; libs/uvit_t2i.py:309-324)
    const float* extra = nullptr;
    if (c.n_extra > 0) {
        if (c.clip_dim > 0) {
            uint16_t* cbf = (uint16_t*)(ws + w.ctx_bf);
            float* cf = (float*)(ws + w.ctx_f32);
            const long n = (long)Bs * c.n_extra * c.clip_dim;
            US_TRY(uspace_cast_f32_bf16(io->context, cbf, n, stream));
            if (pair && pair->batched) US_TRY(uspace_cast_f32_bf16(pair->uncond, cbf + n, n, stream));
            else if (pair) US_TRY(us_cast_bcast_f32_bf16(pair->uncond, cbf + n, (long)c.n_extra * c.clip_dim, Bs, (hipStream_t)stream));
            US_TRY(us_gemm_bf16_ext(cbf, c.clip_dim, nullptr, 0, c.clip_dim, PH(m.cw), c.clip_dim, B * c.n_extra, D,
                                    c.clip_dim, B_ | F_, PF(m.cb), nullptr, 0, cf, D, nullptr, 0, nullptr, sk_on, stream));
            extra = cf;
        } else {
            extra = io->context;
        }
    }
    if (!pair) {
        US_TRY(uspace_embed_tokens(io->x, io->t, io->t_stride, extra, c.n_extra, c.time_first, PF(m.pw), PF(m.pb),
                                   PF(m.pos), x, nullptr, B, c.in_chans, c.img_size, c.patch_size, D, stream));
    } else {
        // both halves read the same x and t; the unconditional half takes the second half of the embedded context (clip_dim > 0) or
        // the caller's unconditional tokens where they lie (one copy: stride 0)
        const long es = (long)c.n_extra * D;
        const float* extra_u = c.clip_dim > 0 ? extra + (size_t)Bs * es : pair->uncond;
        const long es_u = (c.clip_dim > 0 || pair->batched) ? es : 0;
        for (int half_i = 0; half_i < 2; ++half_i)
            US_TRY(us_embed_tokens_rows(io->x, io->t, io->t_stride, half_i ? extra_u : extra, c.n_extra, half_i ? es_u : es, c.time_first,
                                        PF(m.pw), PF(m.pb), PF(m.pos), x + (size_t)half_i * Bs * L * D, nullptr, Bs, B, c.in_chans,
                                        c.img_size, c.patch_size, D, (hipStream_t)stream));
    }
    auto tap = [&]() {
        return hipMemcpyAsync(dump, x, MD * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream) == hipSuccess ? USPACE_OK : USPACE_ERR_LAUNCH;
    };
    if (stop_after == 0) return tap();

    const int half = c.depth / 2;
    // The two LayerNorm modes differ in how "norm then GEMM" is issued for qkv and fc1 and in what the producers of x get.
    // Separate: a LayerNorm launch into h, then a plain GEMM; the producers write x and, where a later GEMM reads it, its bf16 copy.
    // Folded through the GEMMs (include/uspace_hip.h, uspace_gemm_ext): every producer of x that a norm follows (skip_linear, proj,
    // fc2 of the in-blocks) also leaves a centred bf16 copy and per-row partial sums; qkv and fc1 read that copy with gamma-folded
    // weights and finish the normalisation in their epilogues.  No LayerNorm launch except the first centring pass; the residual
    // stream x itself is unchanged (fp32).
    // The long skips are then kept as the CENTRED bf16 copies the in-blocks' fc2 writes for the next norm anyway (round 4: the raw bf16
    // copy beside it was one more 2 M D-byte store per in-block): in-block i's fc2 centres by cskip[i] -- the row means its own
    // fc1 published there instead of into cbuf -- and writes straight into skip slot i, which is also what the next block's qkv
    // reads.  skip_linear(cat([x, skip])) = x W1^T + (skip_c + cskip) W2^T: the second term's constant part is the rank-1 epilogue
    // term cskip[m] * rowsum(W2)[n] (USPACE_EPI_RANK1; libs/uvit.py:158-159).
    constexpr int C_ = USPACE_EPI_CEN_OUT, L_ = USPACE_EPI_LN_IN, K_ = USPACE_EPI_RANK1;
    float* const cskip = (float*)(ws + w.cskip);
    int slots_skip = 0, slots_proj = 0, slots_fc2 = 0;   // partial-sum slots per row of each producer (the 64-wide tile form of short-K launches writes more of them)
    int np = 1;                                   // partial-sum slots of whoever wrote the centred copy last
    const uint16_t* cen_in = xc;                  // the centred copy the next consumer reads
    const float* c_in = cbuf;                     // ... and the constants it was centred by
    uspace_gemm_ext prod{};                       // folded producers: centre by cbuf, write xc + part
    if (fold) {
        slots_skip = us_gemm_part_slots_k(M, D, 2 * D, sk_on), slots_proj = us_gemm_part_slots_k(M, D, D, sk_on);
        slots_fc2 = us_gemm_part_slots_k(M, D, Hd, sk_on);
        if (slots_skip <= 0 || slots_proj <= 0 || slots_fc2 <= 0) return USPACE_ERR_ARG;
        US_TRY(uspace_center_rows(x, xc, cbuf, part, M, D, stream));
        prod.row_c = cbuf; prod.out_cen = xc; prod.ld_cen = D; prod.part_out = part; prod.norm_dim = D; prod.eps = 1e-5f;
        prod.split_ws = plain.split_ws; prod.split_ws_bytes = plain.split_ws_bytes;
    }
    // norm1 -> qkv (fc1 = false) or norm2 -> fc1: folded, one consumer GEMM on the copy `cen` centred by `cen_c`, which publishes the
    // row means into c_out; separate, LayerNorm of x into h and a plain GEMM
    auto norm_gemm = [&](const BlockIdx& b, bool fc1, const uint16_t* cen, const float* cen_c, float* c_out) {
        const int N = fc1 ? Hd : 3 * D, act = fc1 ? G_ : 0;
        uint16_t* const out = fc1 ? f : qkv;
        if (fold) {
            uspace_gemm_ext cons{};
            cons.row_c = cen_c; cons.c_out = c_out; cons.part_in = part; cons.np_in = np; cons.norm_dim = D; cons.eps = 1e-5f;
            cons.colsum = PF(fc1 ? b.fc1_cs : b.qkv_cs);
            return us_gemm_bf16_ext(cen, D, nullptr, 0, D, PH(fc1 ? b.fc1_f : b.qkv_f), D, M, N, D, L_ | B_ | act | H_,
                                    PF(fc1 ? b.fc1_fb : b.qkv_fb), nullptr, 0, nullptr, 0, out, N, &cons, sk_on, stream);
        }
        US_TRY(uspace_layernorm_f32_bf16(x, PF(fc1 ? b.n2w : b.n1w), PF(fc1 ? b.n2b : b.n1b), h, M, D, 1e-5f, stream));
        return us_gemm_bf16_ext(h, D, nullptr, 0, D, PH(fc1 ? b.fc1w : b.qkv), D, M, N, D, fc1 ? (B_ | act | H_) : H_,
                                fc1 ? PF(b.fc1b) : nullptr, nullptr, 0, nullptr, 0, out, N, nullptr, sk_on, stream);
    };
    for (int i = 0; i < m.nblocks; ++i) {
        const BlockIdx& b = m.blk[i];
        const bool is_in = i < half, is_out = i > half, is_last = i == m.nblocks - 1;
        if (is_out) {
            // x = skip_linear(cat([x, skip]))  -- two K slabs, skips popped LIFO (libs/uvit.py:159,340)
            const int si = m.nblocks - 1 - i;
            uspace_gemm_ext e = fold ? prod : plain;
            if (fold) {
                e.row_add = cskip + (size_t)si * M;
                e.col_add = PF(b.skip_cs2);
            }
            US_TRY(us_gemm_bf16_ext(xb, D, skips + (size_t)si * MD, D, D, PH(b.skip_w), 2 * D, M, D, 2 * D, (fold ? K_ | C_ : 0) | B_ | F_,
                                    PF(b.skip_b), nullptr, 0, x, D, nullptr, 0, sk_ptr(e), sk_on, stream));
            np = slots_skip;
            cen_in = xc;
            c_in = cbuf;
        }
        // x += proj(attn(norm1(x)))
        US_TRY(norm_gemm(b, false, cen_in, c_in, cbuf));
        if (maps) US_TRY(uspace_attention_map_bf16(qkv, maps + (size_t)i * map_stride, B, L, H, mw.q0, mw.nq, mw.k0, mw.nk, stream));
        const float* ks = io->key_scale ? io->key_scale + (size_t)i * B * L : nullptr;
        US_TRY(us_attention_any(qkv, ks, h, B, L, H, stream));
        US_TRY(us_gemm_bf16_ext(h, D, nullptr, 0, D, PH(b.projw), D, M, D, D, (fold ? C_ : 0) | B_ | R_ | F_, PF(b.projb), x, D, x, D,
                                nullptr, 0, sk_ptr(fold ? prod : plain), sk_on, stream));
        np = slots_proj;
        // x += fc2(gelu(fc1(norm2(x)))); folded, the row means at norm2 of an in-block stay with its skip
        float* const c2 = fold && is_in ? cskip + (size_t)i * M : cbuf;
        US_TRY(norm_gemm(b, true, xc, cbuf, c2));
        // bf16 copy of the block output: the skip (in-blocks) or the next skip_linear's first K slab; none ahead of the head (its own
        // norm).  Folded, an in-block's copy is the centred one with its partial sums: the next block starts with a norm
        uint16_t* copy = is_in ? skips + (size_t)i * MD : (is_last ? nullptr : xb);
        uspace_gemm_ext e = plain;
        if (fold && is_in) {
            e = prod;
            e.row_c = c_in = c2;
            e.out_cen = copy;
            cen_in = copy;
            copy = nullptr;
            np = slots_fc2;
        }
        US_TRY(us_gemm_bf16_ext(f, Hd, nullptr, 0, Hd, PH(b.fc2w), Hd, M, D, Hd, (fold && is_in ? C_ : 0) | B_ | R_ | F_ | (copy ? H_ : 0),
                                PF(b.fc2b), x, D, x, D, copy, D, sk_ptr(e), sk_on, stream));
        if (i == half) {
            if (io->mid_tap) {
                if (hipMemcpyAsync(io->mid_tap, x, MD * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess)
                    return USPACE_ERR_LAUNCH;
            }
            if (io->mid_delta)  // u-space write hook at the mid block (libs/uvit.py:336, libs/dissection.py:157)
                US_TRY(uspace_add_broadcast_rows(x, xb, io->mid_delta, io->mid_scale, io->mid_row_scale, B, (long)L * D, stream));
        }
        if (i + 1 == stop_after && !is_last) return tap();
    }
    // the head: decoder weights with the last LayerNorm folded in, prepared by uspace_uvit_pack_weights
    US_TRY(us_output_head_packed(x, L, m.extras, PF(m.head_img), PF(m.convw), PF(m.convb), (float*)(ws + w.head), pair ? pair->pred : io->out,
                                 B, c.in_chans, c.img_size, c.patch_size, D, 1e-5f, (hipStream_t)stream));
    if (stop_after == m.nblocks) return tap();
    return USPACE_OK;
}
}  // namespace

extern "C" int uspace_uvit_forward(const uspace_uvit_config* cfg, const void* blob, void* workspace,
                                   size_t workspace_bytes, const uspace_uvit_io* io, int B, uspace_stream_t stream) {
    return forward_impl(cfg, blob, workspace, workspace_bytes, io, B, stream, ForwardOpts{});
}

extern "C" int uspace_uvit_forward_tap(const uspace_uvit_config* cfg, const void* blob, void* workspace, size_t workspace_bytes,
                                       const uspace_uvit_io* io, int B, int stop_after, float* dump, uspace_stream_t stream) {
    if (stop_after < 0) return USPACE_ERR_ARG;
    ForwardOpts opt;
    opt.stop_after = stop_after;
    opt.dump = dump;
    return forward_impl(cfg, blob, workspace, workspace_bytes, io, B, stream, opt);
}

extern "C" int uspace_uvit_forward_maps(const uspace_uvit_config* cfg, const void* blob, void* workspace, size_t workspace_bytes,
                                        const uspace_uvit_io* io, int B, int q0, int nq, int k0, int nk, float* maps,
                                        uspace_stream_t stream) {
    if (!maps) return USPACE_ERR_ARG;
    ForwardOpts opt;
    opt.maps = maps;
    opt.mw = MapWindow{q0, nq, k0, nk};
    return forward_impl(cfg, blob, workspace, workspace_bytes, io, B, stream, opt);
}

// ------------------------------------------------------------------------------------------
// Classifier-free guidance: conditional and unconditional branch of every sample in ONE forward over 2B rows, combined on the device.
// Workspace = that of a plain forward at batch 2B, then the 2B predictions.
// ------------------------------------------------------------------------------------------
namespace {
inline size_t pair_pred_bytes(const uspace_uvit_config& c, int B) {
    return ((size_t)2 * B * c.in_chans * c.img_size * c.img_size * 4 + 255) & ~(size_t)255;
}
constexpr int kMaxPairB = 1 << 29;
}  // namespace

extern "C" size_t uspace_uvit_cfg_workspace_bytes(const uspace_uvit_config* cfg, int B) {
    if (!valid_cfg(cfg) || B <= 0 || B > kMaxPairB) return 0;
    const size_t base = uspace_uvit_workspace_bytes(cfg, 2 * B);
    return base ? base + pair_pred_bytes(*cfg, B) : 0;
}

extern "C" int uspace_uvit_forward_cfg(const uspace_uvit_config* cfg, const void* blob, void* workspace, size_t workspace_bytes,
                                       const uspace_uvit_io* io, int B, const float* uncond, int uncond_batched, float scale,
                                       const float* row_scale, float* pair_out, uspace_stream_t stream) {
    if (!valid_cfg(cfg) || !blob || !workspace || !io || B <= 0 || B > kMaxPairB) return USPACE_ERR_ARG;
    if (cfg->n_extra == 0 || !uncond) return USPACE_ERR_ARG;          // nothing to drop
    if (!io->x || !io->t || !io->out || !io->context || io->mid_tap) return USPACE_ERR_ARG;
    const size_t base = uspace_uvit_workspace_bytes(cfg, 2 * B);
    if (!base || workspace_bytes < base + pair_pred_bytes(*cfg, B)) return USPACE_ERR_WORKSPACE;
    float* pred = pair_out ? pair_out : (float*)((char*)workspace + base);
    const PairArgs pair{uncond, uncond_batched != 0, pred};
    ForwardOpts opt;
    opt.pair = &pair;
    US_TRY(forward_impl(cfg, blob, workspace, base, io, B, stream, opt));
    return uspace_cfg_combine(pred, row_scale, scale, io->out, B, (long)cfg->in_chans * cfg->img_size * cfg->img_size, stream);
}

// ------------------------------------------------------------------------------------------
// hipGraph form of the forward: the ~160 dependent launches of one network evaluation are
// captured once (per batch size / hook mode) and replayed with a single hipGraphLaunch, which
// removes the host launch cost that dominates small batches (B = 4..16 trajectories).
// The io pointers are baked into the graph: the caller keeps them stable and refreshes their
// contents (x, t, context, mid_delta) before each replay.
// ------------------------------------------------------------------------------------------
struct uspace_uvit_graph {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
};

extern "C" int uspace_uvit_graph_create(const uspace_uvit_config* cfg, const void* blob, void* workspace,
                                        size_t workspace_bytes, const uspace_uvit_io* io, int B,
                                        uspace_stream_t capture_stream, uspace_uvit_graph** out) {
    if (!out || !capture_stream) return USPACE_ERR_ARG;   // the legacy NULL stream cannot be captured
    *out = nullptr;
    hipStream_t s = (hipStream_t)capture_stream;
    // one eager run first: first-use initialisation (kernel attributes) is not capturable
    int rc = uspace_uvit_forward(cfg, blob, workspace, workspace_bytes, io, B, capture_stream);
    if (rc != USPACE_OK) return rc;
    if (hipStreamSynchronize(s) != hipSuccess) return USPACE_ERR_LAUNCH;
    if (hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) != hipSuccess) return USPACE_ERR_LAUNCH;
    rc = uspace_uvit_forward(cfg, blob, workspace, workspace_bytes, io, B, capture_stream);
    hipGraph_t graph = nullptr;
    const hipError_t e = hipStreamEndCapture(s, &graph);
    if (rc != USPACE_OK || e != hipSuccess || !graph) {
        if (graph) (void)hipGraphDestroy(graph);
        return rc != USPACE_OK ? rc : USPACE_ERR_LAUNCH;
    }
    hipGraphExec_t exec = nullptr;
    if (hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) != hipSuccess) {
        (void)hipGraphDestroy(graph);
        return USPACE_ERR_LAUNCH;
    }
    uspace_uvit_graph* h = new uspace_uvit_graph;
    h->graph = graph;
    h->exec = exec;
    *out = h;
    return USPACE_OK;
}

extern "C" int uspace_uvit_graph_launch(uspace_uvit_graph* g, uspace_stream_t stream) {
    if (!g || !g->exec) return USPACE_ERR_ARG;
    return hipGraphLaunch(g->exec, (hipStream_t)stream) == hipSuccess ? USPACE_OK : USPACE_ERR_LAUNCH;
}

extern "C" int uspace_uvit_graph_destroy(uspace_uvit_graph* g) {
    if (!g) return USPACE_OK;
    if (g->exec) (void)hipGraphExecDestroy(g->exec);
    if (g->graph) (void)hipGraphDestroy(g->graph);
    delete g;
    return USPACE_OK;
}
