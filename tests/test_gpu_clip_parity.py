"""CLIP text encoder at the CLIP-L shape (D = 768, F = 3072, 12 heads, 12 layers, 77 tokens) against the float64 restatement of
tests/clip_stages.py, on generated parameters (a "workflow" set and a "stress" set: massive first token, large end-of-text channel,
attention-sink head, sharp head) and prompt-shaped ids.

A  every layer against ``layer(T_{k-1}, tight)`` of the GPU's own previous tap, measured on the layer's UPDATE (the residual stream
   cannot hide a wrong branch); tap 0 and the final LayerNorm exactly / to fp32 rounding.
B  end to end from the ids against the plain float64 forward (the whole bf16 budget), the error's growth layer by layer.
C  bit-equality of every prompt across batch sizes: the batch sizes cover every (GEMM shape, tile form, strips) the planner gives
   for B = 1 ... 128, so with A every form is verified (64x64 against float64, every other form against it).
D  prefixes and causality through all 12 layers, bit-exact.
E  the causal attention kernel on its own: tight / loose float64, row 0, future rows, NaN behind the tensor, sink / sharp heads.
F  a workspace full of 0xFF bytes gives the same bits as a fresh one.
G  quick-GELU over every finite bf16 input, the table lookup at 49408 x 768, both LayerNorm kernels at D = 768.

Every prompt is independent of the others (C, D), so the float64 references run on sampled prompts only.  Bounds are about 3x
what an MI355X measured (written beside them) or the analytic bound where that is tighter; bit-equal where an argument says so."""
import ctypes

import numpy as np
import pytest
import torch

from tests import clip_stages as S
from tests import unit_fault_cases as U
from tests.util import fault_projection, rel_l2

pytestmark = pytest.mark.gpu

TOL = dict(
    update_tight=4e-3,      # measured 1.3e-3: ||T_k - layer(T_{k-1}, tight)|| / ||T_k - T_{k-1}||, worst of 12 layers x 2 sets x B 1 / 8
    final_ln=1.8e-7,        # measured 6.1e-8: final LayerNorm vs float64 LN of T_12, rel-L2
    e2e_loose=2e-2,         # measured 5.9e-3 / 6.6e-3 (workflow / stress): last_hidden_state vs the float64 forward from the ids
    att_tight=6e-4,         # measured 1.9e-4 (0 at most shapes): causal attention vs float64 with the kernel's P rounding, rel-L2
    att_loose=6e-3,         # measured 2.0e-3: ... vs plain float64 softmax
    ln_err=22.0,            # measured 7.2 (fp32 out) / 0.9 (bf16 out, beyond one bf16 ulp), in units of the element's fp32 noise
                            # 2^-24 (|gamma| (|x| + |mean|) / sigma + |beta|); the analytic bound (10 roundings in the mean's tree + a few) is 32
)
# every (GEMM shape, tile form, strips) pair the planner gives the four CLIP launches for B = 1 ... 128 (M = 77 B, K-split tail off,
# which is what the forward runs: it passes no sk_ws) first appears at one of these batch sizes; plus the workflow sizes
FORM_BATCHES = (1, 8, 10, 14, 16, 17, 24, 34, 35, 36, 40, 44, 47, 50, 53, 57, 64, 70, 76, 94)
CLIP_GEMMS = dict(qkv=(2304, 768), proj=(768, 768), fc1=(3072, 768), fc2=(768, 3072))
ATT_L = (1, 2, 15, 16, 17, 32, 33, 63, 64, 65, 76, 77, 80, 81, 95, 96, 97, 112, 128, 129, 144, 159, 160)


@pytest.fixture(scope="module")
def models():
    from uspace_amd.libs.clip import CLIPTextTransformer, CLIP_L_TEXT
    n = S.cpu_threads()
    out = {}
    for seed, kind in enumerate(("workflow", "stress")):
        sd = S.clip_params(kind, seed=101 + seed, **CLIP_L_TEXT)
        m = CLIPTextTransformer(**CLIP_L_TEXT)
        m.load_state_dict(sd)
        out[kind] = (sd, m.cuda())
    yield out
    torch.set_num_threads(n)


def _taps(m, ids):
    return [m(ids, hidden_state=k).cpu() for k in range(13)]


# ------------------------------------------------------------------------------------------------------------------ A
@pytest.mark.parametrize("kind", ["workflow", "stress"])
@pytest.mark.parametrize("B", [1, 8])
def test_every_layer_against_float64_tight(models, kind, B):
    sd, m = models[kind]
    ids = S.prompt_ids(8, seed=200)[1:2] if B == 1 else S.prompt_ids(8, seed=201)
    rows = [0] if B == 1 else [0, 1, 4, 7]
    dev = ids.cuda()
    T = _taps(m, dev)
    assert torch.equal(T[0], S.embed(ids, sd).float())          # fp32 table + position, exact
    errs = []
    for k in range(1, 13):
        prev = T[k - 1][rows]
        R = S.layer(prev, sd, k - 1, "tight")
        upd = (T[k][rows].double() - prev.double()).norm()
        errs.append(float((T[k][rows].double() - R).norm() / upd))
    print(f"A {kind} B={B} update errors", ["%.2e" % e for e in errs])
    assert max(errs) < TOL["update_tight"], errs
    out = m(dev).cpu()
    fe = rel_l2(out[rows].numpy(), S.final_norm(T[12][rows], sd).numpy())
    print(f"A {kind} B={B} final LN {fe:.2e}")
    assert fe < TOL["final_ln"]


def test_no_planted_fault_explains_the_gpu_error(models):
    """The update bound of A is 3x a layer's rounding noise; the projection faults of S.FAULTS move a layer by less than ten such
    bounds.  So every layer's residual r = T_k - layer(T_{k-1}, tight) is projected onto each fault's direction d_f (the loose model
    with and without the fault, from the GPU's own previous tap): c_f = <r, d_f> / <d_f, d_f> is 0 for a correct kernel and 1 for one
    with the fault (tests/test_clip_faults_host.py: within 0.25 of either with the tight model in the GPU's place).  Bound: 0.5."""
    sd, m = models["workflow"]
    n, seed, rows = S.FAULT_IDS
    rows = list(rows)
    ids = S.prompt_ids(n, seed=seed)
    T = [t[rows].double() for t in _taps(m, ids.cuda())]
    faults = [f for f, (metric, _what) in S.FAULTS.items() if metric == "projection"]
    worst = dict.fromkeys(faults, 0.0)
    for k in range(12):
        tight, true = S.layer(T[k], sd, k, "tight"), S.layer(T[k], sd, k, "loose")
        for f in faults:
            worst[f] = max(worst[f], abs(fault_projection(T[k + 1], tight, S.layer(T[k], sd, k, "loose", fault=f), true)))
    print("A' workflow |c_f|", " ".join(f"{f} {v:.3f}" for f, v in worst.items()))
    assert worst and max(worst.values()) < S.PROJECTION_GPU, worst


def test_layer_0_normalises_rows_at_eps():
    """On the workflow and stress sets no row a LayerNorm sees has a variance below 0.2, and an eps of 1e-6 moves a layer's update by
    1e-5.  The "tiny" set (both tables at 0.003x, two layers) puts rows with a variance of 2.6e-6 in front of layer 0: there the eps
    clip.hip hands to its LayerNorm launches moves the update by 0.62 (tests/test_clip_faults_host.py).  A's bound on both layers."""
    from uspace_amd.libs.clip import CLIPTextTransformer, CLIP_L_TEXT
    cfg = dict(CLIP_L_TEXT, num_hidden_layers=2)
    sd = S.clip_params("tiny", seed=101, **cfg)
    m = CLIPTextTransformer(**cfg)
    m.load_state_dict(sd)
    m = m.cuda()
    n, seed, rows = S.FAULT_IDS
    rows = list(rows)
    dev = S.prompt_ids(n, seed=seed).cuda()
    T = [m(dev, hidden_state=k).cpu()[rows].double() for k in range(3)]
    assert float(T[0].var(-1).max()) < 1e-5
    errs = [float((T[k + 1] - S.layer(T[k], sd, k, "tight")).norm() / (T[k + 1] - T[k]).norm()) for k in range(2)]
    print("A' tiny update errors", ["%.2e" % e for e in errs])         # measured 1.2e-3
    assert max(errs) < TOL["update_tight"], errs


# ------------------------------------------------------------------------------------------------------------------ B
@pytest.mark.parametrize("kind", ["workflow", "stress"])
def test_end_to_end_against_float64_loose(models, kind):
    sd, m = models[kind]
    ids = S.prompt_ids(8, seed=300)[:2]                          # the empty prompt and one that fills the context
    dev = ids.cuda()
    ref, hidden = S.forward(ids, sd, "loose")
    growth = [rel_l2(m(dev, hidden_state=k).cpu().numpy(), hidden[k].numpy()) for k in range(13)]
    e = rel_l2(m(dev).cpu().numpy(), ref.numpy())
    print(f"B {kind} growth", ["%.2e" % g for g in growth], f"out {e:.2e}")
    assert growth[0] == 0.0
    assert e < TOL["e2e_loose"] and max(growth) < TOL["e2e_loose"], (e, growth)


# ------------------------------------------------------------------------------------------------------------------ C
def _plans():
    from uspace_amd import _hip
    L = _hip.lib()
    plan = (ctypes.c_int * 8)()
    old = L.uspace_gemm_get_sk()
    L.uspace_gemm_set_sk(0)
    try:
        out = {}
        for B in range(1, 129):
            for name, (N, K) in CLIP_GEMMS.items():
                _hip.check(L.uspace_gemm_plan_k(77 * B, N, K, 0, plan), "plan")
                out[B, name] = tuple(plan)
        return out
    finally:
        L.uspace_gemm_set_sk(old)


def _positions(B, plans):
    """Where the 8 probe prompts go in a batch of B: first, last, and on the rows where each launch's main tiles end (the prompt
    that straddles the first strip / remainder row, and the one after it), then evenly spread."""
    if B <= 8:
        return list(range(B))
    want = [0, B - 1]
    for name in CLIP_GEMMS:
        p = plans[B, name]
        bm, tm, ns = p[2], p[4], p[6]
        edge = tm * bm if ns else (tm - 1) * bm                  # first strip row / first row of the last (partial) tile row
        want += [min(edge // 77, B - 1), min(edge // 77 + 1, B - 1), min((77 * B - 1) // 77, B - 1)]
    want += np.linspace(0, B - 1, 8).round().astype(int).tolist()
    pos = []
    for w in want:
        if w not in pos:
            pos.append(int(w))
    return pos[:8]


def test_every_prompt_is_bit_equal_across_batch_sizes(models):
    plans = _plans()
    pairs = {}
    for (B, name), p in plans.items():
        pairs.setdefault((name, p[0], p[6] > 0), []).append(B)
    missing = {k: v[0] for k, v in pairs.items() if not set(v) & set(FORM_BATCHES)}
    assert not missing, f"the planner gives CLIP launches forms no batch size here runs: {missing} -- add them to FORM_BATCHES"
    sd, m = models["workflow"]
    probes = S.prompt_ids(8, seed=400)
    single = [m(probes[i:i + 1].cuda()) for i in range(8)]
    for B in FORM_BATCHES:
        pos = _positions(B, plans)
        ids = S.prompt_ids(B, seed=500 + B, lengths=[(7 * b) % 76 for b in range(B)])    # fillers
        for i, p in enumerate(pos):
            ids[p] = probes[i]
        out = m(ids.cuda())
        for i, p in enumerate(pos):
            assert torch.equal(out[p], single[i][0]), (B, p, i, {n: plans[B, n][:8] for n in CLIP_GEMMS},
                                                        float((out[p] - single[i][0]).abs().max()))


# ------------------------------------------------------------------------------------------------------------------ D
@pytest.mark.parametrize("kind", ["workflow", "stress"])
def test_prefixes_and_causality_are_bit_exact(models, kind):
    sd, m = models[kind]
    ids = S.prompt_ids(8, seed=600)
    full = m(ids.cuda())
    for Lp in (1, 16, 33, 64, 76):
        assert torch.equal(m(ids[:, :Lp].contiguous().cuda()), full[:, :Lp]), Lp
    g = torch.Generator().manual_seed(601)
    for p in (0, 20, 50, 75):
        other = ids.clone()
        other[:, p + 1:] = torch.randint(0, S.EOS + 1, (8, 76 - p), generator=g)
        got = m(other.cuda())
        assert torch.equal(got[:, :p + 1], full[:, :p + 1]), p
        if p < 76:
            assert not torch.equal(got[:, p + 1:], full[:, p + 1:])


# ------------------------------------------------------------------------------------------------------------------ E
def _causal(qkv, B, L, H):
    from uspace_amd import _hip
    out = torch.empty(B, L, 64 * H, dtype=torch.bfloat16, device="cuda")
    _hip.check(_hip.lib().uspace_attention_causal_bf16(_hip.ptr(qkv), _hip.ptr(out), B, L, H, _hip.stream_ptr()), "causal attention")
    return out


@pytest.mark.parametrize("H", [1, 12])
@pytest.mark.parametrize("L", ATT_L)
def test_causal_attention_at_clip_shapes(L, H):
    i = ATT_L.index(L)
    B = (24, 96, 288, 768)[i % 4] // H                             # B * H from 24 to 768 workgroups
    D = 64 * H
    g = torch.Generator().manual_seed(700 + L * 13 + H)
    qkv = torch.randn(B, L, 3 * D, generator=g) * 0.8
    if H == 12:
        e = torch.randn(64, generator=g)
        e = e / e.norm()
        s3 = slice(64 * S.SINK_HEAD, 64 * S.SINK_HEAD + 64)
        qkv[:, :, s3] += 4.0 * e                                  # sink: q . k0 / 8 ~ 4 * 50 / 8 = 25 over the other keys
        qkv[:, 0, D + 64 * S.SINK_HEAD:D + 64 * S.SINK_HEAD + 64] += 50.0 * e
        qkv[:, :, 64 * S.SHARP_HEAD:64 * S.SHARP_HEAD + 64] *= 4.0   # sharp: 4x the logits
    qkv = qkv.to(torch.bfloat16)
    dq = qkv.cuda()
    out = _causal(dq, B, L, H)
    # the first query sees key 0 alone: P = 1 exactly, out = v_0 exactly
    assert torch.equal(out[:, 0], dq[:, 0, 2 * D:])
    # against float64 on sampled sequences (tight: P rounded as the kernel rounds it)
    rows = sorted({0, B - 1})
    q, k, v = (qkv[rows, :, j * D:(j + 1) * D].double() for j in range(3))
    got = out[rows].cpu().double()
    et = rel_l2(got.numpy(), S.causal_attention(q, k, v, H, True).numpy())
    el = rel_l2(got.numpy(), S.causal_attention(q, k, v, H, False).numpy())
    print(f"E L={L} H={H} B={B} tight {et:.2e} loose {el:.2e}")
    assert et < TOL["att_tight"] and el < TOL["att_loose"], (et, el)
    # rows after q are invisible to rows 0..q: other finite K / V there leave those rows bit-identical
    if L > 1:
        qq = L // 2
        other = dq.clone()
        other[:, qq + 1:, D:] = (torch.randn(B, L - qq - 1, 2 * D, generator=g) * 3.0).to(torch.bfloat16).cuda()
        o2 = _causal(other, B, L, H)
        assert torch.equal(o2[:, :qq + 1], out[:, :qq + 1])
    # NaN / Inf behind the tensor (rows past the last sequence: the kernel's padded key tiles read there in no path)
    n = dq.numel()
    big = torch.empty(n + 64 * 3 * D, dtype=torch.bfloat16, device="cuda")
    big[:n] = dq.reshape(-1)
    pat = torch.tensor([0x7FC0, 0x7F80, -0x80, 0x7FFF], dtype=torch.int16)   # NaN, +Inf, -Inf, NaN
    big[n:] = pat.repeat(16 * 3 * D).view(torch.bfloat16).cuda()
    assert torch.equal(_causal(big[:n], B, L, H), out)


# ------------------------------------------------------------------------------------------------------------------ F
@pytest.mark.parametrize("B", [1, 8])
def test_poisoned_workspace_gives_the_same_bits(models, B):
    sd, m = models["workflow"]
    ids = S.prompt_ids(8, seed=800)[:B]
    for L in (33, 64, 77):
        dev = ids[:, :L].contiguous().cuda()
        m._ws.clear()
        fresh = m(dev)
        (key, ws), = m._ws.items()
        ws.fill_(0xFF)                                            # every fp32 / bf16 word of the workspace a NaN
        assert torch.equal(m(dev), fresh), L
        assert m._ws[key] is ws                                   # ... and the forward ran on it
    m._ws.clear()


# ------------------------------------------------------------------------------------------------------------------ G
def _bf16_ulp(r):
    """bf16 ulp at |r| (float64 tensor), the subnormal spacing below the normal range."""
    e = torch.floor(torch.log2(r.abs().clamp_min(2.0 ** -126)))
    return torch.exp2(e - 7)


def test_quick_gelu_every_finite_bf16_input():
    from uspace_amd import _hip
    pat = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    pat = pat[((pat >> 7) & 0xFF) != 0xFF]                         # the 65 280 finite patterns (n % 4 == 0)
    x = torch.from_numpy(pat.view(np.int16).copy()).view(torch.bfloat16)
    d = x.cuda()
    _hip.check(_hip.lib().uspace_quick_gelu_bf16(_hip.ptr(d), d.numel(), _hip.stream_ptr()), "quick_gelu")
    xd = x.double()
    ref = xd * torch.sigmoid(1.702 * xd)
    got = d.cpu().double()
    err = (got - ref).abs()
    # an absolute floor of 2^-122 only where the true result underflows: below the normal range (|y| < 2^-126, subnormal inputs), and
    # for x < -52.1, where exp(-1.702 x) overflows fp32 and the kernel returns -0 (the true |y| there is < 1.6e-37 = 2^-122.2)
    tiny = (ref.abs() < 2.0 ** -126) | (xd < -52.1)
    ok = torch.where(tiny, got.abs() <= 2.0 ** -122, err <= _bf16_ulp(ref))
    worst = float((err / _bf16_ulp(ref))[~tiny].max())              # measured 0.500 ulp
    print(f"G quick-GELU worst {worst:.3f} ulp, {int(tiny.sum())} inputs under the floor")
    assert bool(ok.all()), [(float(xd[i]), float(got[i]), float(ref[i])) for i in torch.nonzero(~ok)[:8, 0]]


def test_table_embed_at_clip_l(models):
    from uspace_amd import _hip
    sd, _ = models["stress"]
    tok, pos = sd["embeddings.token_embedding.weight"], sd["embeddings.position_embedding.weight"]
    ids = S.prompt_ids(64, seed=900)
    assert int(ids.min()) == 0 and int(ids.max()) == S.EOS
    out = torch.empty(64, 77, 768, device="cuda")
    t_, p_, i_ = tok.cuda(), pos.cuda(), ids.to(torch.int32).cuda()
    _hip.check(_hip.lib().uspace_table_embed(_hip.ptr(i_), _hip.ptr(t_), _hip.ptr(p_), _hip.ptr(out), 64, 77, 768, 49408,
                                             _hip.stream_ptr()), "table_embed")
    assert torch.equal(out.cpu(), tok[ids] + pos[None])


@pytest.mark.parametrize("M", [77, 4928])
def test_layernorm_kernels_at_d768(M):
    from uspace_amd import _hip
    D = 768
    g = torch.Generator().manual_seed(1000 + M)
    x = torch.randn(M, D, generator=g) * 1.5 + torch.randn(M, 1, generator=g) * 2.0
    x[::11, list(S.MASSIVE)] = torch.tensor([64.0, -64.0, 64.0, -64.0])    # massive-activation rows
    x[5, 3] = 500.0
    gam, bet = 1.0 + 0.2 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    xd = x.double()
    xh = (xd - xd.mean(-1, keepdim=True)) / torch.sqrt(xd.var(-1, unbiased=False, keepdim=True) + 1e-5)
    ref = xh * gam.double() + bet.double()
    # fp32 noise scale of one element: the rounding of the mean enters as |mean| / sigma, that of x as |x| / sigma
    sigma = torch.sqrt(xd.var(-1, unbiased=False, keepdim=True) + 1e-5)
    scale = 2.0 ** -24 * (gam.double().abs() * (xd.abs() + xd.mean(-1, keepdim=True).abs()) / sigma + bet.double().abs())
    dx, dg, db = x.cuda(), gam.cuda(), bet.cuda()
    L = _hip.lib()
    y32 = torch.empty(M, D, device="cuda")
    _hip.check(L.uspace_layernorm_f32(_hip.ptr(dx), _hip.ptr(dg), _hip.ptr(db), _hip.ptr(y32), M, D, ctypes.c_float(1e-5),
                                      _hip.stream_ptr()), "layernorm_f32")
    e32 = float(((y32.cpu().double() - ref).abs() / scale).max())
    yb = torch.empty(M, D, dtype=torch.bfloat16, device="cuda")
    _hip.check(L.uspace_layernorm_f32_bf16(_hip.ptr(dx), _hip.ptr(dg), _hip.ptr(db), _hip.ptr(yb), M, D, ctypes.c_float(1e-5),
                                           _hip.stream_ptr()), "layernorm_f32_bf16")
    eb = ((yb.cpu().double() - ref).abs() - _bf16_ulp(ref)).clamp_min(0.0) / scale
    print(f"G LN M={M} fp32 {e32:.2f} x 2^-24 scale, bf16 beyond one ulp {float(eb.max()):.2f}")
    assert e32 < TOL["ln_err"]
    assert float(eb.max()) < TOL["ln_err"]
    # rows whose variance is of the order of eps (1e-6 ... 1e-4; the rows above have variances of 2 and more, on which no eps shows),
    # in the same units against float64: an eps of 1e-6 lies 1e6 bounds away (tests/test_clip_faults_host.py).  Measured: 3.8 / 0.0
    assert M in U.CLIP_LAYERNORM_M
    xs, gs, bs = U.ln_eps_rows(64, D, seed=1100 + M)
    ref = torch.from_numpy(U.layernorm_f64(xs, gs, bs))
    scale = torch.from_numpy(U.ln_noise_scale(xs, gs, bs))
    dx, dg, db = (torch.from_numpy(a).cuda() for a in (xs, gs, bs))
    y32 = torch.empty(64, D, device="cuda")
    _hip.check(L.uspace_layernorm_f32(_hip.ptr(dx), _hip.ptr(dg), _hip.ptr(db), _hip.ptr(y32), 64, D, ctypes.c_float(1e-5),
                                      _hip.stream_ptr()), "layernorm_f32")
    e32 = float(((y32.cpu().double() - ref).abs() / scale).max())
    yb = torch.empty(64, D, dtype=torch.bfloat16, device="cuda")
    _hip.check(L.uspace_layernorm_f32_bf16(_hip.ptr(dx), _hip.ptr(dg), _hip.ptr(db), _hip.ptr(yb), 64, D, ctypes.c_float(1e-5),
                                           _hip.stream_ptr()), "layernorm_f32_bf16")
    eb = ((yb.cpu().double() - ref).abs() - _bf16_ulp(ref)).clamp_min(0.0) / scale
    print(f"G LN M={M} rows at eps: fp32 {e32:.2f} x 2^-24 scale, bf16 beyond one ulp {float(eb.max()):.2f}")
    assert e32 < TOL["ln_err"] and float(eb.max()) < TOL["ln_err"]
