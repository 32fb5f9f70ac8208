"""U-ViT forward (uvit.hip) block by block against the float64 restatement of tests/uvit_stages.py, at the shapes the BASELINE
configurations run, in both LayerNorm modes (folded: the default; separate launches: ``uspace_uvit_set_ln_fold(0)``), on the
module's own seeded init ("workflow": LayerNorms (1, 0), zero biases) and on a "stress" set (gamma / beta and biases everywhere,
row means that dwarf the row std, massive channels, outlier tokens, a sink and a sharp head) that makes the fold's beta, its
centring constants and the rank-1 skip term visible.  The GPU's residual stream after every stage comes from
``uspace_uvit_forward_tap``.

A  every block against ``block(T_{k-1}, tight_<mode>)`` of the GPU's own previous tap (out-blocks take their skip from the GPU's
   in-block tap, LIFO; the fold's centring constants from the reference's own previous block), measured on the block's UPDATE
   ||T_k - ref_k|| / ||T_k - T_{k-1}|| -- the residual stream cannot hide a wrong branch; and against the loose float64 block.
   key_scale differs per block (L-t, S-t16): on the workflow set a block that reads its neighbour's slice moves its update by
   about 3e-2, ten times the bound.
A' the planted faults of tests/uvit_stages.py::FAULTS that A's bound cannot see (most of them move a block by less than the bound):
   on small nets, depth 4, the block's residual projected onto every such fault's direction, |c_f| < 0.5 (0: correct, 1: the
   fault); and a "tiny" net whose block 0 normalises rows with a variance of the order of eps, under A's bound.
B  the ends: stage 0 against the float64 embed (fp32-class), the output against the float64 head of T_{depth+1} (fp32-class:
   DESIGN.md 4.3, the hi+lo-split head).
C  end to end against the loose float64 forward from the latents, with the error's growth block by block.
D  the mid hook: T_{half+1} - mid_tap is mid_scale * row_scale * delta as one fp32 add, sample by sample.
E  the tap does not perturb: a forward after a tap call gives the same bits; a tap taken to the end gives the forward's output
   bits; hipGraph replay == eager.
F  a workspace full of 0xFF bytes gives the same bits as a fresh one, both modes, with the in-launch K-split tail (B = 32).
G  one sample across batch sizes: bit-equal where DESIGN.md 2 argues it (separate launches, no launch that cuts K), within a stated
   bound elsewhere.

Samples are independent, so the GPU runs whole batches (which selects the tile plans) and the float64 references run on sampled
samples.  Bounds are about 3x what an MI355X measured (written beside them), or the analytic bound where that is tighter."""
import ctypes

import numpy as np
import pytest
import torch

from tests import uvit_stages as S
from tests.util import fault_projection, rel_l2

pytestmark = pytest.mark.gpu

TOL = dict(
    update_tight=5e-3,      # measured 1.8e-3: ||T_k - block(T_{k-1}, tight)|| / ||T_k - T_{k-1}||, worst over blocks, sets, batch sizes, modes
    update_loose=1.1e-2,    # measured 3.7e-3: ... against the loose float64 block
    embed=3e-7,             # measured 9.2e-8: stage 0 vs float64 embed, rel-L2 (sin / cos of the time token and the patch GEMM in fp32)
    head=1.6e-5,            # measured 5.4e-6: output vs float64 head(T_{depth+1}), rel-L2
    e2e=1e-2,               # measured 6.0e-3: output vs the loose float64 forward from the latents (DESIGN.md 2 contract: 1e-2)
    batch=1.3e-2,           # measured 4.4e-3: one sample's block updates at B = 24 / 1 against B = 64, rel-L2, where bits differ
)
COMMON = dict(img_size=32, patch_size=2, in_chans=4, mlp_ratio=4, qkv_bias=False, mlp_time_embed=False)
NETS = {
    "L-u": (dict(embed_dim=1024, depth=20, num_heads=16, num_classes=-1), False),
    "L-t": (dict(embed_dim=1024, depth=20, num_heads=16, clip_dim=768, num_clip_token=77), True),
    "S-t16": (dict(embed_dim=512, depth=16, num_heads=8, clip_dim=768, num_clip_token=77), True),
    "S-cond": (dict(embed_dim=512, depth=16, num_heads=8, num_classes=1001), False),
}
# (network, parameter set, batch size, hooks): the U-ViT-L batch sizes select 256x256 + strips (64), the K-split tail of fc2 (32) and
# the small-launch K-split with 64x64 tiles (4)
CASES = [("L-u", "workflow", 64, None), ("L-u", "stress", 64, None), ("L-u", "stress", 32, None), ("L-u", "workflow", 32, None),
         ("L-u", "stress", 4, None), ("L-u", "stress", 32, "mid"), ("L-t", "stress", 64, "ks"), ("L-t", "workflow", 64, "ks"),
         ("S-t16", "workflow", 64, "ks"),
         ("S-t16", "stress", 64, "ks"), ("S-cond", "stress", 4, None), ("S-cond", "workflow", 4, None)]
_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _threads():
    n = S.cpu_threads()
    yield
    torch.set_num_threads(n)
    _cache.clear()


def _net(name, kind):
    key = (name, kind)
    if key not in _cache:
        kw, t2i = NETS[name]
        net = S.make_net(dict(COMMON, **kw), kind, seed=1234 if kind == "workflow" else 77, t2i=t2i).eval()
        sd = S.state_dict(net)
        _cache[key] = (net.cuda(), sd, S.Spec(img_size=32, embed_dim=kw["embed_dim"], depth=kw["depth"], num_heads=kw["num_heads"],
                                              num_classes=kw.get("num_classes", -1), t2i=t2i))
    return _cache[key]


def _inputs(spec, net, B, hooks, seed):
    """Latents, per-sample times and whatever the configuration and hook need, on the GPU (dict of _tap / _run keywords) and on
    the CPU (dict of S.forward keywords)."""
    x, t, cpu = S.inputs(spec, B, hooks, seed)          # (tests/uvit_stages.py: the host test of the planted faults builds the same)
    gpu = dict()
    if spec.t2i:
        gpu["context"] = cpu["context"].cuda()
    elif spec.n_extra:
        gpu["context"] = net.label_emb.weight.detach()[cpu["y"].cuda()].contiguous()
    if hooks == "ks":
        gpu["key_scale"] = cpu["key_scale"].cuda()
    if hooks == "mid":
        delta, scale, rows = cpu["mid"]
        gpu.update(mid_delta=delta.cuda(), mid_scale=scale, mid_row_scale=rows.cuda())
    return x, t, gpu, cpu


_rows = S.select_rows


class _Mode:
    def __init__(self, fold):
        self.fold = fold

    def __enter__(self):
        from uspace_amd import _hip
        _hip.check(_hip.lib().uspace_uvit_set_ln_fold(self.fold), "set_ln_fold")

    def __exit__(self, *a):
        from uspace_amd import _hip
        _hip.lib().uspace_uvit_set_ln_fold(-1)


def _folds(spec, B):
    """Whether the forward really folds at this batch size (it falls back to separate launches when a consumer would read more
    than 8 partial-sum slots per row)."""
    from uspace_amd import _hip
    return _hip.lib().uspace_gemm_part_slots_k(B * spec.L, spec.D, 64) <= 8


def _taps(net, spec, x, t, gpu, rows):
    """The GPU's stages 0 .. depth+1 for the sampled samples (CPU fp32) and the forward's output from the last tap call."""
    xd, td = x.cuda(), t.cuda()
    idx = torch.tensor(rows).cuda()
    T = [net._tap(k, xd, td, **gpu)[idx].cpu() for k in range(spec.nblocks)]
    out = torch.empty(x.shape[0], 4, 32, 32, device="cuda")
    T.append(net._tap(spec.nblocks, xd, td, out=out, **gpu)[idx].cpu())
    return T, out[idx].cpu()


def _per_block(spec, sd, T, mode, cpu):
    """A: the update errors of every block fed the GPU's own previous tap."""
    c, cskip, errs = None, [None] * spec.half, []
    for i in range(spec.nblocks):
        prev = T[i].double()
        skip = cs = None
        if i > spec.half:
            si = spec.nblocks - 1 - i                                   # LIFO
            skip, cs = T[si + 1], cskip[si]
        ks = None if "key_scale" not in cpu else cpu["key_scale"][i]
        ref, c = S.block(prev, sd, spec, i, mode, skip=skip, key_scale=ks, c_in=c, c_skip=cs)
        if i < spec.half:
            cskip[i] = c
        if i == spec.half and "mid" in cpu:
            ref = S.mid_hook(ref, *cpu["mid"])
        got = T[i + 1].double()
        errs.append(float((got - ref).norm() / (got - prev).norm()))
    return errs


# ------------------------------------------------------------------------------------------------------------------ A, B, C
@pytest.mark.parametrize("fold", [1, 0])
@pytest.mark.parametrize("case", CASES, ids=["-".join(str(v) for v in c if v) for c in CASES])
def test_every_block_against_float64(case, fold):
    name, kind, B, hooks = case
    net, sd, spec = _net(name, kind)
    x, t, gpu, cpu = _inputs(spec, net, B, hooks, seed=B + 7 * len(kind))
    rows = [B - 1] if B < 8 else [B // 3]
    with _Mode(fold):
        folded = fold and _folds(spec, B)
        assert folded == bool(fold)          # no workflow batch size makes the forward fall back from folding by itself
        T, out = _taps(net, spec, x, t, gpu, rows)
    mode = "tight_fold" if folded else "tight_sep"
    cr = _rows(cpu, rows)
    tight = _per_block(spec, sd, T, mode, cr)
    msg = f"{name} {kind} B={B} {hooks} {mode}"
    print(f"A {msg} update errors", " ".join("%.1e" % e for e in tight))
    assert max(tight) < TOL["update_tight"], (msg, tight)
    if B == 64 or hooks or spec.D == 512:
        loose = _per_block(spec, sd, T, "loose", cr)
        print(f"A {msg} loose", " ".join("%.1e" % e for e in loose))
        assert max(loose) < TOL["update_loose"], (msg, loose)
    # B: the ends
    e0 = rel_l2(T[0].numpy(), S.embed(spec, sd, x[rows], t[rows], y=cr.get("y"), context=cr.get("context"), tight=True).numpy())
    eh = rel_l2(out.numpy(), S.head(spec, sd, T[-1]).numpy())
    print(f"B {msg} embed {e0:.2e} head {eh:.2e}")
    assert e0 < TOL["embed"] and eh < TOL["head"], (msg, e0, eh)
    # C: end to end from the latents
    if B == 64 or hooks:
        ref, stages = S.forward(spec, sd, x[rows], t[rows], "loose", **cr)
        growth = [rel_l2(a.numpy(), b.numpy()) for a, b in zip(T, stages)]
        e = rel_l2(out.numpy(), ref.numpy())
        print(f"C {msg} out {e:.2e} growth", " ".join("%.1e" % g for g in growth))
        assert e < TOL["e2e"], (msg, e)


# ------------------------------------------------------------------------------------------------------------------ A'
def _fault_net(name):
    key = ("fault", name)
    if key not in _cache:
        net, sd, spec, hooks, B = S.fault_net(name)
        _cache[key] = (net.cuda(), sd, spec, hooks, B)
    return _cache[key]


@pytest.mark.parametrize("fold", [1, 0])
@pytest.mark.parametrize("name", ["u512", "t2i512", "u1024", "stress512", "tiny512"])
def test_no_planted_fault_explains_the_gpu_error(name, fold):
    """The update bound of A is 3x the rounding noise of a block, and most planted faults of S.FAULTS move a block by less.  So the
    block's residual r = T_k - block(T_{k-1}, tight_<mode>) is projected onto the direction d_f of every such fault (the loose model
    with and without it, from the GPU's own previous tap): c_f = <r, d_f> / <d_f, d_f> is 0 for a correct kernel and 1 for one with
    the fault; the noise is spread over L D elements and nearly orthogonal to d_f (tests/test_uvit_faults_host.py: within 0.25 of 0
    and of 1 with the tight model in the GPU's place).  Bound: 0.5, the midpoint.  The same for the final LayerNorm's eps in the
    head.  The stress net carries the omitted biases alone: every other direction drowns in the rounding of its massive channels.
    The tiny net carries no projection: it is there for A's bound on block 0, where a wrong LayerNorm eps is a plain fault."""
    net, sd, spec, hooks, B = _fault_net(name)
    seed, rows = S.fault_case(name)
    x, t, gpu, cpu = _inputs(spec, net, B, hooks, seed=seed)
    with _Mode(fold):
        folded = fold and _folds(spec, B)
        assert folded == bool(fold)
        T, out = _taps(net, spec, x, t, gpu, rows)
    mode = "tight_fold" if folded else "tight_sep"
    cr = _rows(cpu, rows)
    kw = {k: cr[k] for k in ("key_scale", "mid") if k in cr}
    T = [a.double() for a in T]
    faults = [f for f, (metric, _what) in S.FAULTS.items() if metric == "projection" and name in S.fault_nets(f)]
    worst = dict.fromkeys(faults, 0.0)
    c, cskip, errs = None, [None] * spec.half, []
    for i in range(spec.nblocks):
        tight, c = S.step(spec, sd, T, i, mode, c=c, cskip=cskip, **kw)
        if i < spec.half:
            cskip[i] = c
        errs.append(float((T[i + 1] - tight).norm() / (T[i + 1] - T[i]).norm()))
        true = S.step(spec, sd, T, i, "loose", **kw)[0]
        for f in faults:
            if i in S.fault_blocks(spec, f):
                cf = fault_projection(T[i + 1], tight, S.step(spec, sd, T, i, "loose", fault=f, **kw)[0], true)
                worst[f] = max(worst[f], abs(cf))
    if S.FAULTS["final_eps_1e-6"][0] == "projection_head" and name in S.fault_nets("final_eps_1e-6"):
        ref = S.head(spec, sd, T[-1])
        worst["final_eps_1e-6"] = abs(fault_projection(out, ref, S.head(spec, sd, T[-1], fault="final_eps_1e-6"), ref))
    print(f"A' {name} B={B} {mode} update errors", " ".join("%.1e" % e for e in errs),
          "|c_f|", " ".join(f"{f} {v:.3f}" for f, v in worst.items()))
    # A's own bound on these nets: what excludes the plain faults of the table at depth 4, and, on the tiny net, whose block 0
    # normalises rows with a variance of the order of eps, a wrong eps handed to either LayerNorm path (measured there: 6.0e-4; 1.2e-3 over these nets)
    assert max(errs) < TOL["update_tight"], (name, mode, errs)
    assert max(worst.values(), default=0.0) < S.PROJECTION_GPU, worst
    assert worst or name == "tiny512"


# ------------------------------------------------------------------------------------------------------------------ D
@pytest.mark.parametrize("fold", [1, 0])
def test_mid_hook_is_one_fp32_add(fold):
    net, sd, spec = _net("L-u", "stress")
    B = 32
    x, t, gpu, cpu = _inputs(spec, net, B, "mid", seed=5)
    tap = torch.empty(B, spec.L, spec.D, device="cuda")
    with _Mode(fold):
        after = net._tap(spec.half + 1, x.cuda(), t.cuda(), mid_tap=tap, **gpu).cpu()
        plain_mid = net._tap(spec.half + 1, x.cuda(), t.cuda()).cpu()
    before = tap.cpu()
    assert torch.equal(before, plain_mid)                              # the hook changes nothing before its add
    d, s, r = gpu["mid_delta"].cpu(), gpu["mid_scale"], gpu["mid_row_scale"].cpu()
    sc = (torch.tensor(s, dtype=torch.float32) * r)[:, None, None]      # fp32 scale * row_scale
    fused = (before.double() + d.double()[None] * sc.double()).float()  # x + delta * sc with one rounding (fma)
    split = before + d[None] * sc                                       # ... with two
    ok = (after == fused) | (after == split)
    assert bool(ok.all()), int((~ok).sum())
    assert not torch.equal(after, before)


# ------------------------------------------------------------------------------------------------------------------ E
@pytest.mark.parametrize("fold", [1, 0])
def test_tap_does_not_perturb_the_forward(fold):
    net, sd, spec = _net("L-u", "workflow")
    B = 32
    x, t, gpu, _ = _inputs(spec, net, B, None, seed=9)
    xd, td = x.cuda(), t.cuda()
    with _Mode(fold):
        ref = net._run(xd, td)
        net._tap(spec.half, xd, td)                                    # stops mid-way: leaves a half-written workspace behind
        assert torch.equal(net._run(xd, td), ref)
        out = torch.empty_like(ref)
        net._tap(spec.nblocks, xd, td, out=out)
        assert torch.equal(out, ref)
        t0 = torch.tensor(0.4, device="cuda").expand(B)
        eager = net._run(xd, t0)
        net.use_graph = True
        try:
            graph = net._run(xd, t0)
            assert torch.equal(eager, graph)
        finally:
            net.use_graph = False
            net.invalidate_packed()


# ------------------------------------------------------------------------------------------------------------------ F
@pytest.mark.parametrize("fold", [1, 0])
@pytest.mark.parametrize("B", [32, 4])
def test_poisoned_workspace_gives_the_same_bits(fold, B):
    from uspace_amd import _hip
    net, sd, spec = _net("L-u", "stress")
    x, t, gpu, _ = _inputs(spec, net, B, None, seed=11)
    xd, td = x.cuda(), t.cuda()
    nbytes = _hip.lib().uspace_uvit_workspace_bytes(ctypes.byref(net._cfg), B)
    with _Mode(fold):
        fresh = torch.empty(B, 4, 32, 32, device="cuda")
        tf = net._tap(spec.nblocks, xd, td, out=fresh, workspace=torch.zeros(nbytes, dtype=torch.uint8, device="cuda"))
        poisoned = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")
        out = torch.empty_like(fresh)
        tp = net._tap(spec.nblocks, xd, td, out=out, workspace=poisoned)
        assert torch.equal(out, fresh) and torch.equal(tp, tf)
        assert torch.equal(net._run(xd, td), fresh)


# ------------------------------------------------------------------------------------------------------------------ G
@pytest.mark.parametrize("fold", [1, 0])
def test_one_sample_across_batch_sizes(fold):
    """Sample 5 of a batch of 64 against itself in batches of 48 (no launch cuts K, the same token-embedding form: bit-equal in
    separate mode), 24 (no launch cuts K; the embedding's 4-token form) and 1 (the small-launch K-split)."""
    from uspace_amd import _hip
    net, sd, spec = _net("L-u", "stress")
    x, t, gpu, _ = _inputs(spec, net, 64, None, seed=13)
    j = 5
    with _Mode(fold):
        T64, o64 = _taps(net, spec, x, t, gpu, [j])
        for B in (48, 24, 1):
            lo = j if B == 1 else 0
            TB, oB = _taps(net, spec, x[lo:lo + B], t[lo:lo + B], {}, [j - lo])
            M = B * spec.L
            ksplit = any(_hip.lib().uspace_gemm_split_ws_bytes(M, n, k) or _hip.lib().uspace_gemm_sk_ws_bytes(M, n, k)
                         for n, k in ((spec.D, spec.D), (spec.D, 2 * spec.D), (spec.D, spec.hidden)))
            eq = [torch.equal(a, b) for a, b in zip(T64, TB)]
            d0 = (TB[0] - T64[0]).abs()
            errs = [float((TB[k + 1].double() - T64[k + 1].double()).norm() / (T64[k + 1].double() - T64[k].double()).norm())
                    for k in range(spec.nblocks)]
            print(f"G fold={fold} B={B} K-split={ksplit}: {sum(eq)} of {len(eq)} stages bit-equal, output equal {torch.equal(o64, oB)}, "
                  f"stage 0: {int((d0 > 0).sum())} elements differ (tokens {sorted(set(torch.nonzero(d0)[:, 1].tolist()))[:12]}, "
                  f"max {float(d0.max()):.1e}), worst update error {max(errs):.2e}")
            if B == 48 and not fold:
                assert all(eq) and torch.equal(o64, oB), eq
            assert max(errs) < TOL["batch"], (B, errs)
