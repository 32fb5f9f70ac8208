"""The calls whose raw output bytes pin the host sequence of a U-ViT forward (uspace_amd/csrc/uvit.hip) bit for bit (a helper, not a
test): small networks built through the two module classes with the seeded init of tests/uvit_stages.py (every norm and bias then
moved off its (1, 0) by seeded noise), run in both
LayerNorm modes (uspace_uvit_set_ln_fold) through every exported form of the forward -- the tap at every stage, the mid hook with its
tap, key scales, attention maps and the paired classifier-free-guidance forward.  Shared by tests/golden/make_uvit_forward_digests.py
(which records the sha256 of every output and the launch recorder's table) and tests/test_gpu_uvit_forward_bits.py (which compares).
A change of the host code that moves no launch and no operand leaves every digest and every table row as it is.

Widths 64 and 128 (skip_linear's two K slabs need a power of two): the head's K-split form needs D % 128 == 0 and at most 4096 patch
tokens, so 128 takes it at batch 3 and the other form at batch 33, 64 the other form at both; batches 3 and 33 are also the two forms
of the token embedding."""
import os

import numpy as np
import torch

from tests import uvit_stages as US
from tests.vit_tower_cases import digest

HERE = os.path.dirname(os.path.abspath(__file__))
DIGESTS = os.path.join(HERE, "golden", "uvit_forward_digests.json")

DEPTH = 2
KINDS = ("uncond", "class", "t2i")
WIDTHS = (64, 128)
BATCHES = (3, 33)
CLIP_DIM, CLIP_TOKENS, NUM_CLASSES = 64, 3, 10
CASES = tuple(f"{kind}-D{D}-B{B}" for kind in KINDS for D in WIDTHS for B in BATCHES)
LN_MODES = (1, 0)                       # folded through the GEMMs, separate launches
MAP_WINDOW = (1, 9, 0, 12)              # (q0, nq, k0, nk)
EPI_LN_IN = 64


def parse(case):
    kind, D, B = case.split("-")
    return kind, int(D[1:]), int(B[1:])


_nets = {}


def net_for(kind, D):
    """The module on the GPU (built once per process)."""
    if (kind, D) not in _nets:
        kw = dict(img_size=32, patch_size=2, in_chans=4, embed_dim=D, depth=DEPTH, num_heads=D // 64, mlp_ratio=4, qkv_bias=False,
                  mlp_time_embed=False)
        if kind == "t2i":
            kw.update(clip_dim=CLIP_DIM, num_clip_token=CLIP_TOKENS)
        else:
            kw.update(num_classes=NUM_CLASSES if kind == "class" else -1)
        net = US.make_net(kw, kind="workflow", seed=D, t2i=kind == "t2i")
        g = torch.Generator().manual_seed(D + 1)
        with torch.no_grad():                                          # the init leaves every norm at (1, 0) and every bias at 0
            for p in net.parameters():
                if p.dim() == 1:
                    p.add_(0.2 * torch.randn(p.shape, generator=g))
        _nets[(kind, D)] = net.cuda().eval()
    return _nets[(kind, D)]


def inputs(case):
    """Seeded device inputs of one case: x, t (per sample), the context in the form ``_run`` takes it (None, label tokens [B, 1, D] or
    CLIP features [B, 3, 64]), the unconditional contexts (one and B), the mid hook's operands and a key-scale table."""
    kind, D, B = parse(case)
    net = net_for(kind, D)
    rng = np.random.default_rng(1000 * D + 10 * B + KINDS.index(kind))
    f = lambda *s, scale=1.0: torch.from_numpy((rng.standard_normal(s) * scale).astype(np.float32)).cuda()
    a = dict(x=f(B, 4, 32, 32), t=torch.from_numpy(rng.uniform(0.05, 0.95, B).astype(np.float32)).cuda(), context=None)
    if kind == "class":
        a.update(context=f(B, 1, D), uncond1=f(1, D), uncondB=f(B, 1, D))
    elif kind == "t2i":
        a.update(context=f(B, CLIP_TOKENS, CLIP_DIM), uncond1=f(CLIP_TOKENS, CLIP_DIM), uncondB=f(B, CLIP_TOKENS, CLIP_DIM))
    L = net.seq_len
    a.update(mid_delta=f(L * D, scale=0.5), mid_rows=torch.from_numpy(rng.uniform(-1.0, 2.0, B).astype(np.float32)).cuda())
    ks = np.ones((DEPTH + 1, B, L), np.float32)
    ks[:, :, rng.integers(0, L, 20)] = 2.5
    ks[1, 0, 0] = 0.0
    a["key_scale"] = torch.from_numpy(ks).cuda()
    ks2 = np.concatenate([ks, np.ones_like(ks)], axis=1)              # a paired forward runs 2B rows
    a["key_scale_pair"] = torch.from_numpy(ks2).cuda()
    return net, a


class ln_mode:
    """with ln_mode(m): the forwards inside run in LayerNorm mode m."""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        from uspace_amd import _hip
        self.old = _hip.lib().uspace_uvit_get_ln_fold()
        assert _hip.lib().uspace_uvit_set_ln_fold(self.mode) == 0

    def __exit__(self, *exc):
        from uspace_amd import _hip
        _hip.lib().uspace_uvit_set_ln_fold(self.old)


def outputs(case, mode):
    """Generator of (call, tensor) of one case in one LayerNorm mode."""
    kind, D, B = parse(case)
    net, a = inputs(case)
    x, t, ctx = a["x"], a["t"], a["context"]
    with ln_mode(mode), torch.no_grad():
        out = torch.empty(B, 4, 32, 32, device="cuda")
        for stage in range(DEPTH + 2):
            yield f"tap{stage}", net._tap(stage, x, t, context=ctx, out=out)
        yield "tap-out", out                                           # the head ran at the last stage
        yield "out", net._run(x, t, context=ctx)
        mid_tap = torch.empty(B, net.seq_len, D, device="cuda")
        yield "mid/out", net._run(x, t, context=ctx, mid_delta=a["mid_delta"], mid_scale=0.75, mid_tap=mid_tap, mid_row_scale=a["mid_rows"])
        yield "mid/tap", mid_tap
        yield "key_scale/out", net._run(x, t, context=ctx, key_scale=a["key_scale"])
        o, maps = net._run(x, t, context=ctx, attn_maps=MAP_WINDOW)
        yield "maps/out", o
        yield "maps/maps", maps
        if kind != "uncond":
            for name, batched in (("uncond1", False), ("uncondB", True)):
                o, pair = net._run(x, t, context=ctx, cfg=(a[name].contiguous(), batched, 1.5, a["mid_rows"], True))
                yield f"cfg-{name}/out", o
                yield f"cfg-{name}/pair", pair
            o, pair = net._run(x, t, context=ctx, key_scale=a["key_scale_pair"], mid_delta=a["mid_delta"], mid_scale=0.75,
                               cfg=(a["uncond1"].contiguous(), False, 1.5, None, True))
            yield "cfg-hooks/out", o
            yield "cfg-hooks/pair", pair


def case_digests(case):
    """{"fold" / "separate": {call: sha256}} of one case, computed on the GPU."""
    out = {}
    for mode in LN_MODES:
        out["fold" if mode else "separate"] = {call: digest(t) for call, t in outputs(case, mode)}
    torch.cuda.synchronize()
    return out


def launch_table(case, mode):
    """The launch recorder's rows [kind, flags, M, N, K, launches] (GEMM and attention launches) of one plain forward, sorted."""
    from uspace_amd import _hip
    net, a = inputs(case)
    with ln_mode(mode), torch.no_grad():
        net._run(a["x"], a["t"], context=a["context"])                 # first use (packing, kernel attributes) stays outside
        torch.cuda.synchronize()
        _hip.prof_all_begin()
        net._run(a["x"], a["t"], context=a["context"])
        torch.cuda.synchronize()
        assert _hip.prof_dropped() == 0
        rec = _hip.prof_all_end()
    return sorted([r["kind"], r["flags"], r["M"], r["N"], r["K"], r["launches"]] for r in rec)


def folded_rows(table):
    """The rows of a launch table that are GEMMs with the LayerNorm finished in their epilogue (USPACE_EPI_LN_IN)."""
    return [r for r in table if r[0] == 0 and r[1] & EPI_LN_IN]
