"""The float64 U-ViT restatement of tests/uvit_stages.py (the reference of tests/test_gpu_uvit_parity.py) pinned on the CPU: its
loose mode against the reference's own outputs and taps (tests/golden/tiny_u, tiny_u_cond, tiny_t2i, p2p_t2i, hooks_u), against
the fp32 numpy oracle at U-ViT-S width; both tight modes with their rounding switched off against loose; and the generated stress
parameters do what they claim."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import uvit_oracle as O
from tests import uvit_stages as S
from tests.util import rel_l2

TINY = dict(img_size=16, patch_size=2, in_chans=4, embed_dim=64, depth=2, num_heads=1)
# the goldens are the reference's fp32 CPU runs: fp32 noise only (measured 0.8e-7 ... 3.5e-7 over every output and tap below)
GOLDEN_TOL = 1e-6


@pytest.fixture(scope="module", autouse=True)
def _threads():
    n = S.cpu_threads()
    yield
    torch.set_num_threads(n)


def _load(golden_dir, name):
    z = np.load(os.path.join(golden_dir, name))
    return z, {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd/")}


def _check_taps(spec, sd, z, h0, key_scale=None):
    """Block by block from the golden's own taps: tok, b0_* (in-block 0), in0, mid, o0_skip, out0, norm, dec."""
    assert rel_l2(h0.numpy(), z["tap/tok"]) < GOLDEN_TOL
    taps = {}
    ks = lambda i: None if key_scale is None else key_scale[i]
    y, _ = S.block(torch.from_numpy(z["tap/tok"]), sd, spec, 0, "loose", key_scale=ks(0), taps=taps)
    for k in ("norm1", "qkv", "attn", "fc1", "mlp"):
        assert rel_l2(taps[k].numpy(), z["tap/b0_" + k]) < GOLDEN_TOL, k
    assert rel_l2(y.numpy(), z["tap/in0"]) < GOLDEN_TOL
    m, _ = S.block(torch.from_numpy(z["tap/in0"]), sd, spec, 1, "loose", key_scale=ks(1))
    assert rel_l2(m.numpy(), z["tap/mid"]) < GOLDEN_TOL
    taps = {}
    o, _ = S.block(torch.from_numpy(z["tap/mid"]), sd, spec, 2, "loose", skip=torch.from_numpy(z["tap/in0"]), key_scale=ks(2),
                   taps=taps)
    assert rel_l2(taps["skip"].numpy(), z["tap/o0_skip"]) < GOLDEN_TOL
    assert rel_l2(o.numpy(), z["tap/out0"]) < GOLDEN_TOL
    taps = {}
    S.head(spec, sd, torch.from_numpy(z["tap/out0"]), taps=taps)
    assert rel_l2(taps["norm"].numpy(), z["tap/norm"]) < GOLDEN_TOL
    assert rel_l2(taps["dec"].numpy(), z["tap/dec"]) < GOLDEN_TOL


def test_loose_matches_reference_tiny_u(golden_dir):
    z, sd = _load(golden_dir, "tiny_u.npz")
    spec = S.Spec(**TINY)
    for i, tv in enumerate(z["tvals"]):
        out, stages = S.forward(spec, sd, z["x"], float(tv), "loose")
        assert rel_l2(out.numpy(), z[f"out{i}"]) < GOLDEN_TOL, i          # measured 1.5e-7
        assert len(stages) == spec.depth + 2
        if i == 1:
            _check_taps(spec, sd, z, stages[0])
            assert torch.equal(stages[1], S.block(stages[0], sd, spec, 0, "loose")[0])


def test_loose_matches_reference_label_token_first(golden_dir):
    z, sd = _load(golden_dir, "tiny_u_cond.npz")
    spec = S.Spec(num_classes=10, **TINY)
    assert spec.extras == 2 and spec.time_first == 0
    out, stages = S.forward(spec, sd, z["x"], float(z["tval"]), "loose", y=z["y"])
    assert rel_l2(stages[0].numpy(), z["tok"]) < GOLDEN_TOL                 # measured 7.8e-8
    assert rel_l2(out.numpy(), z["out"]) < GOLDEN_TOL                       # measured 2.7e-7
    # the label token is row 0, the time token row 1
    lab = sd["label_emb.weight"][torch.as_tensor(z["y"], dtype=torch.long)].double() + sd["pos_embed"][0, 0].double()
    assert torch.allclose(stages[0][:, 0], lab, rtol=0, atol=1e-12)


def test_loose_matches_reference_t2i(golden_dir):
    z, sd = _load(golden_dir, "tiny_t2i.npz")
    spec = S.Spec(t2i=True, clip_dim=64, num_clip_token=77, **TINY)
    assert spec.L == 142 and spec.time_first == 1
    for i, tv in enumerate(z["tvals"]):
        out, stages = S.forward(spec, sd, z["x"], float(tv), "loose", context=z["ctx"])
        assert rel_l2(out.numpy(), z[f"out{i}"]) < GOLDEN_TOL, i
        if i == 1:
            _check_taps(spec, sd, z, stages[0])


def test_loose_matches_reference_key_scale(golden_dir):
    """p2p_t2i.npz: the attention-map edit as per-block column factors (oracle.p2p_column_scale, block ids counted as the reference
    counts them); every case, edited or not."""
    zt, sd = _load(golden_dir, "tiny_t2i.npz")
    z = np.load(os.path.join(golden_dir, "p2p_t2i.npz"))
    cases = json.loads(bytes(z["cases_json"]).decode())
    spec = S.Spec(t2i=True, clip_dim=64, num_clip_token=77, **TINY)
    ids = [z["ids_a0"], z["ids_a1"], z["ids_a2"]]
    B = zt["x"].shape[0]
    edited = 0
    for i, c in enumerate(cases):
        kw = dict(c)
        tv = kw.pop("tval")
        kw.pop("ids")
        kw["target_context_ids"] = ids
        cols = [O.p2p_column_scale(B, spec.L, tv, kw, b) for b in range(spec.nblocks)]
        ks = None
        if any(cs is not None for cs in cols):
            ks = torch.stack([torch.ones(B, spec.L, dtype=torch.float64) if cs is None else torch.from_numpy(cs).double() for cs in cols])
            edited += 1
        out, _ = S.forward(spec, sd, zt["x"], float(tv), "loose", context=zt["ctx"], key_scale=ks)
        assert rel_l2(out.numpy(), z[f"case{i}"]) < GOLDEN_TOL, (i, c)     # measured <= 2.6e-7
    assert edited >= 3


def test_loose_matches_reference_mid_hook(golden_dir):
    """hooks_u.npz mid cases: a token-shaped direction added after the mid block (one row, and the mean of two rows at -0.5)."""
    zt, sd = _load(golden_dir, "tiny_u.npz")
    z = np.load(os.path.join(golden_dir, "hooks_u.npz"))
    spec = S.Spec(**TINY)
    for key, ith, scale in (("mid0", 2, 1.0), ("mid1", "1_3", -0.5)):
        delta = torch.from_numpy(O.select_delta(z["tok_attr"], ith)[0])
        mid_out = []
        out, stages = S.forward(spec, sd, zt["x"], 0.2, "loose", mid=(delta, scale, None), mid_out=mid_out)
        assert rel_l2(out.numpy(), z[key]) < GOLDEN_TOL, key                # measured 1.4e-7
        assert torch.equal(stages[spec.half + 1], S.mid_hook(mid_out[0], delta, scale))
    # a per-sample factor of 1 is the plain hook; 0 is no hook
    delta = torch.from_numpy(O.select_delta(z["tok_attr"], 2)[0])
    rows = torch.tensor([1.0, 0.0, 1.0])
    out, _ = S.forward(spec, sd, zt["x"], 0.2, "loose", mid=(delta, 1.0, rows))
    plain, _ = S.forward(spec, sd, zt["x"], 0.2, "loose")
    assert rel_l2(out[[0, 2]].numpy(), z["mid0"][[0, 2]]) < GOLDEN_TOL
    assert torch.equal(out[1], plain[1])


@pytest.mark.parametrize("t2i", [False, True])
def test_loose_matches_the_fp32_oracle_at_s_width(t2i):
    """U-ViT-S (D = 512, 8 heads; depth 4 to keep it quick) on the stress parameters: the float64 restatement against the fp32
    numpy oracle, output and taps.  Measured 6.6e-7 / 1.4e-6 (uncond / t2i) at the output."""
    kw = dict(img_size=32, patch_size=2, in_chans=4, embed_dim=512, depth=4, num_heads=8, mlp_ratio=4, qkv_bias=False,
              mlp_time_embed=False)
    if t2i:
        kw.update(clip_dim=768, num_clip_token=77)
    else:
        kw.update(num_classes=-1)
    net = S.make_net(kw, "stress", seed=21, t2i=t2i)
    sd = S.state_dict(net)
    spec = S.Spec(img_size=32, embed_dim=512, depth=4, num_heads=8, t2i=t2i)
    ospec = O.UViTSpec(img_size=32, embed_dim=512, depth=4, num_heads=8, t2i=t2i)
    g = torch.Generator().manual_seed(22)
    x = torch.randn(2, 4, 32, 32, generator=g)
    ctx = torch.randn(2, 77, 768, generator=g) if t2i else None
    taps = {}
    ref = O.uvit_forward(ospec, {k: v.numpy() for k, v in sd.items()}, x.numpy(), 0.45,
                         context=None if ctx is None else ctx.numpy(), taps=taps, edit_loc=None)
    out, stages = S.forward(spec, sd, x, 0.45, "loose", context=ctx)
    assert rel_l2(out.numpy(), ref) < 5e-6, rel_l2(out.numpy(), ref)
    assert rel_l2(stages[0].numpy(), taps["tok"]) < 1e-6
    assert rel_l2(stages[spec.half + 1].numpy(), taps["mid"]) < 3e-6
    assert rel_l2(stages[-1].numpy(), taps[f"out{spec.half - 1}"]) < 5e-6


@pytest.mark.parametrize("kind", ["workflow", "stress"])
def test_tight_modes_collapse_to_loose_without_rounding(kind, golden_dir):
    """The tight modes keep their data flow (centring by the previous norm's mean, gamma / beta folded into the weights, the skip
    stored centred with its rank-1 term) with every bf16 rounding switched off: float64 noise from loose.  With the rounding on they
    move by the bf16 budget (measured 1e-3 ... 1e-2), the stress set's fold data flow visibly (row means dwarf the row std)."""
    kw = dict(img_size=16, patch_size=2, in_chans=4, embed_dim=128, depth=4, num_heads=2, mlp_ratio=4, qkv_bias=False,
              mlp_time_embed=False, num_classes=-1)
    net = S.make_net(kw, kind, seed=31)
    sd = S.state_dict(net)
    spec = S.Spec(img_size=16, embed_dim=128, depth=4, num_heads=2)
    g = torch.Generator().manual_seed(32)
    x = torch.randn(2, 4, 16, 16, generator=g)
    ks = 0.5 + torch.rand(spec.nblocks, 2, spec.L, generator=g, dtype=torch.float64)
    mid = (torch.randn(spec.L, spec.D, generator=g), 0.7, torch.tensor([1.0, -2.0]))
    ref, rs = S.forward(spec, sd, x, 0.3, "loose", key_scale=ks, mid=mid)
    for mode in ("tight_sep", "tight_fold"):
        out, st = S.forward(spec, sd, x, 0.3, mode, key_scale=ks, mid=mid, rounding=False)
        assert rel_l2(out.numpy(), ref.numpy()) < 1e-12, mode
        assert max(rel_l2(a.numpy(), b.numpy()) for a, b in zip(st, rs)) < 1e-12, mode
        rounded, _ = S.forward(spec, sd, x, 0.3, mode, key_scale=ks, mid=mid)
        assert 1e-4 < rel_l2(rounded.numpy(), ref.numpy()) < 3e-2, mode


def test_stress_parameters_do_what_they_claim():
    kw = dict(img_size=32, patch_size=2, in_chans=4, embed_dim=512, depth=2, num_heads=8, mlp_ratio=4, qkv_bias=False,
              mlp_time_embed=False, num_classes=-1)
    sd = S.state_dict(S.make_net(kw, "stress", seed=41))
    assert torch.equal(sd["pos_embed"], S.state_dict(S.make_net(kw, "stress", seed=41))["pos_embed"])     # seeded
    spec = S.Spec(img_size=32, embed_dim=512, depth=2, num_heads=8)
    x = torch.randn(2, 4, 32, 32, generator=torch.Generator().manual_seed(42))
    h = S.embed(spec, sd, x, 0.5)
    core = h[..., [c for c in range(512) if c not in (7, 130, 301, 455)]]
    # row means dwarf the row std (outside the massive channels), so the centring constants carry most of the value
    assert float((core.mean(-1).abs() / core.std(-1)).median()) > 5.0
    assert float(h[..., 7].abs().min()) > 30.0
    for n in ("norm1.weight", "norm2.bias", "attn.proj.bias", "mlp.fc1.bias", "mlp.fc2.bias"):
        assert float(sd["in_blocks.0." + n].std()) > 0.05, n
    assert float(sd["out_blocks.0.skip_linear.bias"].abs().min()) > 0.5
    # the sink head: every query's logit for key 0 leads the others by tens; the sharp head's logits spread 4x wider
    taps = {}
    S.block(h, sd, spec, 0, "loose", taps=taps)
    q, k = taps["qkv"][..., :512], taps["qkv"][..., 512:1024]
    r = slice(64 * S.SINK_HEAD, 64 * S.SINK_HEAD + 64)
    s = q[..., r] @ k[..., r].transpose(-1, -2) / 8
    gap = s[:, :, 0] - s[:, :, 1:].amax(-1)
    assert float(gap.min()) > 8 and 15 < float(gap.median()) < 80, (float(gap.min()), float(gap.median()))
    r2, r0 = slice(64 * S.SHARP_HEAD, 64 * S.SHARP_HEAD + 64), slice(0, 64)
    sp = lambda rr: float((q[..., rr] @ k[..., rr].transpose(-1, -2)).std())
    assert sp(r2) > 2.5 * sp(r0)
