"""Classifier-free guidance, shared by tests/test_cfg_host.py and tests/test_gpu_cfg.py: the small networks, their seeded inputs, the
CPU oracle's conditional / unconditional predictions for them (computed once per process), the float64 reference of the guidance
formula, the combine kernel's bound, and the wrong formulas the bounds have to tell from the reference.

Convention (U-ViT's, the configs' ``sample.scale``): v = v_c + s (v_c - v_u); s = 0 is the conditional prediction.  On the device:
out = fmaf(s_b, c - u, c) in fp32 with s_b = s * row_scale[b]."""
import functools

import numpy as np
import torch

_BASE = dict(img_size=16, patch_size=2, in_chans=4, mlp_ratio=4, qkv_bias=False, mlp_time_embed=False)
# name -> (constructor kwargs, text-to-image?)
NETS = {
    "tiny_t2i": (dict(_BASE, embed_dim=64, depth=2, num_heads=1, clip_dim=64, num_clip_token=77), True),      # L = 142
    "mid_t2i": (dict(_BASE, embed_dim=128, depth=4, num_heads=2, clip_dim=128, num_clip_token=77), True),
    "tiny_cls": (dict(_BASE, embed_dim=64, depth=2, num_heads=1, num_classes=11), False),                     # label K = 10 is the empty class
    "long_t2i": (dict(_BASE, img_size=40, embed_dim=64, depth=2, num_heads=1, clip_dim=64, num_clip_token=77), True),   # L = 478: streaming attention
}
# The module's own init (0.02 trunc-normal weights) makes ONE label token among 66 move the class-conditional prediction by 3e-3 of
# its norm on the CPU oracle: no guidance test could tell it from nothing.  With the qkv weights 16 times larger (sharper attention:
# the patch tokens do look at the label) the oracle's ||v_c - v_u|| / ||v_c|| is 0.29.  The text-to-image nets keep the init as it is.
QKV_GAIN = {"tiny_cls": 16.0}
SEED = 2                     # tests.uvit_stages.make_net(kind="workflow", seed=2): the module's own init
T_VAL = 0.35
S_BIG, S_CFG = 7.5, 0.4      # a scale that makes a missing guidance term obvious; the configs' sample.scale
SWEEP = (0.0, 0.4, 7.5)      # per-sample scales at B = 3
FORWARD_TOL = 1e-2           # tests/test_gpu_forward.py: rel-L2 of one forward against the CPU oracle


def make(name, kind="workflow"):
    """The CPU module of ``NETS[name]`` with seeded parameters."""
    from tests import uvit_stages as US
    kw, t2i = NETS[name]
    net = US.make_net(dict(kw), kind=kind, seed=SEED, t2i=t2i)
    if name in QKV_GAIN:
        with torch.no_grad():
            for blk in net._blocks():
                blk.attn.qkv.weight.mul_(QKV_GAIN[name])
    return net


def spec(name):
    from oracle import uvit_oracle as O
    kw, t2i = NETS[name]
    keep = {k: kw[k] for k in ("img_size", "patch_size", "in_chans", "embed_dim", "depth", "num_heads", "mlp_ratio")}
    if t2i:
        return O.UViTSpec(t2i=True, clip_dim=kw["clip_dim"], num_clip_token=kw["num_clip_token"], **keep)
    return O.UViTSpec(num_classes=kw["num_classes"], **keep)


def inputs(name, B, seed=11):
    """Seeded inputs as numpy: x [B,C,S,S], and for a text-to-image net ctx [B,77,clip_dim] with the all-zero empty context
    [77,clip_dim]; for the class-conditional net labels y [B] (never the empty class) with the empty label."""
    kw, t2i = NETS[name]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, kw["in_chans"], kw["img_size"], kw["img_size"], generator=g).numpy()
    if t2i:
        ctx = torch.randn(B, kw["num_clip_token"], kw["clip_dim"], generator=g).numpy()
        return dict(x=x, ctx=ctx, empty=np.zeros((kw["num_clip_token"], kw["clip_dim"]), np.float32))
    K = kw["num_classes"] - 1
    y = torch.randint(0, K, (B,), generator=g).numpy()
    return dict(x=x, y=y, empty=K)


def oracle_pair_at(name, sd, inp, x, t, **kw):
    """(v_c, v_u) of the CPU oracle at state ``x`` and time ``t``, float32 numpy.  ``kw``: hook kwargs, applied to both branches."""
    from oracle import uvit_oracle as O
    sp = spec(name)
    B = x.shape[0]
    if NETS[name][1]:
        empty = np.broadcast_to(inp["empty"], (B,) + inp["empty"].shape[-2:])
        vc = O.uvit_forward(sp, sd, x, np.float32(t), context=inp["ctx"], **kw)
        vu = O.uvit_forward(sp, sd, x, np.float32(t), context=np.ascontiguousarray(empty), **kw)
    else:
        kw.setdefault("edit_loc", None)
        vc = O.uvit_forward(sp, sd, x, np.float32(t), y=inp["y"], **kw)
        vu = O.uvit_forward(sp, sd, x, np.float32(t), y=np.full(B, inp["empty"], np.int64), **kw)
    return vc, vu


@functools.lru_cache(maxsize=None)
def oracle_case(name, B):
    """(state dict as numpy, inputs, v_c, v_u) for ``inputs(name, B)`` at t = T_VAL: computed once, shared, never modified."""
    net = make(name)
    sd = {k: v.detach().numpy() for k, v in net.state_dict().items()}
    inp = inputs(name, B)
    vc, vu = oracle_pair_at(name, sd, inp, inp["x"], T_VAL)
    for a in (vc, vu):
        a.setflags(write=False)
    return sd, inp, vc, vu


# ------------------------------------------------------------------------------------------------------------------ the formula
def row_factors(s, B, row_scale=None):
    """s_b as the device forms it: the fp32 product s * row_scale[b] (row_scale None: s itself), float32 [B]."""
    s = np.float32(s)
    if row_scale is None:
        return np.full(B, s, np.float32)
    return (s * np.asarray(row_scale, np.float32)).astype(np.float32)


def guided_reference(vc, vu, s, row_scale=None):
    """float64 v_c + s_b (v_c - v_u); ``s`` a number, ``row_scale`` None or B per-sample factors."""
    vc, vu = np.asarray(vc, np.float64), np.asarray(vu, np.float64)
    sb = row_factors(s, vc.shape[0], row_scale).astype(np.float64).reshape((-1,) + (1,) * (vc.ndim - 1))
    return vc + sb * (vc - vu)


def combine_bound(vc, vu, s, row_scale=None):
    """(A): |got - ref64| <= 2^-22 (|s_b| |c - u| + |ref|) elementwise -- the fp32 rounding of c - u carried through the product
    and the rounding of the fused multiply-add, 2^-24 relative each, with a factor 4 over."""
    vc, vu = np.asarray(vc, np.float64), np.asarray(vu, np.float64)
    sb = row_factors(s, vc.shape[0], row_scale).astype(np.float64).reshape((-1,) + (1,) * (vc.ndim - 1))
    return 2.0 ** -22 * (np.abs(sb) * np.abs(vc - vu) + np.abs(guided_reference(vc, vu, s, row_scale)))


def _next(a):
    return np.roll(np.asarray(a), -1, axis=0)


# name -> f(vc, vu, s, row_scale) float64: what a broken implementation would return.  The last two need B > 1.
WRONG = {
    "scale_ignored": lambda vc, vu, s, rs: guided_reference(vc, vu, 0.0),
    "branches_swapped": lambda vc, vu, s, rs: guided_reference(vu, vc, s, rs),
    "anchored_on_uncond": lambda vc, vu, s, rs: np.asarray(vu, np.float64) + (guided_reference(vc, vu, s, rs) - np.asarray(vc, np.float64)),
    "uncond_row_of_next_sample": lambda vc, vu, s, rs: guided_reference(vc, _next(vu), s, rs),
    "row_scale_of_next_sample": lambda vc, vu, s, rs: guided_reference(vc, vu, s, _next(rs)),
}


def module_bound(s):
    """(C): ||got - ref|| / max(||v_c||, ||v_u||) <= (1 + 2|s|) FORWARD_TOL -- the forward bound on each branch, carried through
    v_c + s (v_c - v_u) = (1 + s) v_c - s v_u."""
    return (1.0 + 2.0 * abs(float(s))) * FORWARD_TOL


def module_err(got, ref, vc, vu):
    d = np.linalg.norm(np.asarray(got, np.float64) - np.asarray(ref, np.float64))
    return float(d / max(np.linalg.norm(np.asarray(vc, np.float64)), np.linalg.norm(np.asarray(vu, np.float64))))


def guidance_is_visible(vc, vu, s):
    """s ||v_c - v_u|| >= 3 bound ||v_c||: the guidance term is three bounds large, so a result without it cannot pass (C)."""
    vc, vu = np.asarray(vc, np.float64), np.asarray(vu, np.float64)
    return abs(float(s)) * np.linalg.norm(vc - vu) >= 3.0 * module_bound(s) * np.linalg.norm(vc)
