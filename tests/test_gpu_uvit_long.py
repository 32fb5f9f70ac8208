"""The U-ViT forward beyond 336 tokens (latent sides 40 and 64: 401 / 478 and 1 025 / 1 102 tokens), where its attention is the
streaming kernel of uspace_amd/csrc/attention_long.hip: drop-in modules against the CPU oracle within the forward bound of
tests/test_gpu_forward.py (rel-L2 <= 1e-2, max-abs <= 3e-2 max|ref|), one Euler solve against the oracle solve within the bound of
tests/test_gpu_solver.py (1e-2), hipGraph replay against eager, and a guard that the lengths up to 336 stay on the resident kernel."""
import ctypes
import os
import tempfile

import numpy as np
import pytest
import torch

from oracle import odeint_oracle as OO
from oracle import uvit_oracle as O
from tests.test_gpu_forward import close, dev, expand_t
from tests.util import rel_l2

pytestmark = pytest.mark.gpu

BASE = dict(patch_size=2, in_chans=4, mlp_ratio=4, qkv_bias=False, mlp_time_embed=False)
# (name, img_size, embed_dim, num_heads): depth 2 everywhere
NETS = [("uvit", 40, 64, 1), ("uvit_t2i", 40, 64, 1), ("uvit", 64, 64, 1), ("uvit_t2i", 64, 64, 1), ("uvit", 40, 128, 2)]
TOKENS = {("uvit", 40): 401, ("uvit_t2i", 40): 478, ("uvit", 64): 1025, ("uvit_t2i", 64): 1102}
_CACHE = {}


def _net(name, img, D, H):
    """(module on the GPU, oracle spec, state dict as numpy), seeded, built once per shape."""
    key = (name, img, D, H)
    if key not in _CACHE:
        from uspace_amd.tools.utils_uvit import get_nnet
        torch.manual_seed(100 + img + D)
        extra = dict(clip_dim=64, num_clip_token=77) if name == "uvit_t2i" else dict(num_classes=-1)
        net = get_nnet(name, img_size=img, embed_dim=D, depth=2, num_heads=H, **BASE, **extra).to("cuda").eval()
        spec = O.UViTSpec(img_size=img, patch_size=2, in_chans=4, embed_dim=D, depth=2, num_heads=H, t2i=name == "uvit_t2i",
                          clip_dim=64, num_clip_token=77)
        assert spec.L == TOKENS[(name, img)] and spec.L > 336
        sd = {k: v.detach().cpu().numpy() for k, v in net.state_dict().items()}
        _CACHE[key] = (net, spec, sd)
    return _CACHE[key]


def _inputs(spec, B, seed=0):
    g = torch.Generator().manual_seed(9 + seed + spec.L)
    x = torch.randn(B, 4, spec.img_size, spec.img_size, generator=g).numpy()
    ctx = torch.randn(B, 77, 64, generator=g).numpy() if spec.t2i else None
    return x, ctx


def _call(net, spec, x, t, ctx, **kw):
    if spec.t2i:
        return net(dev(x), t, context=dev(ctx), **kw)[0]
    return net(dev(x), t, None, **({"edit_loc": None} if not kw else kw))[0]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name,img,D,H", NETS, ids=lambda v: str(v))
def test_forward_matches_the_oracle(name, img, D, H, B):
    """Plain forward (stride-0 timestep) and per-row timesteps."""
    net, spec, sd = _net(name, img, D, H)
    x, ctx = _inputs(spec, B)
    out = _call(net, spec, x, expand_t(0.35, B), ctx)
    assert out.shape == x.shape and out.dtype == torch.float32
    r = close(out.cpu().numpy(), O.uvit_forward(spec, sd, x, 0.35, context=ctx, edit_loc=None))
    print(f"\n[uvit_long {name} img={img} D={D} L={spec.L} B={B}] rel-L2 {r:.3e}")
    again = _call(net, spec, x, expand_t(0.35, B), ctx)
    assert torch.equal(out, again)
    if B > 1 and img == 40:
        tv = np.linspace(0.1, 0.9, B).astype(np.float32)
        out = _call(net, spec, x, torch.from_numpy(tv).cuda(), ctx)
        close(out.cpu().numpy(), O.uvit_forward(spec, sd, x, tv, context=ctx, edit_loc=None), mx=5e-2)


@pytest.mark.parametrize("img", [40, 64])
def test_mid_block_write_hook_matches_the_oracle(img):
    net, spec, sd = _net("uvit", img, 64, 1)
    x, _ = _inputs(spec, 3, seed=1)
    g = torch.Generator().manual_seed(5)
    with tempfile.TemporaryDirectory() as d:
        np.save(os.path.join(d, "delta_0.20.npy"), (torch.randn(4, spec.L, 64, generator=g) * 0.5).numpy())
        kw = dict(dissect_task="uspace_uvit", dissect_name="write_attr", t_edit=0.4, write_path_root=d, edit_loc="mid", ith_attr=2,
                  write_scale=1.5)
        out, _ = net(dev(x), expand_t(0.2, 3), None, **kw)
        ref = O.uvit_forward(spec, sd, x, 0.2, **kw)
        close(out.cpu().numpy(), ref)
        plain = O.uvit_forward(spec, sd, x, 0.2, edit_loc=None)
        assert rel_l2(ref, plain) > 1e-2                                  # the hook moves the result: the comparison is not vacuous


@pytest.mark.parametrize("img", [40, 64])
def test_p2p_rescale_edit_matches_the_oracle(img):
    """The T2I attention-map edit: key_scale through the streaming kernel while t <= t_edit, nothing after."""
    net, spec, sd = _net("uvit_t2i", img, 64, 1)
    x, ctx = _inputs(spec, 3, seed=2)
    ids = [np.array([3, 5]), np.array([], dtype=np.int64), np.array([0, 76])]
    kw = dict(dissect_name="p2p", fm_direction="decode", t_edit=0.5, block_id="all", target_context_ids=ids,
              token_kwargs=dict(token_dissect="p2p_rescale", p2p_multiplier=8.0))
    out = _call(net, spec, x, expand_t(0.3, 3), ctx, **kw)
    ref = O.uvit_forward(spec, sd, x, 0.3, context=ctx, **kw)
    close(out.cpu().numpy(), ref)
    plain = _call(net, spec, x, expand_t(0.3, 3), ctx)
    assert rel_l2(out.cpu().numpy(), plain.cpu().numpy()) > 1e-4
    late = _call(net, spec, x, expand_t(0.7, 3), ctx, **kw)                # t > t_edit: unedited, bit for bit
    assert torch.equal(late, _call(net, spec, x, expand_t(0.7, 3), ctx))


@pytest.mark.parametrize("name,img", [("uvit", 40), ("uvit_t2i", 64)])
def test_hipgraph_replay_is_bit_identical_to_eager(name, img):
    """What USPACE_UVIT_GRAPH=1 switches on (``use_graph``): the captured launch sequence holds the streaming kernel."""
    net, spec, sd = _net(name, img, 64, 1)
    x, ctx = _inputs(spec, 3, seed=3)
    outs = {}
    try:
        for use in (False, True):
            net.use_graph = use
            outs[use] = [_call(net, spec, x, expand_t(tv, 3), ctx) for tv in (0.1, 0.62, 0.62)]
            outs[use].append(_call(net, spec, x * 0.5, expand_t(0.62, 3), ctx))
    finally:
        net.use_graph = False
    for a, b in zip(outs[False], outs[True]):
        assert torch.equal(a, b)
    assert not torch.equal(outs[True][0], outs[True][1])


def test_euler_solve_matches_the_oracle_solve():
    from uspace_amd.flow_matching import CNF
    net, spec, sd = _net("uvit", 40, 64, 1)
    x, _ = _inputs(spec, 2, seed=4)
    cnf = CNF(net)
    got = cnf.decode(dev(x), None, dissect_name="none", edit_loc=None,
                     solver_kwargs=dict(solver="fixed", solver_fix="euler", solver_fix_step=0.25))
    assert cnf.last_stats.nfe == 4
    ref = OO.solve(lambda t, y: O.uvit_forward(spec, sd, y, np.float32(t), edit_loc=None), x, 0.0, 1.0, method="euler", step_size=0.25)
    assert rel_l2(got.cpu().numpy(), ref) < 1e-2


def test_attention_maps_stay_limited_to_336_tokens():
    from uspace_amd import _hip
    net, spec, sd = _net("uvit_t2i", 40, 64, 1)
    x, ctx = _inputs(spec, 1, seed=6)
    with pytest.raises(_hip.UspaceHipError):
        net.attention_maps(dev(x), expand_t(0.3, 1), dev(ctx))


REC_ATT_LONG = 2            # flags bit of an attention record: the streaming form (include/uspace_hip.h, uspace_prof_all_end)


def _attention_records(net, spec, x, ctx, **kw):
    from uspace_amd import _hip
    _hip.prof_all_begin()
    out = _call(net, spec, x, expand_t(0.35, x.shape[0]), ctx, **kw)
    torch.cuda.synchronize()
    return out, [r for r in _hip.prof_all_end() if r["kind"] == 1]


@pytest.mark.parametrize("name,img,L", [("uvit", 16, 65), ("uvit_t2i", 32, 334), ("uvit_t2i", 40, 478)])
def test_the_forward_takes_the_streaming_kernel_above_336_tokens_only(name, img, L):
    """The recorder marks a launch of the streaming kernel in its flags: every block of a forward at 65 and at 334 tokens launches the
    resident kernel, plain and under key_scale, and every block at 478 tokens the streaming one.  At L <= 336 the output is also bit-equal to
    what the forward gives when its attention launches are (necessarily) the resident kernel's: see the composition test below."""
    from uspace_amd.tools.utils_uvit import get_nnet
    torch.manual_seed(3)
    extra = dict(clip_dim=64, num_clip_token=77) if name == "uvit_t2i" else dict(num_classes=-1)
    net = get_nnet(name, img_size=img, embed_dim=64, depth=2, num_heads=1, **BASE, **extra).to("cuda").eval()
    spec = O.UViTSpec(img_size=img, patch_size=2, in_chans=4, embed_dim=64, depth=2, num_heads=1, t2i=name == "uvit_t2i", clip_dim=64,
                      num_clip_token=77)
    assert spec.L == L
    x, ctx = _inputs(spec, 3)
    want = REC_ATT_LONG if L > 336 else 0
    out, rec = _attention_records(net, spec, x, ctx)
    assert [(r["flags"], r["M"], r["N"], r["K"], r["launches"]) for r in rec] == [(want, 3, L, 64, 3)]
    sd = {k: v.detach().cpu().numpy() for k, v in net.state_dict().items()}
    close(out.cpu().numpy(), O.uvit_forward(spec, sd, x, 0.35, context=ctx, edit_loc=None))
    if spec.t2i:
        ids = [np.array([3, 5]), np.array([], dtype=np.int64), np.array([0, 76])]
        kw = dict(dissect_name="p2p", fm_direction="decode", t_edit=0.5, block_id="all", target_context_ids=ids,
                  token_kwargs=dict(token_dissect="p2p_rescale", p2p_multiplier=8.0))
        _, rec = _attention_records(net, spec, x, ctx, **kw)
        assert [(r["flags"], r["N"], r["launches"]) for r in rec] == [(want | 1, L, 3)]


@pytest.mark.parametrize("L,H", [(334, 2), (65, 1)])
def test_first_block_attention_is_the_resident_kernel_bit_for_bit(L, H):
    """Block 0 of a forward on the separate-LayerNorm path, recomposed from the operator wrappers on the tapped token stream:
    LayerNorm -> qkv GEMM -> ``_hip.attention`` (the resident kernel) -> proj GEMM with bias and residual is, bit for bit, what the
    forward holds after the same launches -- read through a net whose MLP of block 0 adds nothing (fc2 weight and bias zero), so that
    the stage-1 tap IS x + proj(attention).  The same composition with ``_hip.attention_long`` differs in some bits: the check
    separates the two kernels."""
    from uspace_amd import _hip
    from uspace_amd.tools.utils_uvit import get_nnet
    img = {334: 32, 65: 16}[L]
    name = "uvit_t2i" if L == 334 else "uvit"
    torch.manual_seed(11)
    extra = dict(clip_dim=64, num_clip_token=77) if name == "uvit_t2i" else dict(num_classes=-1)
    net = get_nnet(name, img_size=img, embed_dim=64 * H, depth=2, num_heads=H, **BASE, **extra).to("cuda").eval()
    with torch.no_grad():
        net.in_blocks[0].mlp.fc2.weight.zero_()
        net.in_blocks[0].mlp.fc2.bias.zero_()
    spec = O.UViTSpec(img_size=img, patch_size=2, in_chans=4, embed_dim=64 * H, depth=2, num_heads=H, t2i=name == "uvit_t2i",
                      clip_dim=64, num_clip_token=77)
    assert spec.L == L
    B, D = 3, 64 * H
    x, ctx = _inputs(spec, B)
    lib = _hip.lib()
    fold, sk = lib.uspace_uvit_get_ln_fold(), lib.uspace_gemm_get_sk()
    lib.uspace_uvit_set_ln_fold(0)
    lib.uspace_gemm_set_sk(0)           # (the GEMM wrappers below then take the forms the forward takes: no in-launch K-split tail)
    try:
        args = (dev(x), expand_t(0.35, B)) + ((dev(ctx),) if spec.t2i else ())
        tok = net._tap(0, *args).reshape(B * L, D).clone()
        after = net._tap(1, *args).reshape(B * L, D).clone()
        outs = _compose_block0_attention(_hip, net.in_blocks[0], tok, B, L, H)
    finally:
        lib.uspace_uvit_set_ln_fold(fold)
        lib.uspace_gemm_set_sk(sk)
    torch.cuda.synchronize()
    assert torch.equal(outs["resident"], after)
    assert not torch.equal(outs["long"], after)


def _compose_block0_attention(_hip, blk, tok, B, L, H):
    """x + proj(attention(qkv(norm1(x)))) from the operator wrappers, once per attention kernel."""
    D = 64 * H
    bf = lambda w: w.detach().to(torch.bfloat16).contiguous()
    h = _hip.layernorm(tok, blk.norm1.weight.detach().float(), blk.norm1.bias.detach().float())
    qkv = torch.empty(B * L, 3 * D, dtype=torch.bfloat16, device="cuda")
    _hip.gemm(h, bf(blk.attn.qkv.weight), out_bf16=qkv)
    outs = {}
    for form, fn in (("resident", _hip.attention), ("long", _hip.attention_long)):
        a = fn(qkv, B, L, H)
        y = tok.clone()
        nws = _hip.lib().uspace_gemm_split_ws_bytes(B * L, D, D)          # the forward hands proj its K-split workspace
        ws = torch.empty(nws // 4, dtype=torch.float32, device="cuda") if nws else None
        _hip.gemm(a, bf(blk.attn.proj.weight), bias=blk.attn.proj.bias.detach().float(), resid=y, out_f32=y, split_ws=ws)
        outs[form] = y
    return outs
