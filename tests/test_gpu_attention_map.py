"""The head-mean attention map on the GPU: the kernel (uspace_amd/csrc/attention_map.hip) against float64, the forward readout
(``uspace_uvit_forward_maps``) against the plain forward, the float64 stage model and the reference's own ``attn`` tensor
(tests/golden/attn_maps_t2i.npz), the ``vis_am_path`` pictures and the hipGraph path.  Cases, reference, metrics, faults and bounds:
tests/attention_map_cases.py.  Every figure is printed before it is asserted (``pytest -s`` shows them)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from tests import attention_map_cases as AM
from tests import uvit_stages as US
from tests.util import load_sd

pytestmark = pytest.mark.gpu

TINY = dict(img_size=16, patch_size=2, in_chans=4, embed_dim=64, depth=2, num_heads=1, mlp_ratio=4,
            qkv_bias=False, mlp_time_embed=False)
COMMON = dict(img_size=32, patch_size=2, in_chans=4, mlp_ratio=4, qkv_bias=False, mlp_time_embed=False)
S_CFG = dict(embed_dim=512, depth=16, num_heads=8)
MID = dict(img_size=16, patch_size=2, in_chans=4, embed_dim=128, depth=4, num_heads=2, mlp_ratio=4)     # two heads, two skips
T_VIS = 0.30


def _say(name, value, where):
    print(f"MEASURED {name} {value:.3e} at {where} (bound {AM.TOL[name]})")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def expand_t(tv, B):
    return torch.tensor(float(tv), dtype=torch.float32, device="cuda").expand(B)


def build(sd=None, **cfg):
    from uspace_amd.tools.utils_uvit import get_nnet
    net = get_nnet("uvit_t2i", **cfg)
    if sd is not None:
        net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return net.to("cuda").eval()


class ln_fold:
    def __init__(self, fold):
        self.fold = fold

    def __enter__(self):
        from uspace_amd import _hip
        _hip.check(_hip.lib().uspace_uvit_set_ln_fold(self.fold), "set_ln_fold")

    def __exit__(self, *a):
        from uspace_amd import _hip
        _hip.lib().uspace_uvit_set_ln_fold(-1)


class ToyTokenizer:
    """One id per whitespace word between a begin and an end token; decode gives the word back."""

    def __init__(self):
        self.words = ["<s>", "</s>"]

    def encode(self, text):
        ids = [0]
        for w in text.split():
            if w not in self.words:
                self.words.append(w)
            ids.append(self.words.index(w))
        return ids + [1]

    def decode(self, i):
        return self.words[int(i)]


def p2p_kwargs(B, t_edit=0.5, **more):
    ids = [np.array([3, 5], dtype=np.int64), np.array([], dtype=np.int64), np.array([0, 76, 76], dtype=np.int64)]
    kw = dict(dissect_name="p2p", fm_direction="decode", t_edit=t_edit, block_id="all",
              token_kwargs=dict(token_dissect="p2p_rescale", p2p_multiplier=3.0), target_context_ids=[a.copy() for a in ids[:B]])
    kw.update(more)
    return kw


# ------------------------------------------------------------------------------------------------------------------ (a) kernel
@pytest.mark.parametrize("case", AM.CASES, ids=AM.case_id)
def test_kernel_against_float64(case):
    from uspace_amd import _hip
    B, L, H, win, data = case
    w = AM.window(win, L)
    qkv = AM.make_qkv(B, L, H, data)
    got = _hip.attention_map(qkv.cuda().reshape(B * L, -1), B, L, H, *w).cpu().numpy()
    assert got.shape == (B, w[1], w[3]) and np.isfinite(got).all()
    ref = AM.reference(qkv, H, w).numpy()
    r, e = AM.row_err(got, ref), AM.elem_err(got, ref)
    _say("map_row", r, AM.case_id(case))
    _say("map_elem", e, AM.case_id(case))
    assert r <= AM.TOL["map_row"] and e <= AM.TOL["map_elem"]
    if win == "full":
        s = got.astype(np.float64).sum(2)
        assert np.abs(s - 1.0).max() <= 1e-5, "rows of the full map sum to 1"


def test_case_list_covers_what_it_must():
    assert {c[1] for c in AM.CASES} >= set(AM.REQUIRED_L) and {c[2] for c in AM.CASES} >= set(AM.REQUIRED_H)
    assert {c[3] for c in AM.CASES} >= set(AM.REQUIRED_WINDOWS)


def test_kernel_argument_errors():
    from uspace_amd import _hip
    qkv = AM.make_qkv(1, 20, 1, "workflow").cuda().reshape(20, -1)
    for w in ((-1, 4, 0, 4), (0, 0, 0, 4), (17, 4, 0, 4), (0, 4, -1, 4), (0, 4, 0, 0), (0, 4, 19, 2), (0, 21, 0, 1)):
        with pytest.raises(_hip.UspaceHipError):
            _hip.attention_map(qkv, 1, 20, 1, *w)
    out = torch.empty(1, 1, 1, device="cuda")
    assert _hip.lib().uspace_attention_map_bf16(_hip.ptr(qkv), _hip.ptr(out), 1, 337, 1, 0, 1, 0, 1, _hip.stream_ptr()) == -1


# ------------------------------------------------------------------------------------------------------------------ (b) bit-equality
def test_kernel_bit_equal_across_runs_and_batches():
    from uspace_amd import _hip
    for L, H, win in ((334, 16, "ic"), (142, 8, "full"), (257, 16, "odd")):
        B = 5
        w = AM.window(win, L)
        qkv = AM.make_qkv(B, L, H, "workflow").cuda()
        a = _hip.attention_map(qkv.reshape(B * L, -1), B, L, H, *w)
        b = _hip.attention_map(qkv.reshape(B * L, -1), B, L, H, *w)
        assert torch.equal(a, b)
        for s in (0, 3, 4):
            one = _hip.attention_map(qkv[s].contiguous(), 1, L, H, *w)
            assert torch.equal(one[0], a[s]), f"sample {s} alone differs from the same sample inside the batch (L = {L})"


# ------------------------------------------------------------------------------------------------------------------ (c) forward readout
def _inputs(net, B, seed=5):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, net.in_chans, net.img_size, net.img_size, generator=g)
    ctx = torch.randn(B, net.num_clip_token, net.clip_dim, generator=g)
    return x, ctx


def _key_scale(net, B, seed=9):
    g = torch.Generator().manual_seed(seed)
    ks = torch.ones(net.depth + 1, B, net.seq_len)
    ks[:, :, 1:78] = torch.where(torch.rand(net.depth + 1, B, 77, generator=g) < 0.2, torch.tensor(3.0), torch.tensor(1.0))
    ks[:, 0, 4] = 3.0
    return ks


@pytest.mark.parametrize("fold", [1, 0], ids=["fold", "sep"])
def test_forward_maps_leaves_the_prediction_bit_equal(fold):
    """io->out of uspace_uvit_forward_maps == that of uspace_uvit_forward, with and without key_scale; block 0's map does not see
    key_scale."""
    with ln_fold(fold):
        for cfg, seed in ((dict(TINY, clip_dim=64), 2), (dict(MID, clip_dim=128), 3)):
            torch.manual_seed(seed)
            net = build(num_clip_token=77, **cfg)
            B = 3
            x, ctx = _inputs(net, B)
            x, ctx = x.cuda(), ctx.cuda()
            win = net.token_range("image") + net.token_range("context")
            maps = {}
            for name, ks in (("plain", None), ("ks", _key_scale(net, B).cuda())):
                plain = net._run(x, expand_t(T_VIS, B), context=ctx, key_scale=ks)
                out, m = net._run(x, expand_t(T_VIS, B), context=ctx, key_scale=ks, attn_maps=win)
                assert torch.equal(plain, out), f"{name}: the prediction moved"
                assert m.shape == (net.depth + 1, B, win[1], win[3]) and bool(torch.isfinite(m).all())
                maps[name] = m
            assert torch.equal(maps["plain"][0], maps["ks"][0]), "block 0's map saw key_scale"
            assert not torch.equal(maps["plain"][1], maps["ks"][1]), "the edit of block 0 must reach block 1 through the residual stream"


def _model_qkv(net, x, ctx, mode, key_scale=None):
    """bf16 qkv of every block as the float64 stage model has it (tests/uvit_stages.py), [depth + 1][B, L, 3 D]."""
    spec = US.Spec(img_size=net.img_size, patch_size=net.patch_size, in_chans=net.in_chans, embed_dim=net.embed_dim, depth=net.depth,
                   num_heads=net.num_heads, t2i=True, clip_dim=net.clip_dim, num_clip_token=net.num_clip_token)
    sd = US.state_dict(net)
    h = US.embed(spec, sd, x, torch.full((x.shape[0],), T_VIS), context=ctx, tight=True)
    skips, cskips, c, out = [], [], None, []
    for i in range(spec.nblocks):
        skip = cs = None
        if i > spec.half:
            skip, cs = skips.pop(), cskips.pop()
        taps = {}
        h, c = US.block(h, sd, spec, i, mode, skip=skip, key_scale=None if key_scale is None else key_scale[i], c_in=c, c_skip=cs,
                        taps=taps)
        out.append(taps["qkv"].to(torch.bfloat16))
        if i < spec.half:
            skips.append(h)
            cskips.append(c)
    return out


@pytest.mark.parametrize("fold", [1, 0], ids=["fold", "sep"])
def test_forward_maps_against_the_stage_model(fold):
    """Block i's map == the map kernel on the qkv the float64 stage model yields for block i, at the model-level bound."""
    from uspace_amd import _hip
    US.cpu_threads()
    with ln_fold(fold):
        for cfg, seed, kind in ((dict(TINY, clip_dim=64), 2, "workflow"), (dict(MID, clip_dim=128), 3, "stress")):
            net = US.make_net(dict(num_clip_token=77, **cfg), kind=kind, seed=seed, t2i=True)
            B = 2
            x, ctx = _inputs(net, B)
            ks = _key_scale(net, B)
            L, H = net.seq_len, net.num_heads
            really = fold and _hip.lib().uspace_gemm_part_slots_k(B * L, net.embed_dim, 64) <= 8
            qkvs = _model_qkv(net, x, ctx, "tight_fold" if really else "tight_sep", key_scale=ks)
            net = net.cuda().eval()
            win = net.token_range("image") + net.token_range("context")
            _, maps = net._run(x.cuda(), expand_t(T_VIS, B), context=ctx.cuda(), key_scale=ks.cuda(), attn_maps=win)
            for i, q in enumerate(qkvs):
                want = _hip.attention_map(q.cuda().reshape(B * L, -1).contiguous(), B, L, H, *win).cpu().numpy()
                e = AM.block_err(maps[i].cpu().numpy(), want)
                _say("model_qkv", e, f"{kind} D={net.embed_dim} block {i} fold={fold}")
                assert e <= AM.TOL["model_qkv"]


# ------------------------------------------------------------------------------------------------------------------ (d) reference fixture
def test_maps_match_the_reference_tiny(golden_dir):
    z = np.load(os.path.join(golden_dir, "attn_maps_t2i.npz"))
    zt, sd = load_sd(golden_dir, "tiny_t2i.npz")
    net = build(sd, clip_dim=64, num_clip_token=77, **TINY)
    x, ctx = dev(zt["x"]), dev(zt["ctx"])
    B = x.shape[0]
    for tag, t_edit in (("tiny_edit", 0.5), ("tiny_plain", 0.1)):
        maps = net.attention_maps(x, expand_t(T_VIS, B), ctx, **p2p_kwargs(B, t_edit)).cpu().numpy()
        assert maps.shape == (3, B, 64, 77)
        for i in range(3):
            ref = z[f"{tag}/{i}"]
            e = AM.block_err(maps[i], ref)
            _say("ref_tiny", e, f"{tag} block {i}")
            assert e <= AM.TOL["ref_tiny"]
            # the image token each text token looks at most (bounds: attention_map_cases.TOL, argmax_lead)
            am, ar = maps[i].argmax(1), ref.argmax(1)                                   # [B, 77]
            srt = np.sort(ref, axis=1)
            top, lead = srt[:, -1], (srt[:, -1] - srt[:, -2]) / srt[:, -1]
            at_ours = np.take_along_axis(ref, am[:, None, :], 1)[:, 0]
            clear = lead >= AM.TOL["argmax_lead"]
            print(f"MEASURED argmax {tag} block {i}: {int((am != ar).sum())} of {am.size} differ ({int((am != ar)[clear].sum())} of the "
                  f"{int(clear.sum())} clear leads), worst share of the top given up {float(((top - at_ours) / top).max()):.3e}")
            assert clear.sum() >= 100, "the fixture must hold clear leads, or this checks nothing"
            assert (am == ar)[clear].all() and ((top - at_ours) <= AM.TOL["argmax_lead"] * top).all()


def test_maps_match_the_reference_S(golden_dir):
    z = np.load(os.path.join(golden_dir, "attn_maps_t2i.npz"))
    zb = np.load(os.path.join(golden_dir, "big_S_t.npz"))
    meta = json.loads(bytes(z["meta_json"]).decode())
    torch.manual_seed(1234)
    net = build(clip_dim=768, num_clip_token=77, **COMMON, **S_CFG)
    x, ctx = dev(zb["x"]), dev(zb["ctx"])
    B = x.shape[0]
    maps = net.attention_maps(x, expand_t(T_VIS, B), ctx, **p2p_kwargs(B, 0.5)).cpu().numpy()
    assert maps.shape == (17, B, 256, 77)
    for i in meta["S_blocks"]:
        e = AM.block_err(maps[i], z[f"S_edit/{i}"])
        _say("ref_S", e, f"S_edit block {i}")
        assert e <= AM.TOL["ref_S"]


# ------------------------------------------------------------------------------------------------------------------ (e) vis_am_path
def test_forward_writes_the_pictures_and_keeps_its_prediction(golden_dir, tmp_path):
    from PIL import Image
    from uspace_amd.tools import utils_t2i
    zt, sd = load_sd(golden_dir, "tiny_t2i.npz")
    net = build(sd, clip_dim=64, num_clip_token=77, **TINY)
    x, ctx = dev(zt["x"]), dev(zt["ctx"])
    B = x.shape[0]
    prompts = ["a red cat", "a dog on a hill", "snow"]
    kw = p2p_kwargs(B, caption_list=prompts, tokenizer=ToyTokenizer())
    plain, _ = net(x, expand_t(T_VIS, B), ctx, **kw)
    out, aux = net(x, expand_t(T_VIS, B), ctx, vis_am_path=str(tmp_path / "am"), **kw)
    assert aux is None and torch.equal(plain, out)
    names = sorted(os.listdir(tmp_path / "am"))
    assert names == sorted(f"{p}_block{i}_time0.30.png" for p in prompts for i in range(3))
    maps = net.attention_maps(x, expand_t(T_VIS, B), ctx, **kw).cpu().numpy()
    for b, p in enumerate(prompts):
        n_tok = len(p.split()) + 2
        img = np.asarray(Image.open(tmp_path / "am" / f"{p}_block1_time0.30.png"))
        xs, width, height = utils_t2i.tile_offsets(n_tok)
        assert img.shape == (height, width, 3)
        tiles = utils_t2i.cross_attention_tiles(maps[1, b][:, :n_tok], 8)
        for j, x0 in enumerate(xs):
            np.testing.assert_array_equal(img[:256, x0:x0 + 256], tiles[j])
    net(x, expand_t(0.33, B), ctx, vis_am_path=str(tmp_path / "none"), **kw)          # not one of the nine digits
    assert not os.path.exists(tmp_path / "none")


# ------------------------------------------------------------------------------------------------------------------ (f) hipGraph
def test_maps_between_two_graph_replays(golden_dir):
    zt, sd = load_sd(golden_dir, "tiny_t2i.npz")
    net = build(sd, clip_dim=64, num_clip_token=77, **TINY)
    x, ctx = dev(zt["x"]), dev(zt["ctx"])
    B = x.shape[0]
    t = torch.tensor(T_VIS, dtype=torch.float32, device="cuda")           # 0-d: the graph path's timestep form
    eager, _ = net(x, t, ctx)
    net.use_graph = True
    first, _ = net(x, t, ctx)
    assert len(net._graphs) == 1
    maps = net.attention_maps(x, t, ctx)
    assert len(net._graphs) == 1, "a maps evaluation must not capture a graph"
    second, _ = net(x, t, ctx)
    torch.cuda.synchronize()
    assert torch.equal(first, second) and torch.equal(first, eager)
    net.use_graph = False
    assert torch.equal(maps, net.attention_maps(x, t, ctx))
