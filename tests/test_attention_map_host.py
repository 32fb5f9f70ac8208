"""CPU side of the attention-map feature: the bounds of tests/test_gpu_attention_map.py separate every fault of
tests/attention_map_cases.py from the true reference; the token-window names; the ``vis_am_path`` flow of ``UViT.forward`` with the HIP
call stubbed and a toy tokenizer; the heat tiles against the reference's formula (tools/utils_t2i.py:176-183) evaluated here; the new
entry points in the header, the library and the binding."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

from tests import attention_map_cases as AM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = dict(img_size=16, patch_size=2, in_chans=4, embed_dim=64, depth=2, num_heads=1, mlp_ratio=4,
            qkv_bias=False, mlp_time_embed=False)


# ------------------------------------------------------------------------------------------------------------------ bounds vs faults
def test_bounds_are_set_and_cases_cover_the_issue():
    for k, v in AM.TOL.items():
        assert v is not None and 0 < v < 1e-2, k
    assert {c[1] for c in AM.CASES} >= set(AM.REQUIRED_L) and {c[2] for c in AM.CASES} >= set(AM.REQUIRED_H)
    assert {c[3] for c in AM.CASES} >= set(AM.REQUIRED_WINDOWS)
    for B, L, H, win, _ in AM.CASES:
        q0, nq, k0, nk = AM.window(win, L)
        assert 0 <= q0 and nq >= 1 and q0 + nq <= L and 0 <= k0 and nk >= 1 and k0 + nk <= L


def _small(case):
    B, L, H, win, data = case
    return B * H * L * L <= 2e7


@pytest.mark.parametrize("fault", sorted(AM.PERTURBED))
def test_every_fault_misses_the_kernel_bounds(fault):
    fn, data_sets, needs = AM.PERTURBED[fault]
    seen = set()
    for case in AM.CASES:
        B, L, H, win, data = case
        w = AM.window(win, L)
        if data not in data_sets or not needs(B, L, H, w) or not _small(case):
            continue
        qkv = AM.make_qkv(B, L, H, data)
        ref = AM.reference(qkv, H, w).numpy()
        bad = fn(qkv, H, w, AM.fault_key_scale(B, L, w)).numpy()
        r, e = AM.row_err(bad, ref), AM.elem_err(bad, ref)
        assert r > AM.TOL["map_row"] and e > AM.TOL["map_elem"], f"{fault} hides inside the bounds at {AM.case_id(case)}: {r:.3e}, {e:.3e}"
        seen.add(data)
    assert seen == set(data_sets), f"{fault}: no case on {set(data_sets) - seen}"


@pytest.mark.parametrize("case", [c for c in AM.CASES if _small(c)], ids=AM.case_id)
def test_true_reference_lies_inside_the_kernel_bounds(case):
    """The map of the same softmax evaluated by torch on the CPU in fp32 -- the precision the kernel works in, not the kernel -- stays
    inside the row bound the GPU measurement set: the bound is not below what fp32 arithmetic itself costs (worst here 4.6e-6 of the
    8.2e-6).  Rows of the full float64 map sum to 1."""
    B, L, H, win, data = case
    w = AM.window(win, L)
    qkv = AM.make_qkv(B, L, H, data)
    ref = AM.reference(qkv, H, w)
    if win == "full":
        assert float((ref.sum(2) - 1.0).abs().max()) < 1e-12
    f32 = AM.reference(qkv, H, w, dtype=torch.float32)
    assert AM.row_err(f32, ref) <= AM.TOL["map_row"]


# ------------------------------------------------------------------------------------------------------------------ windows
def test_token_ranges_and_argument_errors():
    from uspace_amd.tools import utils_t2i
    from uspace_amd.tools.utils_uvit import get_nnet
    net = get_nnet("uvit_t2i", clip_dim=64, num_clip_token=77, **TINY)
    assert net.token_range("time") == (0, 1) and net.token_range("context") == (1, 77)
    assert net.token_range("image") == (78, 64) and net.token_range("all") == (0, 142)
    assert net.token_range((5, 9)) == (5, 9)
    assert utils_t2i.token_range("image", 77, 256) == (78, 256)
    for bad in ("pixels", (0, 0), (-1, 4), (140, 3), 5, (1, 2, 3)):
        with pytest.raises(ValueError):
            net.token_range(bad)
    assert utils_t2i.VIS_DIGITS == tuple(f"{k / 10:.2f}" for k in range(1, 10))


def test_run_rejects_a_window_outside_the_tokens(monkeypatch):
    from uspace_amd import _hip
    from uspace_amd.tools.utils_uvit import get_nnet
    monkeypatch.setattr(_hip, "require_device", lambda *a, **k: None)
    net = get_nnet("uvit_t2i", clip_dim=64, num_clip_token=77, **TINY)
    for w in ((0, 0, 0, 1), (0, 143, 0, 1), (-1, 1, 0, 1), (0, 1, 141, 2)):
        with pytest.raises(ValueError):
            net._run(torch.zeros(1, 4, 16, 16), torch.zeros(1), context=None, attn_maps=w)
    out, maps = net._run(torch.zeros(0, 4, 16, 16), torch.zeros(0), context=None, attn_maps=(78, 64, 1, 77))
    assert out.shape == (0, 4, 16, 16) and maps.shape == (3, 0, 64, 77)


def test_new_entry_points_are_declared_exported_and_bound():
    from uspace_amd import _hip
    hdr = open(os.path.join(ROOT, "include", "uspace_hip.h")).read()
    declared = set(re.findall(r"USPACE_API\s+[\w\s\*]+?\b(uspace_\w+)\s*\(", hdr))
    lib = ctypes.CDLL(os.path.join(ROOT, "uspace_amd", "libuspace_hip.so"))
    for name in ("uspace_attention_map_bf16", "uspace_uvit_forward_maps"):
        assert name in declared and name in _hip.SIGNATURES and hasattr(lib, name)
    assert len(_hip.SIGNATURES["uspace_attention_map_bf16"][1]) == 10 and len(_hip.SIGNATURES["uspace_uvit_forward_maps"][1]) == 12
    assert len(_hip.UvitIO._fields_) == 10 and _hip.ABI_VERSION == 11
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "uspace_attention_map_bf16" in doc and "uspace_uvit_forward_maps" in doc
    # host-side argument checks of the kernel entry: refused before anything is launched
    fn = _hip.lib().uspace_attention_map_bf16
    one = ctypes.c_void_p(16)
    for args in ((1, 20, 1, -1, 4, 0, 4), (1, 20, 1, 0, 0, 0, 4), (1, 20, 1, 17, 4, 0, 4), (1, 20, 1, 0, 4, 19, 2), (1, 337, 1, 0, 1, 0, 1),
                 (0, 20, 1, 0, 1, 0, 1), (1, 20, 0, 0, 1, 0, 1)):
        assert fn(one, one, *args, None) == -1, args
    assert fn(None, one, 1, 20, 1, 0, 1, 0, 1, None) == -1


def test_map_kernel_uses_no_scratch():
    import importlib.util
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    ks = [k for k in kr.kernels() if "attention_map_kernel" in k["name"]]
    assert len(ks) == 4
    for k in ks:
        assert k["scratch"] == 0 and k["vgpr"] + k["agpr"] <= 512 and k["wg"] == 64, k


# ------------------------------------------------------------------------------------------------------------------ tiles
def test_cross_attention_tiles_follow_the_reference_formula():
    from uspace_amd.tools import utils_t2i
    rng = np.random.default_rng(3)
    for grid, n_tok in ((8, 5), (16, 7)):
        m = rng.random((grid * grid, n_tok)).astype(np.float32) ** 4 * 1e-2
        tiles = utils_t2i.cross_attention_tiles(m, grid)
        assert tiles.shape == (n_tok, 256, 256, 3) and tiles.dtype == np.uint8
        am = torch.from_numpy(m).reshape(grid, grid, n_tok)                  # "(a b) t -> a b t"
        for i in range(n_tok):
            # torch fp32 arithmetic as the reference has it: 255 * m / max(m), three equal channels, truncation to uint8,
            # PIL's default resize
            heat = (255 * am[..., i] / am[..., i].max())[..., None].expand(grid, grid, 3)
            want = np.array(Image.fromarray(heat.numpy().astype(np.uint8)).resize((256, 256)))
            np.testing.assert_array_equal(tiles[i], want)
        assert tiles.max() == 255
    with pytest.raises(ValueError):
        utils_t2i.cross_attention_tiles(np.zeros((60, 3), np.float32), 8)


# ------------------------------------------------------------------------------------------------------------------ vis_am_path
class ToyTokenizer:
    """One id per whitespace word between a begin and an end token; decode gives the word back."""

    def __init__(self):
        self.words = ["<s>", "</s>"]
        self.calls = 0

    def encode(self, text):
        self.calls += 1
        ids = [0]
        for w in text.split():
            if w not in self.words:
                self.words.append(w)
            ids.append(self.words.index(w))
        return ids + [1]

    def decode(self, i):
        return self.words[int(i)]


@pytest.fixture
def stubbed_net(monkeypatch):
    """The tiny T2I module on the CPU with its single HIP call replaced: ``_run`` returns a seeded prediction and, when asked, seeded
    maps, and records how it was called."""
    from uspace_amd import _hip
    from uspace_amd.tools.utils_uvit import get_nnet
    monkeypatch.setattr(_hip, "require_device", lambda *a, **k: None)
    net = get_nnet("uvit_t2i", clip_dim=64, num_clip_token=77, **TINY)
    net.calls = []

    def fake_run(x, timesteps, context=None, key_scale=None, attn_maps=None, **kw):
        net.calls.append(dict(attn_maps=attn_maps, key_scale=key_scale))
        out = torch.full_like(x, 0.5)
        if attn_maps is None:
            return out
        g = torch.Generator().manual_seed(11)
        q0, nq, k0, nk = attn_maps
        net.maps = torch.rand(net.depth + 1, x.shape[0], nq, nk, generator=g) ** 3 / 142.0
        return out, net.maps

    net._run = fake_run
    return net


def _kw(B, **more):
    ids = [np.array([3, 5], dtype=np.int64), np.array([], dtype=np.int64), np.array([0, 76, 76], dtype=np.int64)]
    kw = dict(dissect_name="p2p", fm_direction="decode", t_edit=0.5, block_id="all",
              token_kwargs=dict(token_dissect="p2p_rescale", p2p_multiplier=3.0), target_context_ids=[a.copy() for a in ids[:B]],
              caption_list=["a red cat", "a dog on a hill", "snow"][:B], tokenizer=ToyTokenizer())
    kw.update(more)
    return kw


def test_vis_am_path_end_to_end(stubbed_net, tmp_path):
    from uspace_amd.tools import utils_t2i
    net = stubbed_net
    B = 3
    x, ctx = torch.zeros(B, 4, 16, 16), torch.zeros(B, 77, 64)
    path = tmp_path / "deep" / "am"                                              # created if missing
    kw = _kw(B, vis_am_path=str(path))
    out, aux = net(x, torch.full((B,), 0.3), ctx, **kw)
    assert aux is None and out.shape == x.shape
    assert net.calls[-1]["attn_maps"] == (78, 64, 1, 77) and net.calls[-1]["key_scale"] is not None
    prompts = kw["caption_list"]
    assert sorted(os.listdir(path)) == sorted(f"{p}_block{i}_time0.30.png" for p in prompts for i in range(3))
    maps = net.maps.numpy()
    for b, p in enumerate(prompts):
        n_tok = len(p.split()) + 2
        for blk in range(3):
            img = np.asarray(Image.open(path / f"{p}_block{blk}_time0.30.png").convert("RGB"))
            xs, width, height = utils_t2i.tile_offsets(n_tok)
            assert len(xs) == n_tok and img.shape == (height, width, 3) and height == 256 + 51 and xs[1] == 256 + 6
            tiles = utils_t2i.cross_attention_tiles(maps[blk, b][:, :n_tok], 8)
            for j, x0 in enumerate(xs):
                np.testing.assert_array_equal(img[:256, x0:x0 + 256], tiles[j])
            for x0 in xs[1:]:
                assert (img[:, x0 - 6:x0] == 255).all(), "white gap between two tiles"
            assert (img[256:] != 255).any(), "labels are drawn under the tiles"
    # a later evaluation with the same digit overwrites
    before = {n: os.path.getmtime(path / n) for n in os.listdir(path)}
    net(x, torch.full((B,), 0.304), ctx, **kw)
    assert sorted(os.listdir(path)) == sorted(before)


def test_pictures_only_at_the_nine_digits(stubbed_net, tmp_path):
    net = stubbed_net
    B = 2
    x, ctx = torch.zeros(B, 4, 16, 16), torch.zeros(B, 77, 64)
    kw = _kw(B, vis_am_path=str(tmp_path / "am"), t_edit=1.0)
    for k in range(0, 101):
        t = np.float32(k) / np.float32(100)
        net(x, torch.full((B,), float(t)), ctx, _t_host=float(t), **kw)
    digits = sorted({n.rsplit("_time", 1)[1][:-4] for n in os.listdir(tmp_path / "am")})
    assert digits == [f"{k / 10:.2f}" for k in range(1, 10)]
    assert len(os.listdir(tmp_path / "am")) == 9 * B * 3
    assert sum(1 for c in net.calls if c["attn_maps"] is not None) == 9


def test_nothing_written_elsewhere(stubbed_net, tmp_path):
    net = stubbed_net
    B = 2
    x, ctx, t = torch.zeros(B, 4, 16, 16), torch.zeros(B, 77, 64), torch.full((B,), 0.3)
    p = tmp_path / "am"
    net(x, t, ctx, **_kw(B, vis_am_path=str(p), fm_direction="encode"))
    net(x, t, ctx, **_kw(B))                                                     # no vis_am_path
    net(x, t, ctx, **_kw(B, vis_am_path=None))
    net(x, t, ctx, vis_am_path=str(p), caption_list=["a", "b"])                 # no dissect_name
    net(x, t, ctx, **_kw(B, vis_am_path=str(p), dissect_name="none"))
    assert not p.exists() and all(c["attn_maps"] is None for c in net.calls)
    maps = net.attention_maps(x, t, ctx, queries="image", keys="image", **_kw(B, vis_am_path=str(p)))
    assert not p.exists() and maps.shape == (3, B, 64, 64) and net.calls[-1]["attn_maps"] == (78, 64, 78, 64)


def test_writer_contract(tmp_path):
    from uspace_amd.tools import utils_t2i
    tok = ToyTokenizer()
    maps = np.random.default_rng(1).random((2, 1, 64, 77)).astype(np.float32)
    assert utils_t2i.vis_attention_map(maps, "0.35", vis_am_path=str(tmp_path), caption_list=["x"], tokenizer=tok) == []
    assert utils_t2i.vis_attention_map(maps, "0.30", caption_list=["x"], tokenizer=tok) == []
    assert tok.calls == 0 and os.listdir(tmp_path) == []
    out = utils_t2i.vis_attention_map(torch.from_numpy(maps), "0.90", vis_am_path=str(tmp_path), caption_list=["x y"], tokenizer=tok)
    assert [os.path.basename(p) for p in out] == ["x y_block0_time0.90.png", "x y_block1_time0.90.png"] and tok.calls == 1
    with pytest.raises(ValueError):
        utils_t2i.vis_attention_map(maps, "0.30", vis_am_path=str(tmp_path), caption_list=[], tokenizer=tok)
