"""CPU side of classifier-free guidance: the new entry points in the header, the library, the binding and INTEGRATION.md; their argument
errors, refused before anything is launched; the modules' ValueErrors, raised before any device work; and the bounds of
tests/test_gpu_cfg.py against the wrong formulas of tests/cfg_cases.py on the CPU oracle's predictions for that test's inputs."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import cfg_cases as CC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("uspace_cfg_combine", "uspace_uvit_cfg_workspace_bytes", "uspace_uvit_forward_cfg")


# ------------------------------------------------------------------------------------------------------------------ ABI
def test_entry_points_are_declared_exported_bound_and_documented():
    from uspace_amd import _hip
    hdr = open(os.path.join(ROOT, "include", "uspace_hip.h")).read()
    declared = set(re.findall(r"USPACE_API\s+[\w\s\*]+?\b(uspace_\w+)\s*\(", hdr))
    lib = ctypes.CDLL(os.path.join(ROOT, "uspace_amd", "libuspace_hip.so"))
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert name in declared and name in _hip.SIGNATURES and hasattr(lib, name) and name in doc, name
    assert len(_hip.SIGNATURES["uspace_cfg_combine"][1]) == 7 and len(_hip.SIGNATURES["uspace_uvit_forward_cfg"][1]) == 12
    assert len(_hip.SIGNATURES["uspace_uvit_cfg_workspace_bytes"][1]) == 2
    assert len(_hip.UvitIO._fields_) == 10 and _hip.ABI_VERSION == 11 and _hip.lib().uspace_abi_version() == 11
    assert callable(_hip.cfg_combine) and callable(_hip.uvit_forward_cfg)


def test_combine_argument_errors_are_refused_on_the_host():
    from uspace_amd import _hip
    fn = _hip.lib().uspace_cfg_combine
    one = ctypes.c_void_p(16)
    assert fn(None, None, 0.4, one, 1, 4, None) == -1
    assert fn(one, None, 0.4, None, 1, 4, None) == -1
    for B, per in ((0, 4), (-1, 4), (1, 0), (1, -4)):
        assert fn(one, one, 0.4, one, B, per, None) == -1, (B, per)


def _cfg(**over):
    from uspace_amd import _hip
    kw = dict(img_size=16, patch_size=2, in_chans=4, embed_dim=64, depth=2, num_heads=1, mlp_hidden=256, n_extra=77, clip_dim=64,
              time_first=1)
    kw.update(over)
    return _hip.UvitConfig(*[kw[n] for n, _ in _hip.UvitConfig._fields_])


def test_forward_cfg_argument_errors_are_refused_on_the_host():
    from uspace_amd import _hip
    L = _hip.lib()
    one = ctypes.c_void_p(16)
    big = ctypes.c_size_t(1 << 40)

    def io(**over):
        kw = dict(x=16, t=16, t_stride=0, context=16, mid_delta=None, mid_scale=0.0, mid_tap=None, key_scale=None, out=16,
                  mid_row_scale=None)
        kw.update(over)
        return _hip.UvitIO(*[kw[n] for n, _ in _hip.UvitIO._fields_])

    def call(cfg, io_, B=2, uncond=one, blob=one, ws=one):
        return L.uspace_uvit_forward_cfg(ctypes.byref(cfg), blob, ws, big, ctypes.byref(io_), B, uncond, 0, 0.4, None, None, None)

    t2i, label, plain = _cfg(), _cfg(n_extra=1, clip_dim=0, time_first=0), _cfg(n_extra=0, clip_dim=0)
    assert call(plain, io(context=None)) == -1 and call(plain, io()) == -1          # nothing to drop
    for cfg in (t2i, label):
        assert call(cfg, io(mid_tap=16)) == -1
        assert call(cfg, io(), uncond=None) == -1
        assert call(cfg, io(), B=0) == -1 and call(cfg, io(), B=-3) == -1
        assert call(cfg, io(x=None)) == -1 and call(cfg, io(t=None)) == -1 and call(cfg, io(out=None)) == -1
        assert call(cfg, io(context=None)) == -1
        assert call(cfg, io(), blob=None) == -1 and call(cfg, io(), ws=None) == -1
    assert call(_cfg(embed_dim=60), io()) == -1
    # the workspace is a plain forward's at 2B rows and the 2B predictions behind it; too small a one is refused as such
    for cfg in (t2i, label):
        for B in (1, 3):
            want = L.uspace_uvit_workspace_bytes(ctypes.byref(cfg), 2 * B) + 2 * B * 4 * 16 * 16 * 4
            got = L.uspace_uvit_cfg_workspace_bytes(ctypes.byref(cfg), B)
            assert want <= got < want + 256
            assert L.uspace_uvit_forward_cfg(ctypes.byref(cfg), one, one, got - 1, ctypes.byref(io()), B, one, 0, 0.4, None, None, None) == -3
    assert L.uspace_uvit_cfg_workspace_bytes(ctypes.byref(t2i), 0) == 0 and L.uspace_uvit_cfg_workspace_bytes(ctypes.byref(_cfg(embed_dim=60)), 2) == 0


# ------------------------------------------------------------------------------------------------------------------ modules
@pytest.fixture
def cpu_nets(monkeypatch):
    """The tiny modules on the CPU; any call that got as far as the device would fail loudly, with an error that is no ValueError."""
    def no_device(*a, **k):
        raise AssertionError("device work was reached")
    t2i, cls = CC.make("tiny_t2i"), CC.make("tiny_cls")
    for net in (t2i, cls):
        monkeypatch.setattr(net, "_run", no_device)
    return t2i, cls


def test_t2i_value_errors_come_before_any_device_work(cpu_nets):
    net, _ = cpu_nets
    B = 3
    x, ctx, t = torch.zeros(B, 4, 16, 16), torch.zeros(B, 77, 64), torch.full((B,), 0.3)
    empty = torch.zeros(77, 64)
    with pytest.raises(ValueError, match="empty_context"):
        net(x, t, ctx, cfg_scale=0.4)
    for bad in (torch.zeros(76, 64), torch.zeros(77, 32), torch.zeros(2, 77, 64), torch.zeros(77 * 64), np.zeros((1, 77, 64), np.float32)):
        with pytest.raises(ValueError, match="empty_context"):
            net(x, t, ctx, cfg_scale=0.4, empty_context=bad)
    for bad in ([0.4, 0.4], np.zeros(4, np.float32), torch.zeros(2), [], "high"):
        with pytest.raises(ValueError, match="cfg_scale"):
            net(x, t, ctx, cfg_scale=bad, empty_context=empty)
    with pytest.raises(ValueError, match="cfg_scale"):
        net.attention_maps(x, t, ctx, cfg_scale=0.4, empty_context=empty)


def test_t2i_vis_am_path_under_guidance_is_refused(cpu_nets, monkeypatch, tmp_path):
    from uspace_amd import _hip
    net, _ = cpu_nets
    monkeypatch.setattr(_hip, "require_device", lambda *a, **k: None)
    B = 2
    x, ctx = torch.zeros(B, 4, 16, 16), torch.zeros(B, 77, 64)
    kw = dict(dissect_name="p2p", fm_direction="decode", t_edit=0.5, block_id="all",
              token_kwargs=dict(token_dissect="p2p_rescale", p2p_multiplier=3.0),
              target_context_ids=[np.array([3, 5]), np.array([], dtype=np.int64)], vis_am_path=str(tmp_path / "am"))
    with pytest.raises(ValueError, match="vis_am_path"):
        net(x, torch.full((B,), 0.3), ctx, cfg_scale=0.4, empty_context=torch.zeros(77, 64), **kw)
    assert not (tmp_path / "am").exists()


def test_class_conditional_value_errors_come_before_any_device_work(cpu_nets, tmp_path):
    from uspace_amd.tools.utils_uvit import get_nnet
    _, net = cpu_nets
    B = 3
    x, t, y = torch.zeros(B, 4, 16, 16), torch.full((B,), 0.3), torch.tensor([0, 4, 9])
    for bad in (11, -1, 400):
        with pytest.raises(ValueError, match="empty_label"):
            net(x, t, y, cfg_scale=0.4, empty_label=bad)
    with pytest.raises(ValueError, match="cfg_scale"):
        net(x, t, y, cfg_scale=[0.4, 0.4])
    with pytest.raises(ValueError, match="mid read"):
        net(x, t, y, cfg_scale=0.4, edit_loc="mid", dissect_task="uspace_uvit", dissect_name="read", read_path_root=str(tmp_path),
            batch_id=0)
    assert os.listdir(tmp_path) == []
    plain = get_nnet("uvit", num_classes=-1, **{k: v for k, v in CC.NETS["tiny_cls"][0].items() if k != "num_classes"})
    with pytest.raises(ValueError, match="no label embedding"):
        plain(x, t, None, cfg_scale=0.4)


def test_guidance_scales_forms():
    from uspace_amd.libs._uvit_core import guidance_scales
    for s in (0.4, np.float32(0.4), np.float64(0.4), torch.tensor(0.4), np.array(0.4), 1):
        scale, rows = guidance_scales(s, 3)
        assert rows is None and abs(scale - float(s)) < 1e-7
    for s in ([0.0, 0.4, 7.5], (0.0, 0.4, 7.5), np.array([0.0, 0.4, 7.5])):
        scale, rows = guidance_scales(s, 3)
        assert scale == 1.0 and rows.dtype == np.float32 and rows.tolist() == [0.0, np.float32(0.4), 7.5]
    scale, rows = guidance_scales(torch.tensor([0.0, 0.4, 7.5]), 3)
    assert scale == 1.0 and torch.is_tensor(rows) and rows.numel() == 3


# ------------------------------------------------------------------------------------------------------------------ bounds vs wrong formulas
def test_reference_formula():
    vc, vu = np.array([[1.0, -2.0]]), np.array([[0.5, 1.0]])
    np.testing.assert_array_equal(CC.guided_reference(vc, vu, 0.0), vc)
    np.testing.assert_allclose(CC.guided_reference(vc, vu, -1.0), vu)
    np.testing.assert_allclose(CC.guided_reference(vc, vu, 2.0), [[2.0, -8.0]])
    two = CC.guided_reference(np.repeat(vc, 2, 0), np.repeat(vu, 2, 0), 2.0, [0.0, 0.5])
    np.testing.assert_allclose(two, [[1.0, -2.0], [1.5, -5.0]])
    assert abs(CC.module_bound(7.5) - 0.16) < 1e-12 and abs(CC.module_bound(0.4) - 0.018) < 1e-12


@pytest.mark.parametrize("wrong", sorted(CC.WRONG))
def test_every_wrong_formula_misses_the_bounds(wrong):
    """On the oracle's v_c and v_u for the inputs of the GPU module test (MID, B = 3): each wrong formula leaves the combine bound (A) at
    some element, and all but one the module bound (C) as a whole.  The one: u + s (c - u), the other convention in use, is off by
    exactly c - u, 0.11 ||v_c|| here against (C)'s 0.16 at s = 7.5 -- only (A), which the GPU tests apply to the paired predictions
    of the same call, tells it from the reference."""
    _, _, vc, vu = CC.oracle_case("mid_t2i", 3)
    s, rs = (1.0, np.array(CC.SWEEP, np.float32)) if wrong == "row_scale_of_next_sample" else (CC.S_BIG, None)
    ref = CC.guided_reference(vc, vu, s, rs)
    bad = CC.WRONG[wrong](vc, vu, s, rs)
    assert np.any(np.abs(bad - ref) > CC.combine_bound(vc, vu, s, rs)), wrong
    if wrong != "anchored_on_uncond":
        assert CC.module_err(bad, ref, vc, vu) > CC.module_bound(CC.S_BIG), wrong


def test_guidance_term_is_visible_where_the_gpu_tests_need_it():
    for name in ("mid_t2i", "tiny_cls"):
        _, _, vc, vu = CC.oracle_case(name, 3)
        assert CC.guidance_is_visible(vc, vu, CC.S_BIG), name
        # the conditional prediction alone misses the module bound by far
        assert CC.module_err(vc, CC.guided_reference(vc, vu, CC.S_BIG), vc, vu) > 3 * CC.module_bound(CC.S_BIG)


def test_new_kernels_use_no_scratch():
    import importlib.util
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    ks = [k for k in kr.kernels() if "cfg_combine" in k["name"] or "cast_bcast" in k["name"]]
    assert len(ks) == 3, [k["name"] for k in ks]
    for k in ks:
        assert k["scratch"] == 0, k
