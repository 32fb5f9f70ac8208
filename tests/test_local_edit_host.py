"""CPU side of local edits: the bounds of tests/test_gpu_local_edit.py separate every planted fault of tests/local_edit_cases.py from the
true reference by at least 2 x; the pairing logic of ``decode_local`` against a stubbed ``_run`` that records what every evaluation
receives; the ValueErrors; the three entry points in the header, the library, the binding and INTEGRATION.md."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import local_edit_cases as LE
from uspace_amd.tools import local_edit  # noqa: F401  (without the feature nothing in this file can run)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"uspace_pair_blend": 7, "uspace_mask_from_labels": 11, "uspace_mask_from_maps": 12}


# ------------------------------------------------------------------------------------------------------------------ ABI
def test_entry_points_are_declared_exported_bound_and_documented():
    from uspace_amd import _hip
    hdr = open(os.path.join(ROOT, "include", "uspace_hip.h")).read()
    declared = set(re.findall(r"USPACE_API\s+[\w\s\*]+?\b(uspace_\w+)\s*\(", hdr))
    lib = ctypes.CDLL(os.path.join(ROOT, "uspace_amd", "libuspace_hip.so"))
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name, nargs in NAMES.items():
        assert name in declared and name in _hip.SIGNATURES and hasattr(lib, name) and name in doc, name
        assert len(_hip.SIGNATURES[name][1]) == nargs, name
    assert declared == set(_hip.SIGNATURES)
    assert len(_hip.UvitIO._fields_) == 10 and _hip.ABI_VERSION == 11 and _hip.lib().uspace_abi_version() == 11
    assert callable(_hip.pair_blend) and callable(_hip.mask_from_labels) and callable(_hip.mask_from_maps)


def test_argument_errors_are_refused_on_the_host():
    from uspace_amd import _hip
    L = _hip.lib()
    one, far = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 30)
    blend = L.uspace_pair_blend
    assert blend(None, one, 1, 4, 4, far, None) == -1 and blend(one, None, 1, 4, 4, far, None) == -1 and blend(one, one, 1, 4, 4, None, None) == -1
    for B, C, cells in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4)):
        assert blend(one, one, B, C, cells, far, None) == -1, (B, C, cells)
    assert blend(one, far, 2, 4, 16, ctypes.c_void_p((1 << 20) + 64), None) == -1          # out overlaps pair without being pair
    labels = L.uspace_mask_from_labels
    ok = dict(B=1, H=16, W=16, S=4, dilate=1)
    for over in (dict(B=0), dict(S=0), dict(S=65), dict(H=18), dict(W=6), dict(H=2, W=2), dict(dilate=-1), dict(dilate=5), dict(H=16388, S=1)):
        a = dict(ok, **over)
        assert labels(one, a["B"], a["H"], a["W"], one, a["S"], a["dilate"], 0.0, 0, far, None) == -1, over
    assert labels(None, 1, 16, 16, one, 4, 1, 0.0, 0, far, None) == -1 and labels(one, 1, 16, 16, None, 4, 1, 0.0, 0, far, None) == -1
    maps = L.uspace_mask_from_maps
    ok = dict(n_blocks=3, R=2, G=8, nk=77, patch=2)
    for over in (dict(n_blocks=0), dict(R=0), dict(G=0), dict(G=65), dict(nk=0), dict(patch=0), dict(patch=17)):
        a = dict(ok, **over)
        assert maps(one, a["n_blocks"], a["R"], a["G"], a["nk"], one, one, a["patch"], 0.3, 0, far, None) == -1, over
    assert maps(one, 3, 2, 8, 77, None, one, 2, 0.3, 0, far, None) == -1 and maps(one, 3, 2, 8, 77, one, one, 2, 0.3, 0, None, None) == -1


def test_new_kernels_use_no_scratch():
    import importlib.util
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    ks = [k for k in kr.kernels() if any(n in k["name"] for n in ("pair_blend_kernel", "mask_from_labels_kernel", "mask_from_maps_kernel"))]
    assert len(ks) == 4, [k["name"] for k in ks]
    for k in ks:
        assert k["scratch"] == 0 and k["vgpr"] + k["agpr"] <= 128 and k["lds"] <= 64 * 1024, k


# ------------------------------------------------------------------------------------------------------------------ references and bounds
def test_bounds_are_set_and_cases_cover_the_issue():
    assert TOL_ok(LE.TOL["maps_soft"]) and LE.TOL["maps_soft"] < LE.maps_apriori(LE.MAPS_TOL_CASE)
    assert TOL_ok(LE.TOL["solve_rel_l2"]) and LE.TOL["solve_rel_l2"] <= LE.SOLVE_CAP
    assert LE.TOL["blend_ulp"] == 1.0 and LE.TOL["blend_general"] == 2.0 ** -24
    assert LE.BLEND_SHAPES == [(1, 4, 1), (2, 3, 49), (2, 4, 25), (3, 4, 256), (5, 4, 1024)]
    assert {c[2] for c in LE.MAPS_CASES} == {1, 8, 16} and {c[4] for c in LE.MAPS_CASES} == {1, 2, 4}
    assert {c[3] for c in LE.MAPS_CASES} == {1, 77} and {c[0] for c in LE.MAPS_CASES} == {1, 3, 17} and LE.MAPS_TOL_CASE in LE.MAPS_CASES
    assert {c[3] for c in LE.LABEL_CASES} >= {1, 4, 16} and {c[4] for c in LE.LABEL_CASES} == {0, 1, 2} and max(c[0] for c in LE.LABEL_CASES) == 3
    assert any(c[1] == c[3] and c[2] == c[3] for c in LE.LABEL_CASES) and any(c[1] == 8 * c[3] for c in LE.LABEL_CASES)
    assert any(c[1] != c[2] for c in LE.LABEL_CASES)


def TOL_ok(v):
    return v is not None and 0 < v < 1e-2


def test_blend_reference_formula():
    pair = np.array([[[1.0, -2.0, 3.0, 4.0, -0.0]], [[5.0, 6.0, -7.0, 8.0, 9.0]]], np.float32)        # B = 1, C = 1, cells = 5
    mask = np.array([[0.0, 1.0, np.nan, 0.25, -0.5]], np.float32)
    out = LE.blend_reference(pair, mask)
    np.testing.assert_array_equal(out[0], pair[0])
    np.testing.assert_array_equal(out[1], [[1.0, 6.0, 3.0, 5.0, -0.0]])
    assert np.signbit(out[1, 0, 4])
    assert LE.ulps(np.float32(1.0) + np.spacing(np.float32(1.0)), 1.0) == 1.0
    # the counterexample of the bound's note: 1 ulp of the result is not derivable on arbitrary operands
    s, e, m = np.float32(1.0), np.float32(-1.0000001), np.float32(0.5)
    got = np.float32(np.float64(m) * np.float64(np.float32(e - s)) + np.float64(s))
    ref = LE.blend_reference(np.array([[[s]], [[e]]]), np.array([[m]]))[1, 0, 0]
    assert LE.ulps(got, ref) > 1e3 and abs(got - ref) <= LE.blend_general_bound(np.array([[[s]], [[e]]]), np.array([[m]]))[0, 0, 0]


@pytest.mark.parametrize("shape", LE.BLEND_SHAPES, ids=str)
def test_fp32_blend_lies_inside_its_bounds(shape):
    """The kernel's arithmetic evaluated here (fp32 subtraction; the fused multiply-add as one rounding of the float64 value, which is
    exact enough: the product has 48 bits): within 1 ulp on the near operands, within the derived bound on the general ones."""
    for near in (True, False):
        pair, mask = LE.blend_inputs(shape, near=near)
        B = shape[0]
        s, e, m = pair[:B], pair[B:], mask.reshape(B, 1, -1)
        fma = (m.astype(np.float64) * (e - s).astype(np.float64) + s.astype(np.float64)).astype(np.float32)
        got = np.where(m >= 1, e, np.where(~(m > 0), s, fma))
        ref = LE.blend_reference(pair, mask)[B:]
        if near:
            assert LE.ulps(got, ref).max() <= LE.TOL["blend_ulp"]
        assert np.all(np.abs(got - ref) <= LE.blend_general_bound(pair, mask) * (1 + 1e-9))


@pytest.mark.parametrize("fault", sorted(k for k, v in LE.PERTURBED.items() if v[0] == "blend"))
def test_blend_faults_miss_the_bounds(fault):
    fn = LE.PERTURBED[fault][1]
    seen = 0
    for shape in LE.BLEND_SHAPES:
        B, C, cells = shape
        if (fault == "mask_row_stride" and B < 2) or (fault == "mask_channel0_only" and C < 2):
            continue
        for near in (True, False):
            pair, mask = LE.blend_inputs(shape, near=near)
            ref, bad = LE.blend_reference(pair, mask), fn(pair, mask)
            if near:
                assert LE.ulps(bad[B:], ref[B:]).max() > 2 * LE.TOL["blend_ulp"], (fault, shape)
            assert np.any(np.abs(bad - ref)[B:] > 2 * LE.blend_general_bound(pair, mask)) or not np.array_equal(bad[:B], ref[:B]), (fault, shape)
            seen += 1
    assert seen >= 6


@pytest.mark.parametrize("fault", sorted(k for k, v in LE.PERTURBED.items() if v[0] == "labels"))
def test_label_faults_change_the_exact_mask(fault):
    """The label mask is exact, so its bound is 0: a fault has to change some cell, of the soft and of a binary mask."""
    seen = 0
    for case in LE.LABEL_CASES:
        B, H, W, S, dilate = case
        if (fault == "share_over_S2" and (H // S) * (W // S) == S * S) or (fault == "dilation_wraps" and (dilate == 0 or S <= 2 * dilate + 1)):
            continue
        lab, member = LE.label_maps(case), LE.member_of()
        soft = LE.labels_mask_reference(lab, member, S, dilate, 0.0, True)
        assert not np.array_equal(LE.labels_mask_reference(lab, member, S, dilate, 0.0, True, fault=fault), soft), (fault, case)
        thr = 0.5
        hard = LE.labels_mask_reference(lab, member, S, dilate, thr, False)
        if fault == "dilation_wraps" or H // S > 1:
            assert not np.array_equal(LE.labels_mask_reference(lab, member, S, dilate, thr, False, fault=fault), hard), (fault, case)
        seen += 1
    assert seen >= 3


def test_label_reference_properties():
    case = (3, 32, 64, 4, 1)
    lab, member = LE.label_maps(case), LE.member_of()
    soft0 = LE.labels_mask_reference(lab, member, 4, 0, 0.0, True)
    assert soft0.dtype == np.float32 and 0 < soft0.max() <= 1 and soft0.min() == 0 and np.any((soft0 > 0) & (soft0 < 1))
    assert soft0[0, 0, 0] == 1.0 and soft0[1, -1, -1] == 1.0                                  # the region touches the border
    soft1 = LE.labels_mask_reference(lab, member, 4, 1, 0.0, True)
    assert np.all(soft1 >= soft0) and np.any(soft1 > soft0)
    assert LE.labels_mask_reference(lab, np.zeros(256, np.uint8), 4, 1, 0.0, False).max() == 0
    assert LE.labels_mask_reference(lab, np.ones(256, np.uint8), 4, 0, 0.0, True).min() == 1


@pytest.mark.parametrize("fault", sorted(k for k, v in LE.PERTURBED.items() if v[0] == "maps"))
def test_maps_faults_miss_the_bounds(fault):
    seen = 0
    for case in LE.MAPS_CASES:
        n_blocks, R, G, nk, patch = case
        if G == 1 or (fault in ("batch_max", "cols_wrong_branch") and R < 2) or (fault == "patch_transposed" and G < 2):
            continue
        maps, w, cols = LE.maps_inputs(case)
        _, ref = LE.maps_mask_reference(maps, w, cols, G, patch, LE.MAPS_THR, True)
        _, bad = LE.maps_mask_reference(maps, w, cols, G, patch, LE.MAPS_THR, True, fault=fault)
        assert np.abs(bad - ref).max() > 2 * LE.TOL["maps_soft"], (fault, case)
        hard, norm = LE.maps_mask_reference(maps, w, cols, G, patch, LE.MAPS_THR, False)
        hard_bad, _ = LE.maps_mask_reference(maps, w, cols, G, patch, LE.MAPS_THR, False, fault=fault)
        firm = ~LE.excused(norm, LE.MAPS_THR, LE.TOL["maps_soft"])
        assert np.any(hard_bad[firm] != hard[firm]), (fault, case)
        seen += 1
    assert seen >= 3


@pytest.mark.parametrize("case", LE.MAPS_CASES, ids=str)
def test_maps_inputs_keep_the_reference_clear_of_the_threshold(case):
    """At most 1 % of the cells of the binary reference lie within the bound of the threshold (there either side is right); the
    reference of a row with all-zero cols is all zero; an fp32 evaluation of the same sums stays inside the bound."""
    n_blocks, R, G, nk, patch = case
    maps, w, cols = LE.maps_inputs(case)
    hard, norm = LE.maps_mask_reference(maps, w, cols, G, patch, LE.MAPS_THR, False)
    assert LE.excused(norm, LE.MAPS_THR, LE.TOL["maps_soft"]).mean() <= LE.MAPS_EXCUSED_SHARE
    assert LE.TOL["maps_soft"] < LE.maps_apriori(LE.MAPS_TOL_CASE)
    for r in range(R):
        if not cols[r].any():
            assert hard[r].max() == 0 and norm[r].max() == 0
        elif G > 1:
            assert 0 < hard[r].mean() < 1, (case, r)                       # neither empty nor full: the threshold bites
    assert R <= 2 or not cols[R - 1].any()
    a32 = np.zeros((R, G * G), np.float32)
    for blk in range(n_blocks):
        inner = np.zeros((R, G * G), np.float32)
        for j in range(nk):
            inner = (inner + cols[:, j][:, None] * maps[blk, :, :, j]).astype(np.float32)
        a32 = (a32 + w[blk] * inner).astype(np.float32)
    pooled = LE._window_max(a32.reshape(R, G, G), 1)
    top = pooled.reshape(R, -1).max(axis=1)
    n32 = np.where(top[:, None, None] > 0, pooled / np.where(top > 0, top, 1)[:, None, None], 0).astype(np.float32)
    n32 = np.repeat(np.repeat(n32, patch, axis=1), patch, axis=2)
    assert np.abs(n32 - norm).max() <= LE.maps_apriori(case)


def test_solve_faults_miss_the_bound():
    """On the CPU oracle, SOLVE_CASE: blending the state instead of the velocity, and swapping the halves, leave the solve bound by
    more than 2 x; the masks of the solve tests are what they say."""
    ref = LE.oracle_solve()
    for fault in ("state_blended", "halves_swapped"):
        r = LE.rel_l2(LE.oracle_solve(fault), ref)
        assert r > 2 * LE.TOL["solve_rel_l2"], (fault, r)
    m = LE.soft_bands(2)
    assert set(np.unique(m)) == {0.0, 0.5, 1.0} and not np.array_equal(m[0], m[1])
    assert LE.half_plane(2).mean() == 0.5 and LE.checkerboard(2).mean() == 0.5


def test_euler_reference_keeps_the_outside_and_equals_the_plain_solves_at_the_ends():
    rng = np.random.default_rng(0)
    A = rng.standard_normal((64, 64)) / 8.0
    z = rng.standard_normal((2, 4, 4, 4)).astype(np.float32)
    src = lambda t, x: np.tanh(x.reshape(2, -1) @ A).reshape(x.shape).astype(np.float32)
    edt = lambda t, x: (src(t, x) + np.float32(0.7) * np.cos(x)).astype(np.float32)
    m = LE.half_plane(2, 4)
    edited, source = LE.euler_blend_reference(src, edt, z, m)
    out = np.broadcast_to(m[:, None] == 0, z.shape)
    np.testing.assert_array_equal(edited[out], source[out])
    assert np.all(edited[~out] != source[~out])
    e0, s0 = LE.euler_blend_reference(src, edt, z, np.zeros_like(m))
    np.testing.assert_array_equal(e0, s0)
    e1, _ = LE.euler_blend_reference(src, edt, z, np.ones_like(m))
    plain, _ = LE.euler_blend_reference(edt, edt, z, np.ones_like(m))
    np.testing.assert_array_equal(e1, plain)


# ------------------------------------------------------------------------------------------------------------------ pairing logic
class FakeOps:
    """State arithmetic of the solver on the CPU (what ``CNFBase.state_ops_factory`` may supply)."""

    def prepare(self, y):
        return y.detach().to(torch.float32).contiguous()

    def combine(self, y, ks, coefs):
        out = y.clone()
        for k, c in zip(ks, coefs):
            out = out + float(c) * k
        return out


@pytest.fixture
def stubbed(monkeypatch):
    """The tiny modules on the CPU with their single HIP call replaced: ``_run`` records what it receives and returns a prediction
    that differs between rows; ``pair_blend`` and ``mask_from_maps`` are the references of tests/local_edit_cases.py."""
    from uspace_amd import _hip
    from uspace_amd.libs import dissection
    monkeypatch.setattr(_hip, "require_device", lambda *a, **k: None)
    calls = []

    def fake_run(x, timesteps, context=None, key_scale=None, attn_maps=None, mid_row_scale=None, **kw):
        calls.append(dict(rows=x.shape[0], context=context, key_scale=key_scale, attn_maps=attn_maps, mid_row_scale=mid_row_scale, x=x.clone()))
        out = x * 0.5 + torch.arange(x.shape[0], dtype=torch.float32).reshape(-1, 1, 1, 1) + (0.0 if context is None else context.float().mean(dim=(1, 2) if context.dim() == 3 else 1).reshape(-1, 1, 1, 1))
        if attn_maps is None:
            return out
        q0, nq, k0, nk = attn_maps
        g = torch.Generator().manual_seed(len(calls))
        return out, torch.rand(3, x.shape[0], nq, nk, generator=g) ** 8 / 142.0

    def fake_blend(pair, mask, out=None):
        ref = LE.blend_reference(pair.numpy(), mask.numpy())
        pair.copy_(torch.from_numpy(ref.astype(np.float32)))
        blends.append(mask.clone())
        return pair

    def fake_add(x, delta, scale, x_bf16=None, row_scale=None):
        adds.append(None if row_scale is None else row_scale.clone())
        return x

    def fake_maps(maps, block_w, cols, G, patch, thr=0.3, soft=False):
        map_calls.append(dict(block_w=block_w.clone(), cols=cols.clone(), thr=thr))
        m, _ = LE.maps_mask_reference(maps.numpy(), block_w.numpy(), cols.numpy(), G, patch, thr, soft)
        return torch.from_numpy(m.astype(np.float32))

    blends, adds, map_calls = [], [], []
    monkeypatch.setattr(_hip, "pair_blend", fake_blend)
    monkeypatch.setattr(_hip, "add_broadcast", fake_add)
    monkeypatch.setattr(_hip, "mask_from_maps", fake_maps)
    monkeypatch.setattr(dissection.DeltaCache, "get", lambda self, path, ith, device, n: torch.zeros(n))
    nets = {}
    for name in LE.NETS:
        net = LE.make(name)
        monkeypatch.setattr(net, "_run", fake_run)
        nets[name] = net
    return nets, calls, blends, adds, map_calls


def _cnf(net, t2i):
    from uspace_amd import flow_matching, flow_matching_t2i
    cnf = (flow_matching_t2i if t2i else flow_matching).CNF(net)
    cnf.state_ops_factory = lambda y0: FakeOps()
    return cnf


def test_write_scale_rows_are_zeros_then_the_scales(stubbed, tmp_path):
    nets, calls, blends, adds, _ = stubbed
    cnf = _cnf(nets["tiny_u"], False)
    B = 3
    z = torch.randn(B, 4, 16, 16)
    m = LE.checkerboard(B)
    for scale, want in ((2.0, [0, 0, 0, 2, 2, 2]), ([1.0, -1.0, 0.5], [0, 0, 0, 1, -1, 0.5]), (torch.tensor([1.0, 2.0, 3.0]), [0, 0, 0, 1, 2, 3])):
        del calls[:], blends[:], adds[:]
        edited, source = cnf.decode_local(z, None, mask=m, solver_kwargs=LE.SOLVER, **LE.write_kwargs(str(tmp_path), "tail", scale))
        assert edited.shape == z.shape and source.shape == z.shape and cnf.last_stats.nfe == 4
        assert len(calls) == 4 and all(c["rows"] == 2 * B for c in calls) and len(blends) == 4
        assert torch.equal(calls[0]["x"][:B], z) and torch.equal(calls[0]["x"][B:], z)               # both branches start from z
        assert len(adds) == 3 and all(a.tolist() == want for a in adds)                               # no edit at "0.00"
        assert all(torch.equal(b, torch.from_numpy(m).reshape(B, -1)) for b in blends)
    out = torch.from_numpy(np.broadcast_to(m[:, None] == 0, z.shape).copy())
    assert torch.equal(edited[out], source[out])
    # a mid write: the rows go to the forward as mid_row_scale
    del calls[:]
    cnf.decode_local(z, None, mask=m[0], solver_kwargs=LE.SOLVER, **LE.write_kwargs(str(tmp_path), "mid", [1.0, 2.0, 3.0]))
    assert [None if c["mid_row_scale"] is None else c["mid_row_scale"].tolist() for c in calls] == [None] + [[0, 0, 0, 1, 2, 3]] * 3
    with pytest.raises(ValueError, match="write_scale"):
        cnf.decode_local(z, None, mask=m, solver_kwargs=LE.SOLVER, **LE.write_kwargs(str(tmp_path), "tail", [1.0, 2.0]))


def _p2p(B):
    ids = [np.array([3, 5]), np.array([], dtype=np.int64), np.array([0, 76])][:B]
    return dict(dissect_name="p2p", t_edit=0.5, block_id="all", token_kwargs=dict(token_dissect="p2p_rescale", p2p_multiplier=8.0),
                target_context_ids=ids)


def test_p2p_ids_and_contexts_are_paired(stubbed):
    from uspace_amd.tools import utils_t2i
    nets, calls, blends, _, _ = stubbed
    net = nets["tiny_t2i"]
    cnf = _cnf(net, True)
    B = 3
    z, ctx, ctx_src = torch.randn(B, 4, 16, 16), torch.randn(B, 77, 64), torch.randn(B, 77, 64)
    kw = _p2p(B)
    edited, source = cnf.decode_local(z, context=ctx, mask=LE.half_plane(B), solver_kwargs=LE.SOLVER, **kw)
    assert len(calls) == 4 and all(c["rows"] == 2 * B and c["attn_maps"] is None for c in calls)
    assert all(torch.equal(c["context"], torch.cat([ctx, ctx])) for c in calls)
    want = utils_t2i.key_scale_table(net.depth + 1, 2 * B, net.seq_len, "0.25",
                                     dict(kw, fm_direction="decode", target_context_ids=[np.array([], dtype=np.int64)] * B + kw["target_context_ids"]))
    assert np.all(want[:, :B] == 1) and np.any(want[:, B:] != 1)
    for c, edits in zip(calls, (True, True, True, False)):                                            # t = 0, 0.25, 0.5 <= t_edit < 0.75
        assert (c["key_scale"] is not None) == edits
        if edits:
            np.testing.assert_array_equal(c["key_scale"].numpy(), want)
    assert len(kw["target_context_ids"]) == B                                                         # the caller's list is left alone
    # a replaced prompt: the source rows take the source context
    del calls[:]
    lp = dict(dissect_name="local_prompt", t_edit=0.5, token_kwargs=dict(token_dissect="lp_replace"))
    cnf.decode_local(z, context=ctx, mask=LE.half_plane(B), source=dict(context=ctx_src), solver_kwargs=LE.SOLVER, **lp)
    assert all(torch.equal(c["context"], torch.cat([ctx_src, ctx])) and c["key_scale"] is None for c in calls)
    with pytest.raises(ValueError, match="target_context_ids"):
        cnf.decode_local(z, context=ctx, mask=LE.half_plane(B), solver_kwargs=LE.SOLVER, **dict(kw, target_context_ids=kw["target_context_ids"][:2]))
    with pytest.raises(ValueError, match="context"):
        cnf.decode_local(z, context=ctx, mask=LE.half_plane(B), source=dict(context=ctx_src[:2]), solver_kwargs=LE.SOLVER)


def test_class_labels_are_repeated(stubbed):
    nets, calls, _, _, _ = stubbed
    from uspace_amd.tools.utils_uvit import get_nnet
    torch.manual_seed(0)
    net = get_nnet("uvit", **dict(LE.NETS["tiny_u"][0], num_classes=5))
    seen = []
    net._run = lambda x, t, context=None, **kw: (seen.append(context.clone()), x * 0.5)[1]
    cnf = _cnf(net, False)
    z, y = torch.randn(2, 4, 16, 16), torch.tensor([1, 3])
    cnf.decode_local(z, y, mask=LE.half_plane(2), solver_kwargs=LE.SOLVER, dissect_name="none", edit_loc=None)
    w = net.label_emb.weight.detach()
    assert torch.equal(seen[0], w[torch.tensor([1, 3, 1, 3])])
    del seen[:]
    cnf.decode_local(z, y, mask=LE.half_plane(2), source=dict(y=torch.tensor([0, 2])), solver_kwargs=LE.SOLVER, dissect_name="none", edit_loc=None)
    assert torch.equal(seen[0], w[torch.tensor([0, 2, 1, 3])])


def test_attention_word_mask_is_made_at_every_evaluation(stubbed):
    from uspace_amd.tools.local_edit import AttentionWordMask
    nets, calls, blends, _, map_calls = stubbed
    net = nets["tiny_t2i"]
    cnf = _cnf(net, True)
    B = 2
    z, ctx, ctx_src = torch.randn(B, 4, 16, 16), torch.randn(B, 77, 64), torch.randn(B, 77, 64)
    record = []
    wm = AttentionWordMask(token_ids=([np.array([2]), np.array([4, 5])], np.array([3])), blocks=[0, 2], threshold=0.4, from_t=0.3, record=record)
    edited, source = cnf.decode_local(z, context=ctx, mask=wm, source=dict(context=ctx_src), solver_kwargs=LE.SOLVER, dissect_name="none")
    # t = 0 and 0.25 lie below from_t: plain evaluations, no blend; 0.5 and 0.75 ask for the image x context window
    assert [c["attn_maps"] for c in calls] == [None, None, (78, 64, 1, 77), (78, 64, 1, 77)] and all(c["rows"] == 2 * B for c in calls)
    assert len(blends) == 2 and len(map_calls) == 2 and [t for t, _ in record] == [0.5, 0.75]
    cols = map_calls[0]["cols"].numpy()
    assert cols.shape == (2 * B, 77) and cols.sum() == 5
    assert cols[0, 2] == 1 and cols[1, 4] == 1 and cols[1, 5] == 1 and cols[2, 3] == 1 and cols[3, 3] == 1      # source rows first
    assert map_calls[0]["block_w"].tolist() == [1, 0, 1] and abs(map_calls[0]["thr"] - 0.4) < 1e-7
    for (t, m), b in zip(record, blends):
        assert m.shape == (B, 16, 16) and torch.equal(m.reshape(B, -1), b) and set(m.unique().tolist()) <= {0.0, 1.0}
    assert not torch.equal(record[0][1], record[1][1])                       # stateless: every evaluation's own maps
    # words through an embedder's get_word_inds, per caption and per branch

    class Emb:
        def get_word_inds(self, text, word_place):
            return np.array([i + 1 for i, w in enumerate(text.split(" ")) if w == word_place])

    wm = AttentionWordMask(words=("cat", "dog")).for_captions(Emb(), ["a cat", "the big cat"], ["a dog", "no animal"])
    assert [a.tolist() for a in wm.src_ids] == [[2], [3]] and [a.tolist() for a in wm.edit_ids] == [[2], []]
    wm.check(net, 2)
    with pytest.raises(ValueError):
        wm.check(net, 3)


def test_value_errors(stubbed, tmp_path):
    from uspace_amd.tools.local_edit import AttentionWordMask, LabelRegionMask
    from uspace_amd.tools.seg_metrics import LogitsParser
    nets, calls, _, _, _ = stubbed
    B = 2
    z, ctx = torch.randn(B, 4, 16, 16), torch.randn(B, 77, 64)
    u, t = _cnf(nets["tiny_u"], False), _cnf(nets["tiny_t2i"], True)
    ok = LE.half_plane(B)
    base = dict(solver_kwargs=LE.SOLVER)
    for cnf, cond in ((u, dict(y=None)), (t, dict(context=ctx))):
        with pytest.raises(ValueError, match="cfg_scale"):
            cnf.decode_local(z, mask=ok, cfg_scale=0.4, **cond, **base)
        with pytest.raises(ValueError, match="read"):
            cnf.decode_local(z, mask=ok, edit_loc="tail", dissect_task="uspace_uvit", dissect_name="read", read_path_root=str(tmp_path), batch_id=0,
                             **cond, **base)
        with pytest.raises(ValueError, match="vis_am_path"):
            cnf.decode_local(z, mask=ok, vis_am_path=str(tmp_path / "am"), **cond, **base)
        for bad in (np.zeros((B, 8, 8), np.float32), np.zeros((3, 16, 16), np.float32), np.zeros((B, 2, 16, 16), np.float32), np.zeros(256, np.float32),
                    torch.zeros(16, 8)):
            with pytest.raises(ValueError, match="mask must be"):
                cnf.decode_local(z, mask=bad, **cond, **base)
        for val in (np.nan, -0.1, 1.5):
            bad = ok.copy()
            bad[1, 3, 3] = val
            with pytest.raises(ValueError, match=r"\[0, 1\]"):
                cnf.decode_local(z, mask=bad, **cond, **base)
        with pytest.raises(ValueError, match="mask="):
            cnf.decode_local(z, **cond, **base)
        for good in (ok[0], ok, ok[:, None], torch.from_numpy(ok)):
            cnf.decode_local(z, mask=good, dissect_name="none", edit_loc=None, **cond, **base)
    assert os.listdir(tmp_path) == []
    n = len(calls)
    with pytest.raises(ValueError, match="text-to-image"):
        u.decode_local(z, None, mask=AttentionWordMask(token_ids=(np.array([1]), np.array([1]))), **base)
    unbound = LabelRegionMask(LogitsParser(lambda x: x, 19), [1, 4])
    with pytest.raises(ValueError, match="not bound"):
        u.decode_local(z, None, mask=unbound, **base)
    assert len(calls) == n
    with pytest.raises(ValueError):
        LabelRegionMask(LogitsParser(lambda x: x, 19), [19])
    with pytest.raises(ValueError):
        LabelRegionMask(LogitsParser(lambda x: x, 19), [1], dilate=5)
    with pytest.raises(ValueError):
        AttentionWordMask()
    with pytest.raises(ValueError):
        AttentionWordMask(words="cat", token_ids=(np.array([1]), np.array([1])))
    with pytest.raises(ValueError, match="outside"):
        t.decode_local(z, context=ctx, mask=AttentionWordMask(token_ids=(np.array([77]), np.array([1]))), **base)
    # maps beyond 336 tokens stay out of reach
    from uspace_amd.tools.utils_uvit import get_nnet
    long_net = get_nnet("uvit_t2i", **dict(LE.NETS["tiny_t2i"][0], img_size=40))
    with pytest.raises(ValueError, match="336"):
        _cnf(long_net, True).decode_local(torch.randn(1, 4, 40, 40), context=ctx[:1], mask=AttentionWordMask(token_ids=(np.array([1]), np.array([1]))), **base)
    # the network's own refusals of the opt-in keyword
    with pytest.raises(ValueError, match="maps_window"):
        nets["tiny_t2i"](z, torch.full((B,), 0.3), ctx, maps_window=(78, 64, 1, 77), cfg_scale=0.4, empty_context=torch.zeros(77, 64))


def test_forward_without_the_keyword_is_unchanged(stubbed):
    nets, calls, _, _, _ = stubbed
    net = nets["tiny_t2i"]
    z, ctx = torch.randn(2, 4, 16, 16), torch.randn(2, 77, 64)
    out, aux = net(z, torch.full((2,), 0.3), ctx)
    assert aux is None and calls[-1]["attn_maps"] is None
    pred, maps = net(z, torch.full((2,), 0.3), ctx, maps_window=(78, 64, 1, 77))
    assert calls[-1]["attn_maps"] == (78, 64, 1, 77) and maps.shape == (3, 2, 64, 77) and torch.equal(pred, out)
