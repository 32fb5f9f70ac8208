"""CPU-only checks: host-side control logic, the library/ABI surface, seeded init, solver logic."""
import ctypes
import json
import os
import shutil
import sys
import re

import numpy as np
import pytest
import torch

from oracle import odeint_oracle as OO
from oracle import uvit_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------- ABI
def test_library_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "uspace_hip.h")).read()
    declared = set(re.findall(r"USPACE_API\s+[\w\s\*]+?\b(uspace_\w+)\s*\(", hdr))
    assert len(declared) >= 16
    path = os.path.join(ROOT, "uspace_amd", "libuspace_hip.so")
    assert os.path.exists(path), "run __graft_entry__.build() first"
    lib = ctypes.CDLL(path)
    for name in declared:
        assert hasattr(lib, name), name
    from uspace_amd import _hip
    assert set(_hip.SIGNATURES) == declared
    assert _hip.lib().uspace_abi_version() == _hip.ABI_VERSION == 11


def test_struct_layouts_agree_between_header_binding_and_integration_doc():
    """Every struct of include/uspace_hip.h, field by field (name, C type, order): the ctypes classes of
    uspace_amd/_hip.py, the stub tools/abi_stub.py generates, and the copy of that stub in INTEGRATION.md.
    (Round 1 shipped an INTEGRATION.md stub with 9 of uspace_uvit_io's 10 fields.)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("abi_stub", os.path.join(ROOT, "tools", "abi_stub.py"))
    abi = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(abi)
    from uspace_amd import _hip
    header = dict(abi.parse_structs())
    binding = {"uspace_uvit_config": _hip.UvitConfig, "uspace_uvit_io": _hip.UvitIO, "uspace_vae_config": _hip.VaeConfig,
               "uspace_clip_config": _hip.ClipConfig, "uspace_gemm_ext": _hip.GemmExt}
    assert set(header) == set(binding), "a struct of the header has no ctypes class in _hip.py (or the reverse)"
    assert len(header["uspace_uvit_io"]) == 10 and header["uspace_uvit_io"][-1][0] == "mid_row_scale"
    # the generated stub, executed
    ns = {}
    exec(abi.stub(), ns)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    a, b = doc.index(abi.BEGIN), doc.index(abi.END)
    block = doc[a + len(abi.BEGIN):b]
    code = block.split("```python", 1)[1].rsplit("```", 1)[0]
    ns_doc = {}
    exec(code, ns_doc)
    for name, fields in header.items():
        want = [(f, eval(expr, {"ctypes": ctypes})) for f, expr in fields]
        for label, cls in (("_hip.py", binding[name]), ("abi_stub.py", ns[name]), ("INTEGRATION.md", ns_doc[name])):
            got = list(cls._fields_)
            assert [g[0] for g in got] == [w[0] for w in want], f"{label}: field names of {name}"
            for (fn, gt), (_fn, wt) in zip(got, want):
                assert ctypes.sizeof(gt) == ctypes.sizeof(wt) and gt._type_ == wt._type_, f"{label}: {name}.{fn}"
            assert ctypes.sizeof(cls) == ctypes.sizeof(ns[name]), f"{label}: sizeof({name})"
    # the worked example in INTEGRATION.md uses the generated classes, not a hand-written copy
    assert "class IO(" not in doc and "class Cfg(" not in doc


def test_config_queries_without_gpu():
    from uspace_amd import _hip
    L = _hip.lib()
    cfg = _hip.UvitConfig(32, 2, 4, 1024, 20, 16, 4096, 0, 0, 0)
    n = L.uspace_uvit_num_params(ctypes.byref(cfg))
    assert n == 3 + 21 * 11 + 10 * 2 + 6
    total = sum(L.uspace_uvit_param_numel(ctypes.byref(cfg), i) for i in range(n))
    assert total == 285737124                          # L-uncond parameter count
    cfg_t = _hip.UvitConfig(32, 2, 4, 1024, 20, 16, 4096, 77, 768, 1)
    n_t = L.uspace_uvit_num_params(ctypes.byref(cfg_t))
    assert sum(L.uspace_uvit_param_numel(ctypes.byref(cfg_t), i) for i in range(n_t)) == 286603428
    assert L.uspace_uvit_weight_bytes(ctypes.byref(cfg)) > 285737124 * 2
    assert L.uspace_uvit_workspace_bytes(ctypes.byref(cfg), 64) > 64 * 257 * 1024 * 4
    bad = _hip.UvitConfig(32, 2, 4, 1000, 20, 16, 4096, 0, 0, 0)      # D not a multiple of 64
    assert L.uspace_uvit_num_params(ctypes.byref(bad)) < 0
    assert L.uspace_uvit_weight_bytes(ctypes.byref(bad)) == 0


def test_config_rejects_widths_the_output_head_cannot_run():
    """The head keeps its weight image in LDS up to embed_dim 2048: a wider model is refused by the size queries, before anything is
    packed or enqueued, and by the module."""
    from uspace_amd import _hip
    from uspace_amd.tools.utils_uvit import get_nnet
    L = _hip.lib()
    for D, ok in ((2048, True), (2112, False)):
        cfg = _hip.UvitConfig(32, 2, 4, D, 2, D // 64, 4 * D, 0, 0, 0)
        assert (L.uspace_uvit_num_params(ctypes.byref(cfg)) > 0) == ok
        assert (L.uspace_uvit_workspace_bytes(ctypes.byref(cfg), 4) > 0) == ok
        assert (L.uspace_uvit_weight_bytes(ctypes.byref(cfg)) > 0) == ok
    with pytest.raises(NotImplementedError):
        get_nnet("uvit", img_size=32, patch_size=2, in_chans=4, embed_dim=2112, depth=2, num_heads=33, mlp_ratio=4, qkv_bias=False,
                 mlp_time_embed=False, num_classes=-1)


def test_product_never_imports_oracle():
    for dirpath, _dirs, files in os.walk(os.path.join(ROOT, "uspace_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in src.replace("DESIGN.md §oracle", ""), f"{f} mentions the oracle"


def test_forward_on_cpu_fails_loudly():
    from uspace_amd import _hip
    from uspace_amd.tools.utils_uvit import get_nnet
    net = get_nnet("uvit", img_size=16, patch_size=2, in_chans=4, embed_dim=64, depth=2, num_heads=1)
    with pytest.raises(_hip.UspaceHipError):
        net(torch.zeros(1, 4, 16, 16), torch.zeros(1), None, edit_loc=None)


# ------------------------------------------------------------------------------------------- module surface
TINY = dict(img_size=16, patch_size=2, in_chans=4, embed_dim=64, depth=2, num_heads=1, mlp_ratio=4,
            qkv_bias=False, mlp_time_embed=False)


@pytest.mark.parametrize("name,seed,fname,extra", [
    ("uvit", 1234, "tiny_u.npz", dict(num_classes=-1)),
    ("uvit", 1235, "tiny_u_cond.npz", dict(num_classes=10)),
    ("uvit_t2i", 1236, "tiny_t2i.npz", dict(clip_dim=64, num_clip_token=77)),
])
def test_state_dict_keys_order_and_seeded_init_equal_reference(golden_dir, name, seed, fname, extra):
    from uspace_amd.tools.utils_uvit import get_nnet
    z = np.load(os.path.join(golden_dir, fname))
    torch.manual_seed(seed)
    net = get_nnet(name, **TINY, **extra)
    sd = net.state_dict()
    ref_keys = [k[3:] for k in z.files if k.startswith("sd/")]
    assert list(sd.keys()) == ref_keys
    for k in ref_keys:
        assert tuple(sd[k].shape) == z["sd/" + k].shape
        np.testing.assert_array_equal(sd[k].numpy(), z["sd/" + k], err_msg=k)
    assert net.no_weight_decay() == {"pos_embed"}
    net.load_state_dict({k: torch.from_numpy(z["sd/" + k]) for k in ref_keys}, strict=True)


def test_seeded_init_sha_matches_reference_S(golden_dir):
    import hashlib
    from uspace_amd.tools.utils_uvit import get_nnet
    for kind, name, extra in (("u", "uvit", dict(num_classes=-1)), ("t", "uvit_t2i", dict(clip_dim=768, num_clip_token=77))):
        z = np.load(os.path.join(golden_dir, f"big_S_{kind}.npz"))
        meta = json.loads(bytes(z["meta_json"]).decode())
        torch.manual_seed(meta["weight_seed"])
        net = get_nnet(name, img_size=32, patch_size=2, in_chans=4, embed_dim=512, depth=16, num_heads=8,
                       mlp_ratio=4, qkv_bias=False, mlp_time_embed=False, use_checkpoint=True, **extra)
        h = hashlib.sha256()
        for k, v in net.state_dict().items():
            h.update(k.encode())
            h.update(np.ascontiguousarray(v.numpy()).tobytes())
        assert h.hexdigest() == meta["sha256"]


def test_factory_and_unsupported_configs():
    from uspace_amd.tools.utils_uvit import amortize, get_nnet
    with pytest.raises(NotImplementedError):
        get_nnet("resnet")
    with pytest.raises(NotImplementedError):
        get_nnet("unet_t2i")
    with pytest.raises(NotImplementedError):
        get_nnet("uvit", **dict(TINY, qkv_bias=True))
    with pytest.raises(NotImplementedError):
        get_nnet("uvit", **dict(TINY, embed_dim=96, num_heads=2))     # head_dim 48
    assert amortize(10, 4) == [4, 4, 2] and amortize(8, 4) == [4, 4] and amortize(3, 4) == [3]


# ------------------------------------------------------------------------------------------- hook control plane
def test_should_edit_and_plan_follow_oracle():
    from uspace_amd.libs import dissection as D
    for digit in ("0.00", "0.01", "0.20", "0.40", "0.41", "1.00"):
        for t_edit in (0.4, 0, 1, "every_0.2", "every_0.1"):
            assert D.should_edit(digit, t_edit) == O.should_edit(digit, t_edit), (digit, t_edit)
    for bad in ("sometimes", None, [0.4]):
        with pytest.raises(ValueError):
            D.should_edit("0.10", bad)
    tab = np.arange(5 * 6, dtype=np.float32).reshape(5, 6)
    np.testing.assert_array_equal(D.select_rows(tab, 2), O.select_delta(tab, 2)[0])
    np.testing.assert_array_equal(D.select_rows(tab, "0_2_4"), O.select_delta(tab, "0_2_4")[0])
    base = dict(dissect_task="uspace_uvit", t_edit=0.4, write_path_root="/w", write_scale=2.0)
    p = D.plan_uspace_hook("0.20", dict(base, dissect_name="write_attr", ith_attr="31_39_20"))
    assert (p.kind, p.path, p.ith, p.scale) == ("write", "/w/delta_0.20.npy", "31_39_20", 2.0)
    p = D.plan_uspace_hook("0.20", dict(base, dissect_name="write_pca", ith_component=3, pca_n=100))
    assert (p.path, p.ith) == ("/w/pca100_0.20.npy", 3)
    assert D.plan_uspace_hook("0.41", dict(base, dissect_name="write_attr", ith_attr=1)) is None
    assert D.plan_uspace_hook("0.00", dict(base, dissect_name="write_attr", ith_attr=1)) is None
    assert D.plan_uspace_hook("0.20", dict(base, dissect_task="other", dissect_name="bogus")) is None
    p = D.plan_uspace_hook("0.37", dict(dissect_task="uspace_uvit", dissect_name="read", read_path_root="/r", batch_id=5))
    assert (p.kind, p.path) == ("read", "/r/5_0.37")
    with pytest.raises(ValueError):
        D.plan_uspace_hook("0.20", dict(base, dissect_name="bogus"))


def test_timestep_digit_rounding_cases():
    from uspace_amd.libs._uvit_core import timestep_digit
    assert timestep_digit(0.004) == "0.00" and timestep_digit(0.404) == "0.40" and timestep_digit(0.405) == "0.41"
    assert timestep_digit(np.float32(0.2)) == "0.20" and timestep_digit(1.0) == "1.00"


def test_key_scale_table_equals_oracle_on_golden_cases(golden_dir):
    from uspace_amd.tools import utils_t2i as T
    z = np.load(os.path.join(golden_dir, "p2p_t2i.npz"))
    cases = json.loads(bytes(z["cases_json"]).decode())
    ids = [z["ids_a0"], z["ids_a1"], z["ids_a2"]]
    nb, B, L = 3, 3, 142
    for c in cases:
        kw = dict(c)
        tv = kw.pop("tval")
        kw.pop("ids")
        kw["target_context_ids"] = ids
        digit = f"{float(np.float32(tv)):.2f}"
        got = T.key_scale_table(nb, B, L, digit, kw)
        want = [O.p2p_column_scale(B, L, tv, kw, blk) for blk in range(nb)]
        if got is None:
            assert all(w is None or np.all(w == 1.0) for w in want), c
        else:
            for blk in range(nb):
                w = want[blk] if want[blk] is not None else np.ones((B, L), np.float32)
                np.testing.assert_array_equal(got[blk], w)
    with pytest.raises(ValueError):
        T.key_scale_table(nb, B, L, "0.30", dict(dissect_name="read"))
    with pytest.raises(NotImplementedError):
        T.key_scale_table(nb, B, L, "0.30", dict(dissect_name="p2p", fm_direction="decode", t_edit=0.5,
                                                 token_kwargs=dict(token_dissect="p2p_replace", p2p_multiplier=1)))
    with pytest.raises(ValueError):
        T.block_selected("some", 1)


# ------------------------------------------------------------------------------------------- solver logic on CPU
class NumpyOps:
    """Test-local state arithmetic so the product's odeint control flow can run without a GPU."""

    def __init__(self, like=None):
        pass

    def prepare(self, y):
        return np.asarray(y, np.float32)

    def combine(self, y, ks, coefs):
        out = np.asarray(y, np.float32).copy()
        for k, c in zip(ks, coefs):
            out += np.float32(c) * k
        return out

    def scaled_norm(self, y0, y1, ks, coefs, rtol, atol):
        err = np.zeros_like(y0)
        for k, c in zip(ks, coefs):
            err += np.float32(c) * k
        tol = np.float32(atol) + np.float32(rtol) * np.maximum(np.abs(y0), np.abs(y1))
        return float(np.sqrt(np.mean(np.square(err / tol), dtype=np.float32)))


def _field(t, y):
    return (-0.8 * y + np.float32(np.sin(3.0 * t)) + 0.3 * np.tanh(y)).astype(np.float32)


@pytest.mark.parametrize("method,kw", [
    ("euler", dict(step_size=0.01)), ("midpoint", dict(step_size=0.02)), ("rk4", dict(step_size=0.05)),
    ("dopri5", dict(n_steps=50)), ("dopri5", {}), ("bosh3", {}), ("adaptive_heun", dict(rtol=1e-3, atol=1e-3)),
])
@pytest.mark.parametrize("span", [(0.0, 1.0), (1.0, 0.0), (0.3, 0.9)])
def test_product_odeint_control_flow_matches_oracle(method, kw, span):
    from uspace_amd.odeint import Stats, odeint
    y0 = np.random.default_rng(2).standard_normal((2, 4, 4, 4)).astype(np.float32)
    cnt = {}
    ref = OO.solve(_field, y0, *span, method=method, counters=cnt, **kw)
    st = Stats()
    got = odeint(_field, y0, *span, method=method, ops=NumpyOps(), stats=st, **kw)
    np.testing.assert_allclose(got, ref, rtol=2e-5, atol=2e-6)
    assert st.nfe == cnt["nfe"]


def test_solvers_converge_at_their_order_and_agree():
    exact = lambda y0: None
    f = lambda t, y: (-2.0 * y).astype(np.float32)
    y0 = np.ones((8,), np.float32)
    want = np.exp(-2.0)
    errs = {}
    for m, p in (("euler", 1), ("midpoint", 2), ("rk4", 4)):
        e = [abs(float(OO.solve(f, y0, 0.0, 1.0, method=m, n_steps=n)[0]) - want) for n in (8, 16)]
        errs[m] = e
        assert 0.7 * 2 ** p < e[0] / e[1] < 1.4 * 2 ** p, (m, e)
    fine = OO.solve(f, y0, 0.0, 1.0, method="euler", n_steps=1000)
    adp = OO.solve(f, y0, 0.0, 1.0, method="dopri5")
    assert abs(float(adp[0]) - want) < 1e-5 and abs(float(fine[0]) - want) < 1e-3
    assert OO.grid_points(0, 1, 0.01).size == 101 and OO.grid_points(0, 0.4, 0.01).size == 41
    from uspace_amd.odeint import fixed_grid
    np.testing.assert_array_equal(np.array(fixed_grid(0, 1, 0.01)), OO.grid_points(0, 1, 0.01))
    np.testing.assert_array_equal(np.array(fixed_grid(-1, 0, 0.01)), OO.grid_points(-1, 0, 0.01))


class _F64Ops:
    """fp64 state arithmetic (test-local) so the tableau constants are compared beyond fp32 rounding."""

    def prepare(self, y):
        return np.asarray(y, np.float64)

    def combine(self, y, ks, coefs):
        out = np.asarray(y, np.float64).copy()
        for k, c in zip(ks, coefs):
            out += float(c) * k
        return out

    def scaled_norm(self, y0, y1, ks, coefs, rtol, atol):
        err = sum(float(c) * k for k, c in zip(ks, coefs))
        return float(np.sqrt(np.mean((err / (atol + rtol * np.maximum(np.abs(y0), np.abs(y1)))) ** 2)))


def test_dopri5_step_is_pinned_to_scipy_rk45():
    """Independent pin of the integrator arithmetic.  torchdiffeq -- what the reference calls at
    flow_matching.py:118,140,163,172 -- is absent; scipy.integrate's RK45 is an independent statement of the same
    Dormand-Prince pair.  Pinned here: the stage abscissae / stage matrix / 5th-order weights (through one whole step: y1
    and every stage derivative), the dense-output mid-point weights (scipy's interpolant P at theta = 1/2), the dense
    output against scipy's at other theta to the order of the interpolant, and the error weights up to the one documented
    difference: torchdiffeq's estimate is -2/3 of the textbook b5 - b4 difference scipy uses (its embedded 4th-order
    weights are 1951/21600, 22642/50085, ... with -1/60 for the FSAL stage).  NOT pinned by this test: the step-size
    controller, the initial-step heuristic and the accept rule (they stay "parity unpinned")."""
    from scipy.integrate import RK45
    from scipy.integrate._ivp.rk import rk_step
    from uspace_amd import odeint as oi

    tab = oi._DOPRI5
    # constants, entry by entry
    np.testing.assert_allclose([0.0] + tab["alpha"][:-1], RK45.C, rtol=0, atol=1e-15)
    for i, row in enumerate(tab["beta"][:-1]):
        np.testing.assert_allclose(row, RK45.A[i + 1][: len(row)], rtol=0, atol=1e-15)
    np.testing.assert_allclose(tab["beta"][-1], RK45.B, rtol=0, atol=1e-15)          # FSAL row = 5th-order weights
    np.testing.assert_allclose(tab["c_sol"][:-1], RK45.B, rtol=0, atol=1e-15)
    np.testing.assert_allclose(tab["c_err"], -2.0 / 3.0 * RK45.E, rtol=0, atol=1e-15)
    np.testing.assert_allclose(tab["c_mid"], RK45.P @ (0.5 ** np.arange(1, 5)), rtol=0, atol=1e-15)

    # one whole step on a closed-form, non-autonomous, nonlinear field: product code against scipy's rk_step
    def f(t, y):
        return -1.3 * y + np.sin(3.0 * t) + 0.4 * np.tanh(y) * np.cos(t)

    y0 = np.random.default_rng(5).standard_normal(24)
    t0, h = 0.37, 0.11
    f0 = f(t0, y0)
    st = oi.Stats()
    y1, f1, ks, ratio = oi._adaptive_try(f, tab, _F64Ops(), t0, h, y0, f0, 1.0, st, 1e-5, 1e-5)
    K = np.empty((7, y0.size))
    y1_ref, f1_ref = rk_step(f, t0, y0, f0, h, RK45.A, RK45.B, RK45.C, K)
    assert st.nfe == 6
    np.testing.assert_allclose(y1, y1_ref, rtol=1e-13, atol=1e-14)
    np.testing.assert_allclose(f1, f1_ref, rtol=1e-13, atol=1e-14)
    np.testing.assert_allclose(np.stack(ks), K, rtol=1e-12, atol=1e-13)
    err_ref = -2.0 / 3.0 * (K.T @ RK45.E) * h
    err = sum(h * c * k for c, k in zip(tab["c_err"], ks))
    np.testing.assert_allclose(err, err_ref, rtol=1e-10, atol=1e-16)
    want_ratio = np.sqrt(np.mean((err_ref / (1e-5 + 1e-5 * np.maximum(np.abs(y0), np.abs(y1_ref)))) ** 2))
    assert abs(ratio - want_ratio) <= 1e-9 * want_ratio

    # dense output: the product's quartic through (y0, y_mid, y1, f0, f1) against scipy's interpolant y0 + h K^T P theta^i
    for theta in (0.5, 0.25, 0.8, 1.0):
        got = oi._dense_eval(tab, _F64Ops(), t0, h, y0, y1, f0, f1, ks, t0 + theta * h)
        ref = y0 + h * (K.T @ (RK45.P @ (theta ** np.arange(1, 5))))
        # both are 4th-order interpolants that agree at theta = 0, 1/2, 1 in value and at 0, 1 in slope: equal as polynomials
        np.testing.assert_allclose(got, ref, rtol=1e-11, atol=1e-12)


class _StubNet(torch.nn.Module):
    """CPU stand-in for nnet used only to exercise CNF's solver-selection logic."""

    def __init__(self):
        super().__init__()
        self.calls = []

    def forward(self, x, t, *args, **kwargs):
        self.calls.append((float(t.reshape(-1)[0]), t.stride(), args, dict(kwargs)))
        return -x, None


class TorchCpuOps(NumpyOps):
    def prepare(self, y):
        return y.detach().float()

    def combine(self, y, ks, coefs):
        out = y.clone()
        for k, c in zip(ks, coefs):
            out += float(c) * k
        return out

    def scaled_norm(self, y0, y1, ks, coefs, rtol, atol):
        err = sum(float(c) * k for k, c in zip(ks, coefs))
        tol = atol + rtol * torch.maximum(y0.abs(), y1.abs())
        return float(torch.sqrt(torch.mean((err / tol) ** 2)))


def test_cnf_solver_selection_mirrors_reference():
    from uspace_amd.flow_matching import CNF
    from uspace_amd.flow_matching_t2i import CNF as CNFT
    sk = dict(solver="fixadp", solver_fix="euler", solver_fix_step=0.01, solver_adaptive="dopri5", solver_adaptive_prec=0.01)
    net = _StubNet()
    cnf = CNF(net)
    cnf.state_ops_factory = TorchCpuOps
    assert cnf.net is net
    # non-dissection -> dopri5 1e-5 regardless of solver_kwargs (flow_matching.py:77-84)
    kw = cnf.get_ode_kwargs(solver_kwargs=sk, dissect_name=None)
    assert kw == dict(method="dopri5", rtol=1e-5, atol=1e-5, adjoint_params=())
    fx, ad = cnf.get_ode_kwargs(solver_kwargs=sk, dissect_name="write_attr")
    assert fx["method"] == "euler" and fx["options"] == dict(step_size=0.01) and ad["method"] == "dopri5"
    assert cnf.get_ode_kwargs(solver_kwargs=dict(sk, solver="fixed"), dissect_name="x")["options"]["step_size"] == 0.01
    with pytest.raises(NotImplementedError):
        cnf.get_ode_kwargs(solver_kwargs=dict(sk, solver="zzz"), dissect_name="x")
    assert cnf.is_dissection_mode(dict(dissect_name="read")) and not cnf.is_dissection_mode(dict(dissect_name=None))
    with pytest.raises(KeyError):
        cnf.decode(torch.zeros(2, 4, 4, 4), None)
    with pytest.raises(NotImplementedError):
        cnf.training_losses(None, None, 1e-4)

    z = torch.ones(3, 4, 4, 4)
    out = cnf.decode(z, "LABEL", dissect_name="write_attr", edit_loc=None, t_edit=0.4, solver_kwargs=sk)
    ts = [c[0] for c in net.calls]
    assert ts[:41] == pytest.approx([k * 0.01 for k in range(41)][:41], abs=1e-6) or len(ts) > 41
    assert abs(ts[39] - 0.39) < 1e-6 and abs(ts[40] - 0.4) < 1e-6          # 40 Euler steps then dopri5 from 0.4
    assert all(c[1] == (0,) for c in net.calls)                            # stride-0 timesteps
    assert all(c[2] == ("LABEL",) for c in net.calls)                      # y positional (flow_matching.py:34)
    assert all("_t_host" in c[3] and c[3]["edit_loc"] is None for c in net.calls)
    torch.testing.assert_close(out, z * float(np.exp(-1.0)), rtol=2e-2, atol=1e-3)

    net.calls.clear()
    cnf.encode(z, None, dissect_name=None, solver_kwargs=dict(sk, solver_fix_step=0.25))   # encode: always fixed
    assert [round(c[0], 6) for c in net.calls] == [1.0, 0.75, 0.5, 0.25]

    net.calls.clear()
    cnft = CNFT(net)
    cnft.state_ops_factory = TorchCpuOps
    kw = dict(dissect_name="p2p", solver_kwargs=dict(sk, solver="fixed", solver_fix_step=0.5))
    cnft.decode(z, "CTX", **kw)
    assert [c[3]["fm_direction"] for c in net.calls] == ["decode", "decode"]
    assert all(c[2] == () and c[3]["context"] == "CTX" for c in net.calls)  # context by keyword
    net.calls.clear()
    cnft.encode(z, "CTX", **kw)
    assert [c[3]["fm_direction"] for c in net.calls] == ["encode", "encode"]
    assert [round(c[0], 6) for c in net.calls] == [1.0, 0.5]
    # n_steps extension: "dopri5-50" == 301 evaluations, "euler-50" == 50
    net.calls.clear()
    cnf.decode(z, None, dissect_name="bench", edit_loc=None, solver_kwargs=dict(sk, solver="adaptive", n_steps=50))
    assert len(net.calls) == 301 and cnf.last_stats.nfe == 301
    net.calls.clear()
    cnf.decode(z, None, dissect_name="bench", edit_loc=None, solver_kwargs=dict(sk, solver="fixed", n_steps=50))
    assert len(net.calls) == 50


# ------------------------------------------------------------------------------------------- VAE decoder module
def test_vae_module_surface_and_seeded_init(golden_dir):
    """FrozenAutoencoderKL (libs/autoencoder.py:412-450) decode side: reference key order, seeded init bit-equal to
    the reference's (sha256 from the fixture), full checkpoints load, no CPU decode."""
    import hashlib
    from uspace_amd import _hip
    from uspace_amd.libs.autoencoder import FrozenAutoencoderKL, get_model
    z = np.load(os.path.join(golden_dir, "vae_decoder_tiny.npz"))
    meta = json.loads(bytes(z["meta_json"]).decode())
    torch.manual_seed(meta["weight_seed"])
    vae = FrozenAutoencoderKL(meta["ddconfig"], 4)
    sd = vae.state_dict()
    assert list(sd.keys()) == meta["keys"] and sum(v.numel() for v in sd.values()) == meta["n_params"]
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(np.ascontiguousarray(v.numpy()).tobytes())
    assert h.hexdigest() == meta["sha256"]
    assert not vae.training and not any(p.requires_grad for p in vae.parameters())
    full = dict(sd)
    full["encoder.conv_in.weight"] = torch.zeros(3)
    full["quant_conv.bias"] = torch.zeros(8)
    vae.load_state_dict(full)                                 # encoder half accepted and ignored
    with pytest.raises(RuntimeError):
        vae.load_state_dict({k: v for k, v in sd.items() if k != "decoder.conv_out.bias"})
    with pytest.raises(_hip.UspaceHipError):
        vae.decode(torch.zeros(1, 4, 8, 8))                   # host tensor: no CPU path
    with pytest.raises(NotImplementedError):
        vae(torch.zeros(1, 4, 8, 8), "encode")
    with pytest.raises(NotImplementedError):
        FrozenAutoencoderKL(dict(meta["ddconfig"], attn_resolutions=[8]), 4)
    big = get_model(None)
    assert sum(p.numel() for p in big.parameters()) == 49490199 and big.z_res == 32 and big.scale_factor == 0.18215


def test_vae_config_queries_without_gpu():
    from uspace_amd import _hip
    L = _hip.lib()
    mult = (ctypes.c_int * 4)(1, 2, 4, 4)
    cfg = _hip.VaeConfig(128, mult, 4, 2, 256)
    n = L.uspace_vae_num_params(ctypes.byref(cfg))
    assert n == 140
    assert sum(L.uspace_vae_param_numel(ctypes.byref(cfg), i) for i in range(n)) == 49490199
    assert L.uspace_vae_weight_bytes(ctypes.byref(cfg)) >= 49490199 * 2
    assert L.uspace_vae_workspace_bytes(ctypes.byref(cfg), 8) > 8 * 258 * 258 * 256 * 4
    bad = _hip.VaeConfig(100, mult, 4, 2, 256)                # ch not a multiple of 64
    assert L.uspace_vae_num_params(ctypes.byref(bad)) < 0 and L.uspace_vae_weight_bytes(ctypes.byref(bad)) == 0


# ------------------------------------------------------------------------------------------- CLIP text encoder module
def test_clip_module_surface(golden_dir):
    from uspace_amd import _hip
    from uspace_amd.libs.clip import CLIPTextTransformer, CLIP_L_TEXT, get_word_inds
    z = np.load(os.path.join(golden_dir, "clip_text_tiny.npz"))
    meta = json.loads(bytes(z["meta_json"]).decode())
    m = CLIPTextTransformer(vocab_size=1000, hidden_size=128, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2)
    assert list(m.state_dict().keys()) == meta["keys"]                     # HF CLIPTextModel's own key order
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd/")}
    m.load_state_dict(sd)
    pref = {"text_model." + k: v for k, v in sd.items()}
    pref["text_model.embeddings.position_ids"] = torch.arange(77)[None]    # older checkpoints carry this buffer
    pref["logit_scale"] = torch.zeros(())
    m.load_state_dict(pref)
    with pytest.raises(_hip.UspaceHipError):
        m(torch.zeros(1, 77, dtype=torch.long))                            # host tensor: no CPU path
    with pytest.raises(NotImplementedError):
        CLIPTextTransformer(hidden_act="gelu")
    L = _hip.lib()
    cfg = _hip.ClipConfig(49408, 768, 12, 12, 3072, 77, 1e-5)
    n = L.uspace_clip_num_params(ctypes.byref(cfg))
    assert n == 2 + 16 * 12 + 2
    assert sum(L.uspace_clip_param_numel(ctypes.byref(cfg), i) for i in range(n)) == 123060480   # CLIP-L text model
    assert L.uspace_clip_weight_bytes(ctypes.byref(cfg)) > 49408 * 768 * 4
    assert L.uspace_clip_workspace_bytes(ctypes.byref(cfg), 8) > 8 * 77 * 768 * 4
    bad = _hip.ClipConfig(49408, 768, 8, 12, 3072, 77, 1e-5)              # head_dim != 64
    assert L.uspace_clip_num_params(ctypes.byref(bad)) < 0 and L.uspace_clip_weight_bytes(ctypes.byref(bad)) == 0

    class Tok:                                                              # word pieces: "running" -> "run" "##ning"
        table = {"a": [5], "dog": [6], "running": [7, 8], "fast": [9]}
        names = {5: "a", 6: "dog", 7: "run", 8: "##ning", 9: "fast"}

        def encode(self, text):
            return [0] + [i for w in text.split(" ") for i in self.table[w]] + [1]

        def decode(self, ids):
            return self.names.get(ids[0], "")
    assert get_word_inds("a dog running fast", "running", Tok()).tolist() == [3, 4]
    assert get_word_inds("a dog running fast", 3, Tok()).tolist() == [5]
    assert get_word_inds("a dog running fast", "cat", Tok()).tolist() == []


def test_gemm_tile_planning_on_headline_shapes():
    """uspace_gemm_tile_choice: the U-ViT-L B=64 shapes stay on the measured 256x256 form (3 / 1 / 4 / 1 / 1 rounds);
    narrow outputs and short row counts go to smaller tiles."""
    from uspace_amd import _hip
    L = _hip.lib()

    def choice(M, N):
        s = ctypes.c_int(0)
        return L.uspace_gemm_tile_choice(M, N, ctypes.byref(s)), s.value
    for N in (1024, 3072, 4096):
        assert choice(64 * 257, N)[0] == 0
    assert choice(64 * 334, 512)[0] == 1            # U-ViT-S T2I: 224 tiles of 192x256 = one round instead of 1.3
    assert choice(4 * 257, 1536)[0] == 2 and choice(300, 64)[0] == 2 and choice(16448, 128)[0] == 2
    # 256x128 tiles where 256x256 would leave CUs idle and 128x128 needs two workgroups per CU (config 5 rows, N = 1024)
    assert choice(32 * 257, 1024)[0] == 4 and choice(8 * 257, 4096)[0] == 4 and choice(4 * 257, 4096)[0] == 4
    c, rows = choice(64 * 334, 1024)
    assert c in (1, 3) and (c != 3 or (0 < rows < 64 * 334 and rows % 256 == 0))
    assert L.uspace_gemm_tile_choice(0, 64, None) < 0


def test_hot_kernels_have_no_scratch_and_fit_their_register_budget():
    """Code-object metadata of the built library (tools/kernel_resources.py; no GPU): no GEMM / attention kernel spills to
    scratch, and every kernel that shares a SIMD between two waves (all but the one-workgroup-per-CU ring form of the K-split)
    stays within 256 vector registers."""
    import importlib.util
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"):
        pytest.skip("llvm-objdump not available")
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    ks = kr.kernels()
    names = kr.demangle([k["name"] for k in ks])
    hot = [(k, n) for k, n in zip(ks, names) if "gemm_kernel" in n or "attention_kernel" in n or "gemm_kernel" in k["name"]]
    assert len(hot) > 100
    for k, n in hot:
        assert k["scratch"] == 0, (n, k)
        ring = k["lds"] >= 128 * 1024 and k["wg"] == 256            # 4 waves, 128 KiB of LDS: one wave per SIMD
        assert ring or k["vgpr"] + k["agpr"] <= 256, (n, k)
    assert not [k for k in ks if k["scratch"] > 256], "a kernel with a large scratch frame"


def test_gemm_plans_on_random_shapes():
    """Property test of the host-side planner (uspace_gemm_plan / _part_slots / _split_ws_bytes) over random [M, N, K]: the tile
    rows plus the 16-row strips cover M exactly once, strips never outnumber tile rows, the partial-sum slot count is the number
    of N tiles of the chosen form, and a K-split workspace is S whole [M, N] fp32 images with S in {2, 4, 8}."""
    from hypothesis import given, settings, strategies as st
    from uspace_amd import _hip
    L = _hip.lib()
    out = (ctypes.c_int * 8)()

    @settings(max_examples=400, deadline=None)
    @given(M=st.integers(1, 70000), n4=st.one_of(st.integers(1, 2048), st.sampled_from([64, 128, 256, 512, 768, 1024])), k64=st.integers(1, 128))
    def check(M, n4, k64):
        N, K = 4 * n4, 64 * k64
        assert L.uspace_gemm_plan(M, N, out) == 0
        choice, split, BM, BN, tm, tn, ns, per_round = list(out)
        assert choice in (0, 1, 2, 3, 4) and (BM, BN) in ((256, 256), (192, 256), (128, 128), (256, 128))
        rows = split if choice == 3 else M
        assert (choice == 3) == (0 < split < M and split % 256 == 0) or choice != 3
        assert tn == -(-N // BN) and 0 <= ns <= tm
        if ns:
            assert tm * BM < rows <= tm * BM + 16 * ns and rows > tm * BM + 16 * (ns - 1)
        else:
            assert (tm - 1) * BM < rows <= tm * BM
        # producers of LayerNorm partial sums: 128-wide slots for the 128x128 form, and for the 256x128 form only while that makes at
        # most 8 of them (the consumers read up to 8): wider N falls back to 256-wide tiles
        narrow = choice == 2 or (choice == 4 and -(-N // 128) <= 8)
        # ... and 64-wide slots where the 128x128 tiling would fill 160 workgroups or fewer and that makes at most 8 slots
        tiny = choice == 2 and -(-M // 128) * -(-N // 128) <= 160 and -(-N // 64) <= 8
        out_k = (ctypes.c_int * 8)()
        sk_any = 0
        for prod in (0, 1):
            assert L.uspace_gemm_plan_k(M, N, K, prod, out_k) == 0
            want_tiny = choice == 2 and -(-M // 128) * -(-N // 128) <= 160 and (not prod or -(-N // 64) <= 8)
            assert (out_k[0] == 5) == want_tiny and ((out_k[2], out_k[3]) == (64, 64)) == want_tiny
            if want_tiny:
                assert out_k[5] == -(-N // 64) and out_k[4] * 64 <= M + 63
            if out_k[0] == 6:
                # the in-launch K-split tail (round 6): whole 256-column tiles, a K loop of >= 64 tiles cut into S = 2 ... 4 parts of >= 16,
                # whole rounds of whole-tile workgroups in front, at most 256 workgroups on shared tiles (they wait for each other)
                form, S, bm, bn, tm_k, tn_k, ns_k, n_dp = list(out_k)
                assert (bm, bn) == (256, 256) and N % 256 == 0 and tn_k == N // 256 and K >= 4096 and 2 <= S <= 4 and K // 64 // S >= 16
                n_sk = tm_k * tn_k - n_dp
                assert n_dp % 256 == 0 and 0 < n_sk < 256 and -(-n_sk // 8) * 8 * S <= 256 and (S > 2 or -(-n_sk // 8) * 8 * S >= 224)
                assert 0 <= ns_k <= tm_k and (tm_k * 256 < M <= tm_k * 256 + 16 * ns_k if ns_k else (tm_k - 1) * 256 < M <= tm_k * 256)
                slab = (256 + (16 if ns_k else 0)) * 1024
                sk_any = max(sk_any, -(-n_sk // 8) * 8 * S * slab)
                if prod:
                    assert L.uspace_gemm_part_slots_k(M, N, K) == N // 256
        assert L.uspace_gemm_sk_ws_bytes(M, N, K) == sk_any
        assert L.uspace_gemm_plan_k(M, N, K, 1, out_k) == 0
        for Kq, t in ((K, tiny), (64, tiny)):
            got = L.uspace_gemm_part_slots_k(M, N, Kq)
            if Kq == K and out_k[0] == 6:
                continue
            assert got == (-(-N // 64) if t else -(-N // 128) if narrow else -(-N // 256)), (M, N, Kq)
        assert L.uspace_gemm_part_slots(M, N) == L.uspace_gemm_part_slots_k(M, N, 64)
        ws = L.uspace_gemm_split_ws_bytes(M, N, K)
        if ws:
            S = ws // (M * N * 4)
            assert choice == 2 and ws == S * M * N * 4 and S in (2, 4, 8) and K >= 1024 and (K // 64) % S == 0 and K // S >= 512
            assert -(-M // 128) * -(-N // 128) * S <= 256

    check()


def test_gemm_k_split_tail_plans_and_switch():
    """The in-launch K-split tail (round 6) as the host sees it: which BASELINE launches have one (fc2 of U-ViT-L -- K = 4096 -- at the row
    counts whose 256x256 tiles do not fill whole rounds; never the headline, never K <= 2048, never U-ViT-S), its workspace size, the
    partial-sum slots a producer then writes, and the process-wide switch (every query answers for the current setting)."""
    from uspace_amd import _hip
    L = _hip.lib()
    out = (ctypes.c_int * 8)()

    def plan(M, N, K, prod=1):
        assert L.uspace_gemm_plan_k(M, N, K, prod, out) == 0
        return list(out)
    slab, slab_x = 256 * 1024, 272 * 1024
    try:
        assert L.uspace_gemm_get_sk() == 1
        # config 3 (64 x 334 rows): one whole round + 76 tiles in 3 K parts, 8 strips; config 5 (32 x 257): 128 tiles x 2, 2 strips; 16 per GPU: x 4
        assert plan(64 * 334, 1024, 4096)[:2] == [6, 3] and plan(64 * 334, 1024, 4096)[4:] == [83, 4, 8, 256]
        assert plan(32 * 257, 1024, 4096)[:2] == [6, 2] and plan(32 * 257, 1024, 4096)[4:] == [32, 4, 2, 0]
        assert plan(16 * 257, 1024, 4096)[:2] == [6, 4]
        assert L.uspace_gemm_sk_ws_bytes(64 * 334, 1024, 4096) == 80 * 3 * slab_x
        assert L.uspace_gemm_sk_ws_bytes(32 * 257, 1024, 4096) == 128 * 2 * slab_x
        assert L.uspace_gemm_sk_ws_bytes(30 * 256 + 500, 1024, 4096) == 128 * 2 * slab_x         # 31 tile rows + 16 strips (244 rows left)
        assert plan(10 * 256 + 200, 1024, 4096)[:2] == [6, 4] and plan(10 * 256 + 200, 1024, 4096)[4:] == [11, 4, 0, 0]   # 200 rows left > 10 strips: an 11th tile row
        assert L.uspace_gemm_sk_ws_bytes(10 * 256 + 200, 1024, 4096) == 48 * 4 * slab             # ... no strips: 256 KiB slabs; 44 tiles padded to 6 groups of 8
        assert L.uspace_gemm_part_slots_k(32 * 257, 1024, 4096) == 4                              # 256-wide tiles: one stride for the whole launch
        assert L.uspace_gemm_part_slots_k(32 * 257, 1024, 1024) == 8                              # proj stays on 256x128 tiles
        for M, N, K in ((64 * 257, 1024, 4096), (64 * 257, 4096, 1024), (64 * 257, 3072, 1024),    # the headline: whole rounds, no tail
                        (64 * 334, 1024, 2048), (64 * 334, 1024, 1024), (32 * 257, 3072, 1024),    # K loops below 64 tiles: the exchange costs more than it saves
                        (64 * 334, 512, 2048), (4 * 257, 512, 2048), (24 * 257, 1024, 4096)):      # U-ViT-S; small launches; 96 tiles x 2 would idle a quarter of the CUs
            assert plan(M, N, K)[0] != 6 and L.uspace_gemm_sk_ws_bytes(M, N, K) == 0, (M, N, K)
        # the U-ViT workspace carries the slabs and one set of counters per GEMM launch only where a launch has a tail
        cfg = _hip.UvitConfig(32, 2, 4, 1024, 20, 16, 4096, 0, 0, 0)
        with_sk = {B: L.uspace_uvit_workspace_bytes(ctypes.byref(cfg), B) for B in (64, 32)}
        assert L.uspace_gemm_set_sk(0) == 0 and L.uspace_gemm_get_sk() == 0
        assert plan(32 * 257, 1024, 4096)[0] == 4 and L.uspace_gemm_sk_ws_bytes(32 * 257, 1024, 4096) == 0
        assert L.uspace_gemm_part_slots_k(32 * 257, 1024, 4096) == 8
        without = {B: L.uspace_uvit_workspace_bytes(ctypes.byref(cfg), B) for B in (64, 32)}
        assert with_sk[64] == without[64] and with_sk[32] - without[32] >= 128 * 2 * slab_x
        assert L.uspace_gemm_set_sk(2) < 0
    finally:
        L.uspace_gemm_set_sk(-1)
    assert L.uspace_gemm_get_sk() == 1


def test_gemm_k_split_workspace_sizes():
    """uspace_gemm_split_ws_bytes: only launches of 128x128 tiles that leave most CUs idle and have a long K are split
    (S K ranges, S * M * N fp32 partial sums): the fc2 / skip_linear shapes of the small batches; never the headline shapes."""
    from uspace_amd import _hip
    L = _hip.lib()
    ws = L.uspace_gemm_split_ws_bytes
    assert ws(4 * 257, 512, 2048) == 4 * 4 * 257 * 512 * 4          # U-ViT-S fc2, batch 4: 36 tiles x 4 ranges
    assert ws(4 * 257, 512, 1024) == 2 * 4 * 257 * 512 * 4          # ... skip_linear: K = 1024 only with <= 40 tiles
    assert ws(4 * 257, 1024, 4096) == 2 * 4 * 257 * 1024 * 4        # U-ViT-L fc2, batch 4: 72 tiles x 2 ranges
    assert ws(4 * 257, 1024, 1024) == 0 and ws(4 * 257, 512, 512) == 0 and ws(4 * 257, 1536, 512) == 0
    for M in (32 * 257, 64 * 257, 64 * 334):
        for N, K in ((1024, 4096), (1024, 2048), (512, 2048), (4096, 1024)):
            assert ws(M, N, K) == 0
    assert ws(0, 512, 2048) == 0 and ws(1028, 512, 100) == 0


def test_gemm_plans_cover_the_rows_and_waste_little_of_a_round():
    """uspace_gemm_plan over the row counts of every BASELINE configuration (B*L: 4*257, 32*257, 32*334, 64*257, 64*334) and
    every output width of the two model sizes: the tile rows plus the 16-row strips cover M exactly, strips never outnumber
    tile rows, and the launch fills its rounds of workgroups to at least 60 % (85 % on the headline shapes) -- except where
    the whole problem is smaller than one round."""
    from uspace_amd import _hip
    L = _hip.lib()
    out = (ctypes.c_int * 8)()
    worst = {}
    for M in (4 * 257, 32 * 257, 32 * 334, 64 * 257, 64 * 334):
        for N in (512, 1024, 1536, 2048, 3072, 4096):
            assert L.uspace_gemm_plan(M, N, out) == 0
            choice, split, BM, BN, tm, tn, ns, per_round = list(out)
            rows = split if choice == 3 else M
            assert tm * BM + 16 * ns >= rows > (tm - 1) * BM + (16 * (ns - 1) if ns else 0)        # covers, no empty tile row / strip
            assert 0 <= ns <= tm and tn == -(-N // BN)
            if ns:
                assert tm * BM < rows                                                               # strips only for a real remainder
            wgs = tm * tn
            rounds = -(-wgs // per_round)
            fill = wgs / (rounds * per_round)
            worst[(M, N)] = fill
            if wgs >= per_round:
                assert fill >= 0.60, (M, N, list(out), fill)
    for N in (1024, 3072, 4096):
        assert worst[(64 * 257, N)] >= 0.99                  # the headline shapes run in whole rounds (1 / 3 / 4)
    assert L.uspace_gemm_plan(64 * 257, 4096, out) == 0 and list(out)[4:7] == [64, 16, 4]            # 64 tile rows, 4 strips
    assert L.uspace_gemm_plan(0, 64, out) < 0


def test_hookplan_scalar_and_row_scales():
    from uspace_amd.libs.dissection import HookPlan
    for s in (2, 0.5, np.float32(0.5), np.float64(0.5), np.int64(2), torch.tensor(0.5), np.array(0.5), np.linspace(0, 1, 3)[1]):
        p = HookPlan("write", "f", 0, s)
        assert p.row_scales is None and p.scale == float(s), type(s)
    for s in ([0.5, 1.0], np.array([0.5, 1.0]), torch.tensor([0.5, 1.0]), torch.tensor([0.5])):
        p = HookPlan("write", "f", 0, s)
        assert p.scale == 1.0 and p.row_scales.dtype == np.float32 and p.row_scales.ndim == 1


def test_get_word_inds_reference_fixture(golden_dir):
    """tests/golden/word_inds.json: the reference's libs/clip.py:6-27 get_word_inds run on a toy word-piece tokenizer
    (generated by make_golden.py --only-word-inds); the rewritten helper must give the same token positions."""
    from uspace_amd.libs.clip import get_word_inds
    fx = json.load(open(os.path.join(golden_dir, "word_inds.json")))

    class Tok:                                            # greedy longest-match word pieces, "##" continuations
        def __init__(self, vocab):
            self.vocab = list(vocab)
            self.index = {p: i + 2 for i, p in enumerate(self.vocab)}

        def _word(self, w):
            out, pos = [], 0
            while pos < len(w):
                end = next(e for e in range(len(w), pos, -1) if (w[pos:e] if pos == 0 else "##" + w[pos:e]) in self.index)
                out.append(self.index[w[pos:end] if pos == 0 else "##" + w[pos:end]])
                pos = end
            return out

        def encode(self, text):
            return [0] + [i for w in text.split(" ") for i in self._word(w)] + [1]

        def decode(self, ids):
            return self.vocab[ids[0] - 2] if ids[0] >= 2 else ""
    tok = Tok(fx["vocab"])
    assert len(fx["cases"]) >= 20
    multi = 0
    for c in fx["cases"]:
        got = get_word_inds(c["text"], c["word_place"], tok)
        assert got.tolist() == c["expected"], c
        multi += len(c["expected"]) > 1
    assert multi >= 5                                     # words split into several pieces / repeated words are covered
    assert get_word_inds("a photo of a running dog", [0, 4], tok).tolist() == sorted(
        get_word_inds("a photo of a running dog", 0, tok).tolist() + get_word_inds("a photo of a running dog", 4, tok).tolist())


def test_built_library_matches_the_sources_in_the_tree():
    """The .so is git-ignored and travels prebuilt.  build() leaves uspace_amd/csrc/_build/BUILD_STAMP.json (sha256 of the library
    and of every source it was built from): the library in the tree must be that library, built from the sources in the tree."""
    import sys
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    path = os.path.join(ROOT, "uspace_amd", "csrc", "_build", "BUILD_STAMP.json")
    if not os.path.exists(path):
        pytest.skip("no build stamp: __graft_entry__.build() has not run in this checkout")
    old, now = json.load(open(path)), ge.build_stamp()
    assert old["library_sha256"] == now["library_sha256"], "libuspace_hip.so changed since build() stamped it"
    assert old["sources"] == now["sources"], [k for k in now["sources"] if old["sources"].get(k) != now["sources"][k]]
    assert "uspace_amd/csrc/gemm.hip" in now["sources"]


def test_ring_form_tiny_launches_plan_for_two_workgroups_per_cu():
    """The 64x64 ring form holds 66-74 KiB of LDS: 512 workgroups per round, and a remainder of a few rows is a strip, not a second
    round (fc1 of U-ViT-L at 2 x 257 rows: 8 x 64 workgroups + one strip instead of 9 x 64).  The two-stage form keeps 1024."""
    from uspace_amd import _hip
    L = _hip.lib()
    out = (ctypes.c_int * 8)()
    assert L.uspace_gemm_plan_k(514, 4096, 1024, 0, out) == 0          # 16 K tiles: the ring form
    assert list(out)[:1] == [5] and (out[2], out[3]) == (64, 64)
    assert (out[4], out[5], out[6], out[7]) == (8, 64, 1, 512)
    assert L.uspace_gemm_plan_k(1028, 2048, 512, 0, out) == 0          # 8 K tiles, 544 tiles: the two-stage form
    assert out[0] == 5 and (out[4], out[5], out[7]) == (17, 32, 1024)
    assert L.uspace_gemm_plan_k(1028, 512, 512, 1, out) == 0           # proj of U-ViT-S at 4 x 257 rows: ring, one round either way
    assert out[0] == 5 and (out[4], out[5], out[6], out[7]) == (17, 8, 0, 512)


def test_cnf_reuses_the_device_scalars_of_its_time_grid():
    """CNFBase._timesteps on a fixed grid: one 0-dim tensor per distinct time (never written again), expanded per call -- no fill
    launch per evaluation; bounded, oldest first.  Error-controlled solves (no two times alike) get a fresh scalar per call."""
    from uspace_amd.flow_matching import CNF

    class Net(torch.nn.Module):
        def forward(self, x, t, y=None, **kw):
            return x, None

    cnf = CNF(Net())
    x = torch.zeros(3, 4, 2, 2)
    f1, _ = cnf._timesteps(0.25, x)
    f2, th2 = cnf._timesteps(0.25, x)
    assert f1.data_ptr() != f2.data_ptr() and th2 == 0.25 and not cnf.__dict__.get("_t_scalars")      # adaptive: nothing cached
    cnf._grid_is_fixed = True
    a, th = cnf._timesteps(0.25, x)
    b, _ = cnf._timesteps(torch.tensor(0.25), x)
    c, _ = cnf._timesteps(0.5, x)
    assert th == 0.25 and a.shape == (3,) and a.stride(0) == 0 and float(a[0]) == 0.25 and float(c[2]) == 0.5
    assert a.data_ptr() == b.data_ptr() != c.data_ptr()
    per_sample = torch.tensor([0.1, 0.2, 0.3])
    d, thd = cnf._timesteps(per_sample, x)
    assert d is per_sample and thd is None
    for k in range(cnf._T_SCALARS_MAX + 5):
        cnf._timesteps(10.0 + k, x)
    assert len(cnf._t_scalars) == cnf._T_SCALARS_MAX and (x.device, 0.25) not in cnf._t_scalars
    # which solves run on a fixed grid: euler / n_steps do, plain dopri5 does not
    sk = dict(solver="fixed", solver_fix="euler", solver_fix_step=0.5, solver_adaptive="dopri5", solver_adaptive_prec=1e-3)
    cnf2 = CNF(Net())
    cnf2.state_ops_factory = TorchCpuOps
    cnf2.decode(x, None, dissect_name="w", edit_loc=None, solver_kwargs=sk)
    assert sorted(k[1] for k in cnf2._t_scalars) == [0.0, 0.5]
    # the flag lives for the duration of a solve only: a call outside one gets a fresh scalar and leaves the cache alone
    assert not cnf2._grid_is_fixed
    o1, _ = cnf2._timesteps(0.5, x)
    o2, _ = cnf2._timesteps(0.5, x)
    assert o1.data_ptr() != o2.data_ptr() and len(cnf2._t_scalars) == 2
    cnf2.decode(x, None, dissect_name="w", edit_loc=None, solver_kwargs=dict(sk, solver="adaptive"))
    assert not cnf2._grid_is_fixed and len(cnf2._t_scalars) == 2                                        # untouched by the adaptive solve
    cnf2.decode(x, None, dissect_name="w", edit_loc=None, solver_kwargs=dict(sk, solver="adaptive", n_steps=4))
    assert not cnf2._grid_is_fixed and len(cnf2._t_scalars) > 2                                         # dopri5 on 4 equal steps cached its times


def test_graph_replay_is_opt_in(monkeypatch):
    from uspace_amd.tools.utils_uvit import get_nnet
    kw = dict(img_size=8, patch_size=2, in_chans=4, embed_dim=64, depth=2, num_heads=1, mlp_ratio=4, qkv_bias=False,
              mlp_time_embed=False, num_classes=-1)
    monkeypatch.delenv("USPACE_UVIT_GRAPH", raising=False)
    assert get_nnet("uvit", **kw).use_graph is False
    monkeypatch.setenv("USPACE_UVIT_GRAPH", "1")
    assert get_nnet("uvit", **kw).use_graph is True


def test_lab_hook_cannot_reach_a_product_build():
    """gemm.hip's lab hook (the tile-form override) exists only under -DUSPACE_LAB=1, which only the lab build script defines: csrc/Makefile
    builds with -DUSPACE_LAB=0 -Werror=undef, and the hook's code is not in what that build compiles; the switches that produced wrong
    results on purpose (ablations, same-panel staging) and the retired lab forms (four-wave, chain) are gone from the source (patches under
    tools/lab/dropped/, or the last commit that held them), and no build debris (-save-temps output) is tracked next to the sources."""
    import shutil
    import subprocess
    csrc = os.path.join(ROOT, "uspace_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "-DUSPACE_LAB=0" in mk and "-Werror=undef" in mk and "USPACE_LAB=1" not in mk and "gemm4" not in mk
    assert "-DUSPACE_LAB=1" in open(os.path.join(ROOT, "tools", "lab", "build_variant.sh")).read()
    src = open(os.path.join(csrc, "gemm.hip")).read()
    for gone in ("USPACE_ABLATE", "USPACE_SAME_PANELS", "USPACE_DMA_FLAT", "USPACE_KTRACE", "USPACE_FULL_LINES", "K_STAMP", "USPACE_FORM4", "USPACE_CHAIN"):
        assert gone not in src, gone
    # every lab-only region is fenced by the VALUE of the lab flag, which is 0 in a product build
    for m in re.finditer(r"^#\s*if\s+(.*)$", src, re.M):
        cond = m.group(1)
        if "USPACE_" in cond and "defined" not in cond:
            assert re.fullmatch(r"!?USPACE_LAB\s*", cond), cond
    hipcc = "/opt/rocm/bin/hipcc"
    if os.path.exists(hipcc):
        base = [hipcc, "-std=c++17", "--offload-arch=gfx950", "--cuda-host-only", "-E", "-o", "-", os.path.join(csrc, "gemm.hip")]
        product = subprocess.run(base + ["-DUSPACE_LAB=0", "-Werror=undef"], capture_output=True, text=True)
        assert product.returncode == 0, product.stderr[-300:]
        assert "uspace_lab_gemm_force_tile" not in product.stdout and "g_force_tile" not in product.stdout
        lab = subprocess.run(base + ["-DUSPACE_LAB=1", "-DUSPACE_SK_MIN_NK=16", "-DUSPACE_SK_MIN_KT=4"], capture_output=True, text=True)
        assert lab.returncode == 0 and "uspace_lab_gemm_force_tile" in lab.stdout, lab.stderr[-300:]
    if shutil.which("git") and os.path.isdir(os.path.join(ROOT, ".git")):
        tracked = subprocess.run(["git", "-C", ROOT, "ls-files", "uspace_amd"], capture_output=True, text=True).stdout.split()
        junk = [f for f in tracked if f.endswith((".s", ".bc", ".hipi", ".o", ".so")) or "/lib.so." in f or "hipv4-amdgcn" in f]
        assert not junk, junk


def test_gelu_polynomial_in_the_header_keeps_its_stated_accuracy():
    """The fused erf-GELU epilogue evaluates exp2 of a polynomial (uspace_amd/csrc/common.h, US_GELU_C*; fitted by tools/fit_gelu.py).
    The coefficients as committed, evaluated the way the kernel does (fp32 Horner, one rounding per fma), stay within the bounds the
    header states against the exact erfc form of nn.GELU (reference libs/timm.py:97) -- three orders of magnitude below the bf16
    rounding of the stored activation; the GPU parity tests compare the kernel itself with libm's erf."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("fit_gelu", os.path.join(ROOT, "tools", "fit_gelu.py"))
    fg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fg)
    c = fg.header_coefficients()
    assert len(c) == 7                                       # degree 6: the kernel's Horner chain is written for exactly that
    e_abs, e_rel = fg.errors(c)
    assert e_abs <= 4.1e-7 and e_rel <= 1.0e-6, (e_abs, e_rel)


def test_two_workspaces_stay_resident_lru():
    """The write_scales sweep (one 9 x B solve) next to plain B solves alternates two batch sizes: neither switch reallocates;
    a third size evicts the least recently used one.  (Sizes come from the library's own query; CPU memory stands in here.)"""
    from uspace_amd.tools.utils_uvit import get_nnet
    net = get_nnet("uvit", img_size=8, patch_size=2, in_chans=4, embed_dim=64, depth=2, num_heads=1, mlp_ratio=4, qkv_bias=False,
                   mlp_time_embed=False, num_classes=-1)
    cpu = torch.device("cpu")
    a, b = net._workspace_for(10, cpu), net._workspace_for(90, cpu)
    assert a.numel() < b.numel() and len(net._workspace) == 2
    for _ in range(3):
        assert net._workspace_for(10, cpu) is a and net._workspace_for(90, cpu) is b
    c = net._workspace_for(4, cpu)                       # least recently used is B = 10
    assert list(net._workspace) == [(90, "cpu"), (4, "cpu")] and net._workspace_for(90, cpu) is b
    assert net._workspace_for(4, cpu) is c and net._workspace_for(10, cpu) is not a and len(net._workspace) == 2
