"""tests/attention_long_cases.py pinned on the CPU: the coverage of its case list, its plan mirror against uspace_attention_long_plan of
the built library, the float64 model of the streamed arithmetic against the plain float64 softmax on every case (the measurement behind
ROW_MODEL), and the sensitivity of every bound of tests/test_gpu_attention_long.py: each faulty reference lies at least twice the bound
away from the true one, in the metric the GPU test uses."""
import ctypes
import importlib.util
import os

import pytest
import torch

from tests import attention_cases as AC
from tests import attention_long_cases as LC
from tests import uvit_stages as S

TOL = AC.TOL
FACTOR = 2.0
USPACE_ERR_ARG = -1
REF_CHUNK = 32


# ------------------------------------------------------------------------------------------------------------------ coverage
def test_cases_cover_the_lengths_and_both_sides_of_the_plan_switch():
    assert len(set(LC.CASES)) == len(LC.CASES)
    assert set(LC.REQUIRED_L) <= {c[1] for c in LC.CASES}
    assert {c[4] for c in LC.CASES} == set(AC.DATA_SETS)
    assert all(c[0] <= 2 and c[2] <= 2 for c in LC.CASES if c[1] > 6 * LC.KT + 1)
    assert all(c[0] >= 2 for c in LC.CASES if c[3])                                       # the all-zero key_scale row
    for L in (17, 129, 337):                                                              # B * H right below and at the switch
        bh = LC.switch_bh(L)
        assert {bh - 1, bh} <= {c[0] * c[2] for c in LC.CASES if c[1] == L}
        assert LC.plan(bh - 1, L, 1, False)[1] == 64 and LC.plan(bh, L, 1, False)[1] == 128
    for scaled in (False, True):
        assert {LC.plan(*c[:4])[1] for c in LC.CASES if c[3] == scaled} == {64, 128}
        assert {c[1] for c in LC.CASES if c[3] == scaled} >= {337, 1025, 1102, 2049}
    # 'edges' (the rescale in both directions: sink on key 0, dominant key L - 1) at the long lengths
    assert {c[1] for c in LC.CASES if c[4] == "edges"} >= {337, 1025, 1102, 2049}
    assert set(LC.SHARED_L) <= {c[1] for c in LC.CASES} and max(LC.SHARED_L) <= LC.RESIDENT_MAX_L


# ------------------------------------------------------------------------------------------------------------------ plan
PLAN_BH = (1, 2, 3, 4, 5, 7, 15, 16, 28, 29, 56, 57, 63, 64, 65, 127, 128, 129, 170, 171, 255, 256, 257, 511, 512, 513, 1024, 2048)


def test_mirror_matches_the_plan_of_the_built_library():
    """uspace_attention_long_plan (host-side, no GPU) against the mirror for L = 1 .. 2 100, both key_scale settings and B * H around
    every value at which the switch can fall (512 / ceil(L / 128): 512, 256, 171, 128, 103, ..., 31), as B x 1 head and B / 16 x 16."""
    from uspace_amd import _hip
    plan = _hip.lib().uspace_attention_long_plan
    out = (ctypes.c_int * 6)()
    seen = set()
    for L in range(1, 2101):
        sw = LC.switch_bh(L)
        shapes = [(bh, 1) for bh in PLAN_BH + (sw - 1, sw, sw + 1) if bh > 0] + [(bh // 16, 16) for bh in PLAN_BH if bh % 16 == 0]
        for scaled in (0, 1):
            for B, H in shapes:
                assert plan(B, L, H, scaled, out) == 0, (B, L, H, scaled)
                assert tuple(out) == LC.plan(B, L, H, scaled), (B, L, H, scaled, list(out))
                assert out[5] <= 80 * 1024 and out[3] == B * H * -(-L // out[1])
                seen.add(out[1])
    assert seen == {64, 128}


def test_plan_refuses_bad_arguments():
    from uspace_amd import _hip
    L_ = _hip.lib()
    out = (ctypes.c_int * 6)()
    big = 2 ** 31 - 1
    for B, L, H in ((0, 400, 1), (1, 0, 1), (1, 400, 0), (-1, 400, 1), (1, -5, 1), (1, 400, -2),
                    (2 ** 16, 2 ** 15, 1),          # B * L = 2^31
                    (1, 400, big // 192 + 1),       # 3 * H * 64 > INT_MAX
                    (2 ** 16, 400, 2 ** 15),        # B * H = 2^31
                    (2 ** 10, 2 ** 20, 2 ** 10)):   # the grid
        for scaled in (0, 1):
            assert L_.uspace_attention_long_plan(B, L, H, scaled, out) == USPACE_ERR_ARG, (B, L, H)
    assert L_.uspace_attention_long_plan(1, 400, 1, 0, None) == USPACE_ERR_ARG
    assert L_.uspace_attention_long_plan(2 ** 10, 2 ** 20, 1, 0, out) == 0            # B * L = 2^30 fits
    # the launch refuses the same before it touches the GPU
    for B, L, H in ((0, 400, 1), (1, 0, 1), (1, 400, 0), (2 ** 16, 2 ** 15, 1)):
        assert L_.uspace_attention_long_bf16(ctypes.c_void_p(64), None, ctypes.c_void_p(64), B, L, H, None) == USPACE_ERR_ARG
    assert L_.uspace_attention_long_bf16(None, None, ctypes.c_void_p(64), 1, 400, 1, None) == USPACE_ERR_ARG
    assert L_.uspace_attention_long_bf16(ctypes.c_void_p(64), None, None, 1, 400, 1, None) == USPACE_ERR_ARG
    # the resident form keeps its limit
    o8 = (ctypes.c_int * 8)()
    assert L_.uspace_attention_plan(1, 336, 1, 0, o8) == 0 and L_.uspace_attention_plan(1, 337, 1, 0, o8) == USPACE_ERR_ARG


def test_kernel_uses_no_scratch_and_fits_two_workgroups_per_cu():
    """Code-object metadata of the built library (tools/kernel_resources.py; no GPU): the four instantiations of attn_stream_kernel
    (key_scale or not x one or two query tiles per wave), none with scratch, none above the 256 registers that let two 4-wave
    workgroups share a CU.  Its name stays clear of the resident kernel's, which tests/test_attention_cases.py matches by substring."""
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"):
        pytest.skip("llvm-objdump not available")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(root, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    ks = [k for k in kr.kernels() if "attn_stream_kernel" in k["name"]]
    assert len(ks) == 4 and not any("attention_kernel" in k["name"] for k in ks)
    for k in ks:
        assert k["scratch"] == 0 and k["vgpr"] + k["agpr"] <= 256 and k["wg"] == 64 * LC.NW, k


# ------------------------------------------------------------------------------------------------------------------ the model
def test_model_is_the_plain_softmax_without_rounding_and_for_one_tile():
    x = AC.make_qkv(2, 150, 2, "edges").to(torch.float64)
    ks = AC.make_key_scale(2, 150).to(torch.float64)
    for k in (None, ks):
        assert float((LC.streamed_attention(x, 2, False, k) - S.attention(x, 2, False, k)).abs().max()) < 1e-12
        # one tile that holds every key: the resident kernel's arithmetic, bit for bit
        assert torch.equal(LC.streamed_attention(x, 2, True, k, kt=150), S.attention(x, 2, True, k))
    assert float((LC.rescale_dropped(x, 2, False) - S.attention(x, 2, False)).abs().max()) > 1e-2
    y = AC.make_qkv(2, 60, 2, "edges").to(torch.float64)                                   # one key tile: nothing to rescale
    assert torch.equal(LC.rescale_dropped(y, 2, True), LC.streamed_attention(y, 2, True))


_MODEL = {}


def _model_figures(case):
    if case not in _MODEL:
        B, L, H, scaled, data = case
        qkv = AC.make_qkv(B, L, H, data)
        ks = AC.make_key_scale(B, L) if scaled else None
        head = row = env = 0.0
        for i in range(0, B * H, REF_CHUNK):
            heads = list(range(i, min(B * H, i + REF_CHUNK)))
            model = AC.reference(qkv, H, heads, True, ks, fn=LC.streamed_attention).numpy()
            plain = AC.reference(qkv, H, heads, False, ks).numpy()
            ksh = None if ks is None else ks[torch.as_tensor(heads) // H]
            a = TOL["env_a"] * AC.envelope_a(AC.head_qkv(qkv, H, heads), ksh)
            head, row = max(head, AC.head_err(model, plain)), max(row, AC.row_err(model, plain))
            env = max(env, AC.envelope_excess(model, plain, TOL["env_k"], a))
        _MODEL[case] = dict(head=head, row=row, env=env)
    return _MODEL[case]


@pytest.mark.parametrize("case", LC.CASES, ids=AC.case_id)
def test_streamed_model_against_plain_float64(case):
    """The float64 model of the streamed arithmetic stays within the project's head bound of the plain float64 softmax, inside the
    analytic envelope, and its worst query row within ROW_MODEL (the table holds the worst value this test measures over CASES)."""
    n = S.cpu_threads()
    try:
        f = _model_figures(case)
        print(f"\n[model {AC.case_id(case)}] head={f['head']:.3e} row={f['row']:.3e} env={f['env']:.3f}")
        assert f["head"] <= AC.tol("att_loose", case[3]), f
        assert f["env"] <= 1.0, f
        assert f["row"] <= LC.ROW_MODEL["ks" if case[3] else "plain"], f
    finally:
        torch.set_num_threads(n)


def test_row_model_table_is_what_the_cases_measure():
    """ROW_MODEL is the measurement, not a loosened one: the worst case reaches at least 0.9 of its entry."""
    n = S.cpu_threads()
    try:
        for scaled, key in ((False, "plain"), (True, "ks")):
            worst = max(_model_figures(c)["row"] for c in LC.CASES if c[3] == scaled)
            assert 0.9 * LC.ROW_MODEL[key] <= worst <= LC.ROW_MODEL[key], (key, worst)
    finally:
        torch.set_num_threads(n)


# ------------------------------------------------------------------------------------------------------------------ sensitivity
def _distances(fault, data, L, env, with_ks):
    fn = LC.PERTURBED[fault][0]
    B, H = 3, 2
    qkv = AC.make_qkv(B, L, H, data)
    ks = AC.make_key_scale(B, L) if with_ks else None
    heads = list(range((B - 1) * H))                                  # (not the sample whose key_scale row is 0)
    true = AC.reference(qkv, H, heads, False, ks).numpy()             # the GPU test's reference: plain float64
    bad = AC.reference(qkv, H, heads, True, ks, fn=fn).numpy()        # what a faulty kernel would store
    sfx = "_ks" if with_ks else ""
    if env:
        ksh = None if ks is None else ks[torch.as_tensor(heads) // H]
        a = TOL["env_a"] * AC.envelope_a(AC.head_qkv(qkv, H, heads), ksh)
        return {"envelope": AC.envelope_excess(bad, true, TOL["env_k"], a)}
    return {"att_loose" + sfx: AC.head_err(bad, true) / AC.tol("att_loose", with_ks),
            "row" + sfx: AC.row_err(bad, true) / LC.row_bound(with_ks)}


@pytest.mark.parametrize("L", [337, 1025])
@pytest.mark.parametrize("fault", sorted(LC.PERTURBED))
def test_every_bound_separates_every_fault(fault, L):
    """distance(faulty reference, plain float64) >= 2 x bound for the head bound, the row bound and the envelope, on the data sets meant
    to expose the fault; the faults that do not need key_scale are tried without and with it.  See the printed ratios (pytest -s)."""
    n = S.cpu_threads()
    try:
        _, needs_ks, rel_sets, env_sets, ks_sets = LC.PERTURBED[fault]
        runs = [(False, d, needs_ks) for d in rel_sets] + [(True, d, needs_ks) for d in env_sets]
        runs += [(env, d, True) for d in ks_sets for env in (False, True)]
        ratios = {}
        for env, data, with_ks in runs:
            for k, v in _distances(fault, data, L, env, with_ks).items():
                ratios[(k, data, "ks" if with_ks else "plain")] = v
        print(f"\n[sensitivity {fault} L={L}] " + " ".join(f"{k}/{d}/{w}={v:.3g}" for (k, d, w), v in sorted(ratios.items())))
        assert {k.split("_ks")[0] for k, _, _ in ratios} == {"att_loose", "row", "envelope"}
        assert min(ratios.values()) >= FACTOR, ratios
    finally:
        torch.set_num_threads(n)
