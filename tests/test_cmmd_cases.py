"""CPU-only checks of the RBF-kernel MMD behind CMMD: the float64 reference of tests/cmmd_cases.py (planted faults, the
statistics of a set against itself, where the score sits against the sums) and what uspace_metric_rbf_sums refuses before it
launches, through the built library.  The kernel itself is checked in tests/test_gpu_cmmd.py."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from tests import cmmd_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNS = [(case, nz) for case in C.CASES for nz in C.NORMALIZE]


@pytest.mark.parametrize("case,normalize", RUNS, ids=lambda v: str(v).replace(" ", ""))
def test_every_planted_fault_moves_the_score_far_beyond_its_bound(case, normalize):
    ref = C.ref_of(case, normalize)
    assert ref["bound"] > 0 and np.all(ref["sum_bounds"] >= 0)           # (a one-row set: Sxx = 0 with a bound of 0)
    for fault in C.FAULTS:
        bad = C.ref_of(case, normalize, False, fault)
        if C.fault_applies(fault, case, normalize):
            moved = abs(bad["score"] - ref["score"])
            assert moved >= C.FAULT_MARGIN * ref["bound"], (fault, moved, ref["bound"])
        if C.fault_moves_sums(fault, normalize):
            moved = np.abs(bad["sums"] - ref["sums"])
            assert np.all(moved > 0) and np.all(moved >= C.FAULT_MARGIN * ref["sum_bounds"]), (fault, moved, ref["sum_bounds"])


def test_every_fault_is_judged_somewhere_in_every_case():
    """No fault escapes a case altogether under normalisation (the setting CMMD runs in), and only the two data-dependent ones are
    exempt without it."""
    for case in C.CASES:
        for fault in C.FAULTS:
            assert C.fault_applies(fault, case, 1) or C.fault_moves_sums(fault, 1), (case, fault)
            if fault not in ("not_normalised", "padding_columns_included"):
                assert C.fault_applies(fault, case, 0), (case, fault)


def test_the_score_lives_in_the_fourth_digit_of_the_means():
    """Normalised at sigma = 10 every kernel value is >= 0.98 while the score x 1000 is of order 1 on the clustered sets: what makes
    the fp64 fixed-order reduction necessary.  Without normalisation the kernel values span many decades (exp at large arguments)."""
    for case in C.CASES[:4]:
        r = C.ref_of(case, 1)
        assert r["kmin"] > 0.98 and 0.3 < r["score"] < 2.0, (case, r["kmin"], r["score"])
    assert min(C.ref_of(case, 0)["kmin"] for case in C.CASES) < 1e-90
    r = C.ref_of(C.CASES[4], 1)
    assert r["sums"][0] == 0.0                      # a one-row set has no off-diagonal pair


@pytest.mark.parametrize("case", C.CASES[:4], ids=str)
@pytest.mark.parametrize("normalize", C.NORMALIZE)
def test_a_set_against_itself(case, normalize):
    x, _ = C.sets_of(case)
    v = C.ref_score(x, x, C.SIGMA, bool(normalize), unbiased=False)
    u = C.ref_score(x, x, C.SIGMA, bool(normalize), unbiased=True)
    assert abs(v["score"]) <= v["bound"]
    assert u["score"] <= u["bound"]
    assert u["score"] < 0.0                         # strictly: 2 (Sxx - n (n - 1)) / (n^2 (n - 1)) with every K < 1


def test_hand_case():
    """Two points at distance 2 against one of them, sigma = 1, by hand: K = exp(-2)."""
    x = np.array([[0, 0], [2, 0]], np.float32)
    y = np.array([[0, 0]], np.float32)
    k = math.exp(-2.0)
    r = C.ref_score(x, y, sigma=1.0, normalize=False, scale=1.0)
    assert np.allclose(r["sums"], [2 * k, 0.0, 1 + k], rtol=1e-15, atol=0)
    assert abs(r["score"] - ((2 * k + 2) / 4 + 1.0 - (1 + k))) < 1e-15
    # normalised: the zero row stays the zero vector, (2, 0) becomes (1, 0): D2 = 1 between them
    r = C.ref_score(x, y, sigma=1.0, normalize=True, scale=1.0)
    assert np.allclose(r["sums"], [2 * math.exp(-0.5), 0.0, 1 + math.exp(-0.5)], rtol=1e-15, atol=0)


# ------------------------------------------------------------------------------------------- ABI
def test_symbol_is_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "uspace_hip.h")).read()
    declared = set(re.findall(r"USPACE_API\s+[\w\s\*]+?\b(uspace_\w+)\s*\(", hdr))
    from uspace_amd import _hip
    lib = ctypes.CDLL(os.path.join(ROOT, "uspace_amd", "libuspace_hip.so"))
    name = "uspace_metric_rbf_sums"
    assert name in declared and name in _hip.SIGNATURES and hasattr(lib, name)
    assert len(_hip.SIGNATURES[name][1]) == 11 and callable(_hip.metric_rbf_sums)
    assert re.search(r"#define USPACE_ABI_VERSION 11\b", hdr) and _hip.ABI_VERSION == 11 and _hip.lib().uspace_abi_version() == 11


def test_argument_errors_need_no_gpu():
    """USPACE_ERR_ARG (-1) and USPACE_ERR_WORKSPACE (-3) come back before any GPU work."""
    from uspace_amd import _hip
    L = _hip.lib()
    p = ctypes.c_void_p(64)                  # never dereferenced: every call below is refused first
    big = 1 << 30

    def rbf(x=p, nx=10, y=p, ny=20, F=4, gamma=0.005, normalize=1, sums=p, ws=p, nbytes=big):
        return L.uspace_metric_rbf_sums(x, nx, y, ny, F, gamma, normalize, sums, ws, nbytes, None)

    for kw in (dict(x=None), dict(y=None), dict(sums=None), dict(ws=None), dict(nx=0), dict(ny=0), dict(nx=-3), dict(nx=(1 << 24) + 1),
               dict(ny=(1 << 24) + 1), dict(F=0), dict(gamma=-1e-9), dict(gamma=math.inf), dict(gamma=math.nan), dict(normalize=2),
               dict(normalize=-1)):
        assert rbf(**kw) == -1, kw
    need = L.uspace_metric_workspace_bytes(10, 20, 1, 20)
    assert need == (10 + 20 + 3 * 1) * 8
    assert rbf(nbytes=need - 1) == -3 and rbf(nbytes=0) == -3
    assert L.uspace_metric_workspace_bytes(129, 257, 1, 257) == (129 + 257 + 3 * 5) * 8
    assert rbf(nx=129, ny=257, nbytes=(129 + 257 + 3 * 5) * 8 - 1) == -3
    assert rbf(nx=1 << 24, ny=1 << 24, nbytes=0) == -3            # the largest sets are sizes, not argument errors


def test_wrapper_refuses_host_tensors():
    import torch

    from uspace_amd import _hip
    x = torch.zeros(4, 8)
    with pytest.raises(_hip.UspaceHipError):
        _hip.metric_rbf_sums(x, x, 0.005)
