"""CPU-only checks of the feature-set metrics: the inputs and float64 references of tests/metric_cases.py (near-tie guard,
a hand-computed example, planted faults), the host logic of uspace_amd/tools/feature_metrics.py and the ABI surface."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import metric_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("uspace_metric_workspace_bytes", "uspace_metric_knn_radius2", "uspace_metric_manifold", "uspace_metric_poly_sums")


# ------------------------------------------------------------------------------------------- the cases
@pytest.mark.parametrize("case", MC.CASES, ids=str)
def test_no_near_ties(case):
    """A condition on the inputs, not a tolerance: no membership or coverage decision of a case has a relative gap
    |d^2 - r^2| / r^2 below 1e-6, which is what lets the GPU test demand exact equality of every count and boolean.  A case
    that breaks it is replaced, not skipped."""
    p = MC.parts_of(case)
    gap = MC.min_decision_gap(p)
    print(f"{case}: smallest relative decision gap {gap:.3e}")
    assert gap >= MC.MIN_DECISION_GAP
    # the ceiling of the GPU's distance error, relative to d^2, stays far below that gap
    real, fake = MC.sets_of(case)
    nr, nf = MC.ref_norms2(real), MC.ref_norms2(fake)
    worst = float(((nf[:, None] + nr[None, :]) / p["d_fr"]).max())
    assert MC.DIST_FACTOR * case[3] * MC.U * worst < 1e-2 * MC.MIN_DECISION_GAP


def test_cases_are_non_trivial():
    """The reference's numbers for the cases (recorded to three decimals): every quantity is away from 0 and 1 except in the
    deliberately tiny case 4."""
    want = {0: (0.844, 0.297, 1.510, 0.667), 1: (0.798, 0.443, 1.517, 0.757), 2: (0.719, 0.078, 1.906, 0.395),
            3: (0.846, 0.446, 1.285, 0.877), 4: (1.000, 1.000, 0.949, 1.000), 6: (0.984, 0.641, 1.178, 0.719),
            7: (0.878, 0.465, 1.430, 0.670)}
    for case in MC.CASES:
        r = MC.prdc_from_parts(MC.parts_of(case), case[4])
        got = (r["precision"], r["recall"], r["density"], r["coverage"])
        assert np.allclose(got, want[case[0]], atol=5.1e-4), (case, got)


def test_hand_made_example():
    """Six points in the plane, k = 1.  real = (0,0) (3,0) (0,4), fake = (1,0) (3,1) (10,10).
    Radii: real 9, 9, 16 (|R0R1|^2 = 9, |R0R2|^2 = 16, |R1R2|^2 = 25); fake 5, 5, 130 (|G0G1|^2 = 5, |G0G2|^2 = 181, |G1G2|^2 = 130).
    D2(fake_j, real_i): G0: 1, 4, 17;  G1: 10, 1, 18;  G2: 200, 149, 136.
    Real balls holding G0: R0, R1 (17 > 16); G1: R1 alone (10 > 9, 18 > 16); G2: none  -> counts 2, 1, 0: precision 2/3, density 3/3.
    Fake balls holding R0: G0 (1 <= 5); R1: G0, G1 (4, 1 <= 5); R2: none (17, 18 > 5; 136 > 130) -> counts 1, 2, 0: recall 2/3.
    Nearest fake of R0, R1, R2: 1, 1, 17 against radii 9, 9, 16 -> coverage 2/3."""
    p = MC.ref_parts(MC.HAND_REAL, MC.HAND_FAKE, 1)
    assert p["r_real"].tolist() == [9, 9, 16] and p["r_fake"].tolist() == [5, 5, 130]
    assert p["d_fr"].tolist() == [[1, 4, 17], [10, 1, 18], [200, 149, 136]]
    assert p["count_f"].tolist() == [2, 1, 0] and p["count_r"].tolist() == [1, 2, 0] and p["min_r"].tolist() == [1, 1, 17]
    assert MC.prdc_from_parts(p, 1) == dict(precision=2 / 3, recall=2 / 3, density=1.0, coverage=2 / 3)
    # K(a, b) = (a.b + 1)^2 over all three of each set, x = fake: G0.G1 = 3, G0.G2 = 10, G1.G2 = 40 -> 2 (16 + 121 + 1681) = 3636;
    # every product of two real points is 0 -> 6; fake x real: (1, 16, 1) + (1, 100, 25) + (1, 961, 1681) = 2787
    idx = np.arange(3, dtype=np.int32)[None]
    sums, major = MC.ref_poly_sums(MC.HAND_FAKE, MC.HAND_REAL, idx, idx, 2, 1.0, 1.0)
    assert sums.tolist() == [[3636, 6, 2787]] and major.tolist() == sums.tolist()
    assert MC.mmd2(sums, 3)[0] == pytest.approx(3636 / 6 + 6 / 6 - 2 * 2787 / 9, rel=1e-15)


def test_planted_faults_move_the_results():
    """Each planted fault moves at least one case by more than 100 x the GPU bound: the PRDC numbers are held to exact equality,
    so any change of a count shows, and it must be at least one sample's worth; KID is held to the propagated bound of the sums."""
    for fault in MC.PRDC_FAULTS:
        moved = 0.0
        for case in MC.CASES:
            real, fake = MC.sets_of(case)
            good = MC.prdc_from_parts(MC.parts_of(case), case[4])
            bad = MC.ref_prdc(real, fake, case[4], fault)
            moved = max(moved, max(abs(good[k] - bad[k]) for k in good))
        print(f"{fault}: largest change of a PRDC number {moved:.3f}")
        assert moved > 1.0 / 300, fault
    real, fake = MC.sets_of(MC.CASES[0])
    good = MC.prdc_from_parts(MC.parts_of(MC.CASES[0]), 3)
    bad = MC.ref_prdc(real, fake, 3, "self_in_radius")
    assert round(good["precision"], 3) == 0.844 and round(bad["precision"], 3) == 0.817
    assert round(good["recall"], 3) == 0.297 and round(bad["recall"], 3) == 0.240
    for fault in MC.KID_FAULTS:
        ratio = 0.0
        for case in MC.KID_CASES:
            real, fake = MC.sets_of(case)
            for degree in (1, 3):
                good = MC.ref_kid(fake, real, 7, 17, degree=degree)
                bad = MC.ref_kid(fake, real, 7, 17, degree=degree, fault=fault)
                ratio = max(ratio, abs(good["mean"] - bad["mean"]) / good["mean_bound"])
        print(f"{fault}: KID mean moves by {ratio:.3e} x its bound")
        assert ratio > 100, fault


# ------------------------------------------------------------------------------------------- host logic
def _cpu_sets(n_real=30, n_fake=20, F=8):
    g = torch.Generator().manual_seed(0)
    return torch.randn(n_real, F, generator=g), torch.randn(n_fake, F, generator=g)


def test_value_errors_come_before_any_device_work():
    from uspace_amd.tools.feature_metrics import FeatureBank, kid_score, prdc
    real, fake = _cpu_sets()
    for size in (1, 21, 31):                                  # below 2, above the smaller set, above both
        with pytest.raises(ValueError):
            kid_score(fake, real, subsets=2, subset_size=size)
    with pytest.raises(ValueError):
        kid_score(fake, real, subsets=2, subset_size=5, degree=0)
    with pytest.raises(ValueError):
        kid_score(fake, real[:, :4], subsets=2, subset_size=5)
    for k in (0, 17, 20, 1.5):                                # below 1, above 16, above n_fake - 1, not an integer
        with pytest.raises(ValueError):
            prdc(real, fake, nearest_k=k)
    with pytest.raises(ValueError):
        prdc(real[:5], fake, nearest_k=5)                     # n_real - 1 = 4
    with pytest.raises(ValueError):
        FeatureBank(dims=100, device="cpu")
    with pytest.raises(ValueError):
        FeatureBank(dims=64, device="cpu").update_features(torch.zeros(3, 65))
    with pytest.raises(ValueError):
        FeatureBank.from_features(torch.zeros(7))


def test_cpu_tensors_raise_uspace_hip_error():
    """Valid arguments on the CPU get as far as the kernel call's device check: there is no CPU path."""
    from uspace_amd._hip import UspaceHipError
    from uspace_amd.tools.feature_metrics import FeatureBank, kid_score, prdc
    real, fake = _cpu_sets()
    with pytest.raises(UspaceHipError):
        kid_score(fake, real, subsets=2, subset_size=5)
    with pytest.raises(UspaceHipError):
        prdc(real, fake, nearest_k=5)
    with pytest.raises(UspaceHipError):
        prdc(FeatureBank.from_features(real), FeatureBank.from_features(fake), nearest_k=3)


def test_subset_draw_order_is_pinned():
    """seed = 2020, n = (30 fake, 20 real), m = 5, two subsets: per subset the fake draw comes first, then the real one, from one
    np.random.RandomState(seed).  The indices were recorded from numpy's legacy generator, whose stream is frozen."""
    from uspace_amd.tools.feature_metrics import draw_subsets
    idx_f, idx_r = draw_subsets(30, 20, 2, 5, 2020)
    assert idx_f.dtype == np.int32 and idx_r.dtype == np.int32
    assert idx_f.tolist() == [[14, 17, 19, 20, 23], [13, 28, 25, 12, 24]]
    assert idx_r.tolist() == [[5, 8, 10, 0, 13], [8, 12, 6, 9, 4]]
    ref_f, ref_r = MC.draw_subsets_ref(30, 20, 2, 5, 2020)
    assert (ref_f == idx_f).all() and (ref_r == idx_r).all()


def test_mmd2_unbiased_formula():
    from uspace_amd.tools.feature_metrics import mmd2_unbiased
    sums = np.array([[3636.0, 6.0, 2787.0], [12.0, 6.0, 9.0]])
    got = mmd2_unbiased(sums, 3)
    assert got.dtype == np.float64
    assert got.tolist() == [3636 / 6 + 6 / 6 - 2 * 2787 / 9, 12 / 6 + 6 / 6 - 2 * 9 / 9]


def test_feature_bank_on_cpu_tensors(tmp_path):
    """Storage, growth by chunks, dtype conversion, save and load need no kernel."""
    from uspace_amd.tools.feature_metrics import FeatureBank
    bank = FeatureBank(dims=64, device="cpu")
    assert len(bank) == 0 and tuple(bank.features.shape) == (0, 64)
    g = torch.Generator().manual_seed(1)
    parts = [torch.randn(n, 64, generator=g) for n in (3, 1500, 700)]          # crosses the first chunk and forces a regrowth
    bank.update_features(parts[0])
    bank.update_features(parts[1].double())
    bank.update_features(parts[2].to(torch.bfloat16))
    bank.update_features(torch.zeros(0, 64))
    want = torch.cat([parts[0], parts[1].double().float(), parts[2].to(torch.bfloat16).float()])
    assert len(bank) == 2203 and bank.features.dtype == torch.float32 and torch.equal(bank.features, want)
    path = str(tmp_path / "bank.npz")
    bank.save(path)
    with np.load(path) as f:
        assert list(f.keys()) == ["features"] and f["features"].dtype == np.float32 and f["features"].shape == (2203, 64)
    back = FeatureBank.load(path, device="cpu")
    assert len(back) == 2203 and back.dims == 64 and torch.equal(back.features, want)
    bank.reset()
    assert len(bank) == 0 and tuple(bank.features.shape) == (0, 64)
    clip = FeatureBank.from_features(torch.ones(4, 768, dtype=torch.float64))   # any width: the CLIP embeddings
    assert clip.dims == 768 and clip.features.dtype == torch.float32 and len(clip) == 4
    with pytest.raises(ValueError):
        clip.update(torch.zeros(1, 3, 8, 8))                                    # no model behind arbitrary features


def test_path_functions_mirror_the_fid_signature():
    import inspect
    from uspace_amd.tools import feature_metrics as FM
    from uspace_amd.tools.fid_score import calculate_fid_given_paths
    fid = inspect.signature(calculate_fid_given_paths).parameters
    for fn, extra in ((FM.calculate_prdc_given_paths, ["nearest_k"]), (FM.calculate_kid_given_paths, [])):
        got = inspect.signature(fn).parameters
        names = [n for n in got if n not in extra and got[n].kind is not inspect.Parameter.VAR_KEYWORD]
        assert names == list(fid)
        for n in fid:
            assert got[n].default == fid[n].default, n
    assert inspect.signature(FM.calculate_prdc_given_paths).parameters["nearest_k"].default == 5
    with pytest.raises(RuntimeError):
        FM.calculate_prdc_given_paths(("/nonexistent/a", "/nonexistent/b"), device="cpu")


# ------------------------------------------------------------------------------------------- ABI
def test_abi_surface():
    hdr = open(os.path.join(ROOT, "include", "uspace_hip.h")).read()
    declared = set(re.findall(r"USPACE_API\s+[\w\s\*]+?\b(uspace_\w+)\s*\(", hdr))
    from uspace_amd import _hip
    lib = ctypes.CDLL(os.path.join(ROOT, "uspace_amd", "libuspace_hip.so"))
    for name in NAMES:
        assert name in declared and name in _hip.SIGNATURES and hasattr(lib, name), name
    assert re.search(r"#define USPACE_ABI_VERSION 11\b", hdr) and _hip.ABI_VERSION == 11 and _hip.lib().uspace_abi_version() == 11
    for fn in ("metric_knn_radius2", "metric_manifold", "metric_poly_sums", "metric_workspace"):
        assert callable(getattr(_hip, fn))


def test_workspace_bytes_without_gpu():
    from uspace_amd import _hip
    wb = _hip.lib().uspace_metric_workspace_bytes
    assert wb(300, 257, 0, 0) == (300 + 257) * 8
    assert wb(300, 0, 0, 0) == 300 * 8
    assert wb(300, 257, 7, 50) == (300 + 257 + 7 * 3 * 1) * 8
    assert wb(300, 257, 7, 65) == (300 + 257 + 7 * 3 * 2) * 8
    assert wb(1 << 24, 1 << 24, 0, 0) == 2 * (1 << 24) * 8
    for bad in ((0, 5, 0, 0), (-1, 5, 0, 0), (5, -1, 0, 0), ((1 << 24) + 1, 5, 0, 0), (5, (1 << 24) + 1, 0, 0), (5, 5, -1, 0),
                (5, 5, 2, 0), (5, 5, 0, -1)):
        assert wb(*bad) == 0, bad


def test_argument_errors_need_no_gpu():
    """The entry points validate before they launch: USPACE_ERR_ARG (-1) and USPACE_ERR_WORKSPACE (-3) come back without a device."""
    from uspace_amd import _hip
    L = _hip.lib()
    p = ctypes.c_void_p(64)                  # never dereferenced: every call below is refused first
    assert L.uspace_metric_knn_radius2(p, 10, 4, 10, p, p, 1 << 20, None) == -1       # k > n - 1
    assert L.uspace_metric_knn_radius2(p, 100, 4, 17, p, p, 1 << 20, None) == -1      # k > 16
    assert L.uspace_metric_knn_radius2(p, 100, 4, 0, p, p, 1 << 20, None) == -1
    assert L.uspace_metric_knn_radius2(p, 100, 0, 3, p, p, 1 << 20, None) == -1       # F < 1
    assert L.uspace_metric_knn_radius2(p, 100, 4, 3, None, p, 1 << 20, None) == -1
    assert L.uspace_metric_knn_radius2(p, 100, 4, 3, p, p, 799, None) == -3
    assert L.uspace_metric_manifold(p, 10, p, 10, 4, p, None, None, p, 1 << 20, None) == -1      # no output
    assert L.uspace_metric_manifold(p, 10, p, 10, 4, None, p, None, p, 1 << 20, None) == -1      # count without radii
    assert L.uspace_metric_manifold(p, 10, p, 10, 4, p, p, p, p, 159, None) == -3
    poly = lambda degree, m=5, ws=1 << 20: L.uspace_metric_poly_sums(p, 10, p, 10, 4, p, p, 2, m, degree, 0.25, 1.0, p, p, ws, None)
    assert poly(0) == -1 and poly(9) == -1 and poly(3, m=11) == -1 and poly(3, m=0) == -1
    assert poly(3, ws=(10 + 10 + 2 * 3) * 8 - 1) == -3
