"""GPU checks of the feature-set metrics (uspace_amd/csrc/metrics.hip, uspace_amd/tools/feature_metrics.py) against the float64
references, cases and bounds of tests/metric_cases.py."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import metric_cases as MC

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()                # (a copy: the cached cases are read-only)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int64 if t.dtype == torch.float64 else t.dtype)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _run(real, fake, k, ws_fill=None):
    """The four launches of prdc on device tensors, optionally on workspaces filled with the byte ``ws_fill`` beforehand."""
    from uspace_amd import _hip
    ws = (lambda nx, ny=0: _hip.metric_workspace(nx, ny, device=real.device, fill=ws_fill)) if ws_fill is not None else (lambda *a: None)
    r_real = _hip.metric_knn_radius2(real, k, ws=ws(len(real)))
    r_fake = _hip.metric_knn_radius2(fake, k, ws=ws(len(fake)))
    count_f, min_f = _hip.metric_manifold(fake, real, r_real, ws=ws(len(fake), len(real)))
    count_r, min_r = _hip.metric_manifold(real, fake, r_fake, ws=ws(len(real), len(fake)))
    torch.cuda.synchronize()
    return dict(r_real=r_real, r_fake=r_fake, count_f=count_f, min_f=min_f, count_r=count_r, min_r=min_r)


@functools.lru_cache(maxsize=None)
def _gpu_of(case):
    real, fake = MC.sets_of(case)
    return _run(_dev(real), _dev(fake), case[4])


# ------------------------------------------------------------------------------------------- distances
def _distance_ratios(case):
    """Worst |got - ref| / ceiling of radius2 (both sets) and min_d2 (both directions)."""
    real, fake = MC.sets_of(case)
    p, g, F = MC.parts_of(case), _gpu_of(case), case[3]
    nr, nf = MC.ref_norms2(real), MC.ref_norms2(fake)
    rows = (("radius2 real", g["r_real"], p["r_real"], MC.dist_ceiling(nr, nr, F)),
            ("radius2 fake", g["r_fake"], p["r_fake"], MC.dist_ceiling(nf, nf, F)),
            ("min_d2 real->fake", g["min_r"], p["min_r"], MC.dist_ceiling(nr, nf, F)),
            ("min_d2 fake->real", g["min_f"], p["d_fr"].min(1), MC.dist_ceiling(nf, nr, F)))
    out = {}
    for name, got, ref, ceil in rows:
        got = got.cpu().numpy()
        assert got.dtype == np.float64 and got.shape == ref.shape and np.isfinite(got).all()
        out[name] = float((np.abs(got - ref) / ceil).max())
    return out


@pytest.mark.parametrize("case", MC.CASES, ids=str)
def test_distances(case):
    """radius2 and min_d2 against the float64 reference: |got - ref| <= 8 F 2^-53 (|x|^2 + |y|^2), the largest pair of the row."""
    ratios = _distance_ratios(case)
    print(f"{case}: worst |got - ref| / ceiling: " + ", ".join(f"{k} {v:.3e}" for k, v in ratios.items()))
    for name, r in ratios.items():
        assert r <= 1.0, (name, r)


def test_distances_scalar_load_path():
    """F % 4 != 0 takes the guarded scalar loads (rows are not 16-byte aligned) and a ragged last K step: F = 70, and F = 3 < one step."""
    from uspace_amd import _hip
    for seed, F in ((11, 70), (12, 3)):
        real, fake = MC.make_sets(seed, 40, 33, F)
        p = MC.ref_parts(real, fake, 2)
        g = _run(_dev(real), _dev(fake), 2)
        nr, nf = MC.ref_norms2(real), MC.ref_norms2(fake)
        assert (np.abs(g["r_real"].cpu().numpy() - p["r_real"]) <= MC.dist_ceiling(nr, nr, F)).all()
        assert (np.abs(g["r_fake"].cpu().numpy() - p["r_fake"]) <= MC.dist_ceiling(nf, nf, F)).all()
        assert (np.abs(g["min_r"].cpu().numpy() - p["min_r"]) <= MC.dist_ceiling(nr, nf, F)).all()
        if MC.min_decision_gap(p) >= MC.MIN_DECISION_GAP:
            assert (g["count_f"].cpu().numpy() == p["count_f"]).all() and (g["count_r"].cpu().numpy() == p["count_r"]).all()


# ------------------------------------------------------------------------------------------- counts and decisions
@pytest.mark.parametrize("case", MC.CASES, ids=str)
def test_counts_and_prdc_are_exact(case):
    from uspace_amd.tools.feature_metrics import FeatureBank, prdc
    real, fake = MC.sets_of(case)
    p, g, k = MC.parts_of(case), _gpu_of(case), case[4]
    assert g["count_f"].dtype == torch.int32 and g["count_r"].dtype == torch.int32
    count_f, count_r = g["count_f"].cpu().numpy(), g["count_r"].cpu().numpy()
    assert (count_f == p["count_f"]).all() and (count_r == p["count_r"]).all()
    assert ((count_f > 0) == (p["count_f"] > 0)).all() and ((count_r > 0) == (p["count_r"] > 0)).all()
    covered = (g["min_r"] <= g["r_real"]).cpu().numpy()
    assert (covered == (p["min_r"] <= p["r_real"])).all()
    want = MC.prdc_from_parts(p, k)
    got = prdc(_dev(real), _dev(fake), nearest_k=k)
    assert all(type(v) is float for v in got.values())
    assert got == want, (got, want)
    assert prdc(FeatureBank.from_features(_dev(real)), FeatureBank.from_features(_dev(fake)), nearest_k=k) == want


# ------------------------------------------------------------------------------------------- KID
@pytest.mark.parametrize("degree", (1, 3))
@pytest.mark.parametrize("m", (50, 17))
@pytest.mark.parametrize("case", MC.KID_CASES, ids=str)
def test_kid(case, m, degree):
    from uspace_amd import _hip
    from uspace_amd.tools.feature_metrics import draw_subsets, kid_score
    real, fake = MC.sets_of(case)
    ref = MC.ref_kid(fake, real, 7, m, degree=degree)
    x, y = _dev(fake), _dev(real)
    idx_f, idx_r = draw_subsets(len(fake), len(real), 7, m, 2020)
    assert (idx_f == ref["idx"][0]).all() and (idx_r == ref["idx"][1]).all()
    sums = _hip.metric_poly_sums(x, y, _dev(idx_f), _dev(idx_r), degree, 1.0 / case[3], 1.0)
    err = np.abs(sums.cpu().numpy() - ref["sums"])
    print(f"{case} m={m} degree={degree}: worst |sum - ref| / bound {float((err / ref['sum_bound']).max()):.3e}")
    assert (err <= ref["sum_bound"]).all()
    mean, std = kid_score(x, y, subsets=7, subset_size=m, degree=degree)
    print(f"  mean {mean!r} (ref {ref['mean']!r}, bound {ref['mean_bound']:.2e}), std {std!r} (ref {ref['std']!r}, bound {ref['std_bound']:.2e})")
    assert abs(mean - ref["mean"]) <= ref["mean_bound"] and abs(std - ref["std"]) <= ref["std_bound"]
    assert kid_score(x, y, subsets=7, subset_size=m, degree=degree) == (mean, std)             # the same seed: the same bits
    assert _same_bits(sums, _hip.metric_poly_sums(x, y, _dev(idx_f), _dev(idx_r), degree, 1.0 / case[3], 1.0))
    assert kid_score(x, y, subsets=7, subset_size=m, degree=degree, seed=1)[0] != mean         # another draw


# ------------------------------------------------------------------------------------------- structure
@pytest.mark.parametrize("case", [MC.CASES[0], MC.CASES[3]], ids=str)
def test_bit_equal_run_to_run_and_on_a_poisoned_workspace(case):
    """Every output twice, and once more on workspaces filled with 0xFF bytes (NaN as fp64): nothing read may be uninitialised."""
    from uspace_amd import _hip
    real, fake = MC.sets_of(case)
    x, y = _dev(real), _dev(fake)
    first, again, poisoned = _gpu_of(case), _run(x, y, case[4]), _run(x, y, case[4], ws_fill=0xFF)
    for name in first:
        assert _same_bits(first[name], again[name]), name
        assert _same_bits(first[name], poisoned[name]), name
    from uspace_amd.tools.feature_metrics import draw_subsets
    idx = [_dev(a) for a in draw_subsets(len(fake), len(real), 3, 17, 5)]
    sums = _hip.metric_poly_sums(y, x, idx[0], idx[1], 3, 1.0 / case[3], 1.0)
    ws = _hip.metric_workspace(len(fake), len(real), 3, 17, device=x.device, fill=0xFF)
    assert torch.isnan(ws.view(torch.float64)).all()
    assert _same_bits(sums, _hip.metric_poly_sums(y, x, idx[0], idx[1], 3, 1.0 / case[3], 1.0, ws=ws))
    assert torch.isfinite(sums).all()


def test_radius_is_independent_of_the_other_rows_order_and_of_far_rows():
    from uspace_amd import _hip
    case = MC.CASES[0]
    real, _ = MC.sets_of(case)
    base = _gpu_of(case)["r_real"]
    perm = np.random.default_rng(3).permutation(len(real))
    got = _hip.metric_knn_radius2(_dev(real[perm]), case[4])
    assert _same_bits(got, base[torch.from_numpy(perm).cuda()])                   # row perm[i] of the original sits at i
    far = np.concatenate([real, real[:64] + np.float32(1000.0)])
    got = _hip.metric_knn_radius2(_dev(far), case[4])
    assert _same_bits(got[:len(real)], base)


def test_manifold_of_a_row_alone_equals_the_row_in_the_set():
    from uspace_amd import _hip
    case = MC.CASES[0]
    real, fake = MC.sets_of(case)
    g = _gpu_of(case)
    x, y = _dev(real), _dev(fake)
    for i in (0, 70, len(real) - 1):
        count, mn = _hip.metric_manifold(x[i:i + 1].contiguous(), y, g["r_fake"])
        assert _same_bits(count, g["count_r"][i:i + 1]) and _same_bits(mn, g["min_r"][i:i + 1])
    count, mn = _hip.metric_manifold(x, y, None, want_count=False)                # min_d2 alone needs no radii
    assert count is None and _same_bits(mn, g["min_r"])


def test_identical_sets_give_ones():
    from uspace_amd.tools.feature_metrics import prdc
    a = _dev(MC.sets_of(MC.CASES[2])[0])
    r = prdc(a, a.clone(), nearest_k=5)
    assert r["precision"] == 1.0 and r["recall"] == 1.0 and r["coverage"] == 1.0 and r["density"] > 0


def test_argument_errors():
    from uspace_amd import _hip
    x = _dev(MC.sets_of(MC.CASES[4])[0])                                           # 17 rows
    L = _hip.lib()
    ws = _hip.metric_workspace(17, 17, 2, 5, device=x.device)
    r2 = torch.zeros(17, dtype=torch.float64, device=x.device)
    idx = torch.zeros(2, 5, dtype=torch.int32, device=x.device)
    sums = torch.zeros(2, 3, dtype=torch.float64, device=x.device)
    P, S = _hip.ptr, _hip.stream_ptr()
    assert L.uspace_metric_knn_radius2(P(x), 17, 64, 17, P(r2), P(ws), ws.numel(), S) == -1            # k > n - 1 (and 17 > 16)
    assert L.uspace_metric_knn_radius2(P(x[:10]), 10, 64, 10, P(r2), P(ws), ws.numel(), S) == -1       # k > n - 1
    assert L.uspace_metric_manifold(P(x), 17, P(x), 17, 64, P(r2), None, None, P(ws), ws.numel(), S) == -1
    assert L.uspace_metric_poly_sums(P(x), 17, P(x), 17, 64, P(idx), P(idx), 2, 5, 0, 1.0, 1.0, P(sums), P(ws), ws.numel(), S) == -1
    with pytest.raises(_hip.UspaceHipError):
        _hip.metric_knn_radius2(x, 17)
    with pytest.raises(_hip.UspaceHipError):
        _hip.metric_knn_radius2(x[:10].contiguous(), 10)
    with pytest.raises(_hip.UspaceHipError):
        _hip.metric_manifold(x, x, r2, want_count=False, want_min=False)
    with pytest.raises(_hip.UspaceHipError):
        _hip.metric_poly_sums(x, x, idx, idx, 0, 1.0, 1.0)
    with pytest.raises(_hip.UspaceHipError):
        _hip.metric_knn_radius2(x.cpu(), 3)
    assert _hip.metric_knn_radius2(x, 16).shape == (17,)                           # the largest k the set allows still runs


# ------------------------------------------------------------------------------------------- end to end
def test_end_to_end_from_images(tmp_path):
    """9 real and 9 generated random 64^2 images through a seeded Inception-v3: the bank's features are model.features of the
    quantised images, banks and raw tensors give the same numbers, and so do the same images written as PNGs."""
    from PIL import Image
    from uspace_amd.tools.feature_metrics import FeatureBank, calculate_kid_given_paths, calculate_prdc_given_paths, kid_score, prdc
    from uspace_amd.tools.inception import InceptionV3
    model = InceptionV3([3], seed=0).cuda()
    g = torch.Generator().manual_seed(5)
    imgs = {"real": torch.rand(9, 3, 64, 64, generator=g), "fake": torch.rand(9, 3, 64, 64, generator=g)}
    banks, feats = {}, {}
    for name, x in imgs.items():
        bank = FeatureBank(2048, device="cuda", model=model)
        bank.update(x)
        q = x.cuda().mul(255).add(0.5).clamp(0, 255).to(torch.uint8)
        feats[name] = model.features(q.float() / 255, 3)
        assert len(bank) == 9 and _same_bits(bank.features.view(torch.int32), feats[name].view(torch.int32))
        banks[name] = bank
        os.makedirs(tmp_path / name)
        for i, a in enumerate(q.permute(0, 2, 3, 1).cpu().numpy()):
            Image.fromarray(a).save(str(tmp_path / name / f"{i}.png"))
    got = prdc(banks["real"], banks["fake"], nearest_k=3)
    assert got == prdc(feats["real"], feats["fake"], nearest_k=3)
    kid = kid_score(banks["fake"], banks["real"], subsets=4, subset_size=6)
    assert kid == kid_score(feats["fake"], feats["real"], subsets=4, subset_size=6) and np.isfinite(kid).all()
    paths = (str(tmp_path / "real"), str(tmp_path / "fake"))
    # one batch of 9, as above (9 files: the folder's sorted order is the numeric one)
    folder = calculate_prdc_given_paths(paths, nearest_k=3, device="cuda", batch_size=9, num_workers=0, model=model)
    banks["fake"].save(str(tmp_path / "fake.npz"))
    mixed = calculate_prdc_given_paths((paths[0], str(tmp_path / "fake.npz")), nearest_k=3, device="cuda", batch_size=9,
                                       num_workers=0, model=model)
    print(f"prdc in memory {got}, from folders {folder}, folder + bank file {mixed}; kid {kid}")
    assert folder == got and mixed == got
    assert calculate_kid_given_paths(paths, device="cuda", batch_size=9, num_workers=0, model=model, subsets=4, subset_size=6) == kid
