"""CPU-only checks of tests/eval_suite_cases.py: the float64 references against hand-computed values, the case lists, and the
proof that every bound of tests/test_gpu_eval_suite.py separates every planted fault.

Smallest effect of each fault over the cases that can show it, as the float64 references give it with these seeds (printed by
the tests; what is asserted is the margin the bounds need, 1000 x, not these figures): global marginal 0.21 relative on the mean,
classes truncated to 1000 2.0e-4, KL direction swapped 0.99, mean of exp 4.4e-3, ceil-sized splits 3.2e-4 on the mean and 1.1e-3
on the std, ddof = 1 3.6e-3 on the std, a dropped bias of std 0.5 4.9e-3; spatial faults 0.71 (stage 15), 1.2 (last channels,
(c, h, w) order)."""
import numpy as np
import pytest

from tests import eval_suite_cases as EC


def test_bounds_are_the_projects_own():
    from tests.test_gpu_inception import TOL
    for k, v in EC.TOL.items():
        assert TOL[k] == v, k


def test_hand_made_inception_score():
    """Two classes, four rows, two splits.  Rows 0-1: p = (1/2, 1/2) and (1/2, 1/2): every KL is 0, score 1.
    Rows 2-3: p = (0.8, 0.2) and (0.2, 0.8), pbar = (1/2, 1/2): KL = 0.8 log 1.6 + 0.2 log 0.4 for both, score = exp(KL)."""
    l8, l2 = np.log(0.8), np.log(0.2)
    x = np.array([[0.0, 0.0], [3.0, 3.0], [l8, l2], [l2 + 5, l8 + 5]])
    s = EC.ref_split_scores(x, 2)
    kl = 0.8 * np.log(1.6) + 0.2 * np.log(0.4)
    assert s[0] == pytest.approx(1.0, abs=1e-15) and s[1] == pytest.approx(np.exp(kl), rel=1e-14)
    mean, std = EC.ref_inception_score(x, 2)
    assert mean == pytest.approx((1 + np.exp(kl)) / 2, rel=1e-14) and std == pytest.approx((np.exp(kl) - 1) / 2, rel=1e-13)
    # a one-hot row against a uniform marginal: KL = log C; p = 0 terms contribute nothing (and give no NaN)
    onehot = np.full((3, 3), -1e4)
    onehot[np.arange(3), np.arange(3)] = 0.0
    assert EC.ref_split_scores(onehot, 1)[0] == pytest.approx(3.0, rel=1e-14)


def test_split_rule():
    assert EC.split_bounds(10, 3) == [(0, 3), (3, 6), (6, 10)]
    assert EC.split_bounds(97, 10)[:3] == [(0, 9), (9, 19), (19, 29)] and EC.split_bounds(97, 10)[-1] == (87, 97)
    assert EC.split_bounds(10, 3, "ceil_splits") == [(0, 4), (4, 8), (8, 10)]
    for (N, _C, splits) in EC.IS_CASES:
        b = EC.split_bounds(N, splits)
        assert b[0][0] == 0 and b[-1][1] == N and all(b[i][1] == b[i + 1][0] for i in range(splits - 1))
        assert all(hi > lo for lo, hi in b)


def test_cases_are_non_trivial():
    """The scores are well above 1 wherever a split has several rows, and the splits differ; with one row per split every score
    is exactly 1 (a row is its own marginal)."""
    for case in EC.IS_CASES:
        s = EC.ref_split_scores(EC.logits_of(case), case[2])
        print(case, "scores", np.round(s, 4))
        if case[0] // case[2] > 1:
            assert s.min() > 2.0
            if case[2] > 1:
                assert np.std(s) / np.mean(s) > 1e-3
        else:
            assert np.abs(s - 1).max() < 1e-12
    x = EC.logits_of(EC.ZERO_CASE, True)
    assert 0.05 < (x == np.float32(-1e4)).mean() < 0.06 and (x[:, 3] == np.float32(-1e4)).all()
    s = EC.ref_split_scores(x, EC.ZERO_CASE[2])
    assert np.isfinite(s).all() and s.min() > 2.0
    p = EC.softmax64(x)
    assert (p[:, 3] == 0).all() and (p == 0).mean() > 0.05          # p = 0 and pbar = 0 really occur


def test_every_is_fault_exceeds_the_bound_1000_times():
    worst = {}
    for fault in EC.IS_FAULTS:
        exposed = [c for c in EC.IS_CASES if EC.fault_exposed_by(fault, c)]
        assert exposed, fault
        for case in exposed:
            x = EC.logits_of(case)
            d_mean, d_std = EC.is_deviation(EC.ref_inception_score(x, case[2]), EC.ref_inception_score(x, case[2], fault))
            worst[fault] = (min(worst.get(fault, (np.inf, np.inf))[0], d_mean), min(worst.get(fault, (np.inf, np.inf))[1], d_std))
            if fault == "ddof1":
                assert d_std > 1000 * EC.TOL["stats"], (fault, case, d_std)
            else:
                assert d_mean > 1000 * EC.TOL["stats"], (fault, case, d_mean)
            if fault == "ceil_splits":
                assert d_std > 1000 * EC.TOL["stats"], (fault, case, d_std)
    for fault, (m, s) in worst.items():
        print(f"{fault}: smallest change over its cases: mean {m:.3e}, std {s:.3e}")
    # the single-split case exposes only the split-independent faults
    single = EC.IS_CASES[2]
    assert [f for f in EC.IS_FAULTS if EC.fault_exposed_by(f, single)] == ["kl_swapped", "mean_of_exp", "dropped_bias"]


def test_every_logit_fault_exceeds_the_bound():
    for case in EC.LOGIT_CASES:
        pool, W, b = EC.logit_operands(case)
        ref = EC.ref_logits(pool, W, b)
        assert ref.shape == (case[0], case[2])
        if case[2] > 1:
            assert (ref < 0).any() and (ref > 0).any()
        for fault in EC.LOGIT_FAULTS:
            if fault == "relu" and not (ref < 0).any():
                continue
            if fault == "k_truncated" and case[1] == 16:
                continue
            d = EC.worst_row_rel_l2(EC.ref_logits(pool, W, b, fault), ref)
            assert d > 10 * EC.TOL["stage"], (case, fault, d)


@pytest.fixture(scope="module")
def restated_stages():
    """Stages 14 and 15 of the float64 restatement for one seeded image (computed once)."""
    import torch
    from tests import inception_stages as S
    from uspace_amd.tools.inception import InceptionV3
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    sd = {k: v.detach() for k, v in InceptionV3(seed=0).state_dict().items()}
    x = torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(2)).double()
    s14 = S.forward(sd, x, last=14)
    s15 = S.stage(sd, 15, s14)
    return s14.numpy(), s15.numpy()


def test_every_spatial_fault_exceeds_the_bound(restated_stages):
    s14, s15 = restated_stages
    assert s14.shape == (1, 768, 17, 17)
    ref = EC.ref_spatial(s14)
    assert ref.shape == (1, 2023)
    # (h, w, c) order: element (h, w, c) sits at (h * 17 + w) * 7 + c
    assert ref[0, (5 * 17 + 3) * 7 + 2] == s14[0, 2, 5, 3]
    bad = dict(stage_15=EC.ref_spatial(s15), last_channels=EC.ref_spatial(s14, fault="last_channels"),
               chw_order=EC.ref_spatial(s14, fault="chw_order"))
    assert sorted(bad) == sorted(EC.SPATIAL_FAULTS)
    for fault, v in bad.items():
        d = EC.rel_l2(v, ref)
        print(f"{fault}: rel-L2 {d:.3e}")
        assert d > 10 * EC.TOL["stage"], (fault, d)
    # the order fault is a permutation: it counts against the element-wise comparison only (sFID is permutation-invariant)
    assert np.array_equal(np.sort(bad["chw_order"].ravel()), np.sort(ref.ravel()))
