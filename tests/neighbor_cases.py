"""Shared by tests/test_neighbor_cases.py (CPU) and tests/test_gpu_neighbors.py (GPU); a helper, not a test: the inputs, the
float64 numpy references, the planted faults and the bounds of the memorisation checks (uspace_amd/tools/neighbors.py,
uspace_metric_topk).  The sets are those of tests/metric_cases.py.

Bounds (derived, not fitted; u = 2^-53):
  refined distances  |got - ref| <= 4 F u ref.  The differences x_f - y_f of fp32 values are exact in fp64 (or err by u relative where
              the exponents are far apart, which the factor covers); F squares and F additions in any order err by at most
              (F + 1) u sum, so 4 F u has room for both.  An exact copy reports == 0.0.
  indices, authenticity booleans and percentage: exact equality.  What allows it is a condition on the inputs, asserted here
              (``check_gaps``, ``ref_authenticity``), not a measurement: every gap between consecutive neighbours among a row's first
              k + 1 is at least 1000 x that row's ``dist_ceiling`` (the Gram selection's error), or exactly 0 between bit-equal
              rows; every authenticity decision has a relative gap of at least 1e-4.
  Z_U         the host fp64 arithmetic on identical ranks: 1e-12 relative (``check_rank_gaps`` asserts that no two distances that
              are not bit-equal lie within 1e-9 relative of each other, a thousand times the refined distances' error).
"""
import functools

import numpy as np

from tests import metric_cases as MC

U = MC.U
REFINE_FACTOR = 4.0
MIN_GAP_CEILINGS = 1000.0
MIN_AUTH_GAP = 1e-4
MIN_RANK_GAP = 1e-9
Z_RTOL = 1e-12
K_MAX = 16

TOPK_FAULTS = ("self_included", "ties_by_arrival", "index_base_dropped", "kth_is_k_plus_1", "rows_columns_swapped", "unrefined")
FAULTS = TOPK_FAULTS + ("auth_radius_of_query", "u_without_ties")


def ks_of(case):
    return sorted({1, case[4], K_MAX})


# ------------------------------------------------------------------------------------------ float64 references
def arrival_key(j):
    """The position at which the kernel's insertion path meets column j: the 128-column tile, then the lane's turn (j % 16), then
    the lane's walk over its eight columns."""
    j = np.asarray(j)
    return (j // 128) * 128 + (j % 16) * 8 + (j % 128) // 16


def gram_d2(x, y):
    """|x|^2 + |y|^2 - 2 x.y in float64, the norms and the dot product summed in different orders (pairwise against sequential):
    what a kernel reports that skips the refinement.  An exact copy comes out near 1e-13, not 0."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    dot = np.array([[np.cumsum(a * b)[-1] for b in y] for a in x])
    return np.maximum(0.0, (x ** 2).sum(1)[:, None] + (y ** 2).sum(1)[None, :] - 2.0 * dot)


def ref_topk(x, y, k, index_base=0, self_base=-1, fault=None, d=None):
    """(d2 float64 [nx, k], idx int64 [nx, k]): the k smallest of every row of ref_d2(x, y) in the order (d2, index), the index
    index_base + j, without the column index_base + j == self_base + i; short rows end in (+inf, -1)."""
    d = np.array(MC.ref_d2(x, y) if d is None else d)
    if fault == "unrefined":
        d = gram_d2(x, y)
    if fault == "rows_columns_swapped":
        d = d.T.copy()
    nx, ny = d.shape
    eligible = np.ones((nx, ny), bool)
    if self_base >= 0 and fault != "self_included":
        j = self_base + np.arange(nx) - index_base
        ok = (j >= 0) & (j < ny)
        eligible[np.arange(nx)[ok], j[ok]] = False
    d2 = np.full((nx, k), np.inf)
    idx = np.full((nx, k), -1, np.int64)
    cols = np.arange(ny)
    second = arrival_key(cols) if fault == "ties_by_arrival" else cols
    skip = 1 if fault == "kth_is_k_plus_1" else 0
    for i in range(nx):
        c = cols[eligible[i]]
        order = c[np.lexsort((second[c], d[i, c]))][skip:skip + k]
        d2[i, :len(order)] = d[i, order]
        idx[i, :len(order)] = order + (0 if fault == "index_base_dropped" else index_base)
    return d2, idx


def gap_ceilings(x, y, k, self_base=-1, index_base=0):
    """The smallest gap between consecutive neighbours among every row's first k + 1, in units of the row's dist_ceiling, over the
    gaps that are not exactly 0 (bit-equal rows of y)."""
    d2, _ = ref_topk(x, y, min(k + 1, len(y)), index_base, self_base)
    ceil = MC.dist_ceiling(MC.ref_norms2(x), MC.ref_norms2(y), x.shape[1])
    with np.errstate(invalid="ignore"):
        gaps = np.diff(d2, axis=1) / ceil[:, None]
    gaps = gaps[np.isfinite(gaps) & (gaps != 0.0)]
    return float(gaps.min()) if gaps.size else np.inf


def check_gaps(x, y, k, self_base=-1, index_base=0):
    g = gap_ceilings(x, y, k, self_base, index_base)
    assert g >= MIN_GAP_CEILINGS, f"neighbour gap of {g:.3e} selection ceilings: the indices are not decided"
    return g


def refined_bound(ref, F):
    return REFINE_FACTOR * F * U * ref


def ref_authenticity(fake, train, fault=None):
    """dict(authentic bool [n_fake], pct, d2, idx, train_d2, gap): gap is the smallest relative |d2 - r| / r of a decision."""
    d2, idx = ref_topk(fake, train, 1)
    d2, idx = d2[:, 0], idx[:, 0]
    train_d2 = ref_topk(train, train, 1, self_base=0)[0][:, 0]
    radius = train_d2[idx]
    if fault == "auth_radius_of_query":
        radius = ref_topk(fake, fake, 1, self_base=0)[0][:, 0]
    authentic = d2 > radius
    return dict(authentic=authentic, pct=100.0 * int(authentic.sum()) / len(fake), d2=d2, idx=idx, train_d2=train_d2,
                gap=float((np.abs(d2 - radius) / radius).min()))


def ref_u(l_fake, l_test, fault=None):
    """The Mann-Whitney U of L(fake) against L(test), counted pair by pair: L(fake) > L(test) counts 1, a tie one half."""
    a, b = np.asarray(l_fake, np.float64)[:, None], np.asarray(l_test, np.float64)[None, :]
    return float((a > b).sum() + (0.0 if fault == "u_without_ties" else 0.5 * (a == b).sum()))


def ref_zu(l_fake, l_test, fault=None):
    m, n = len(l_fake), len(l_test)
    return (ref_u(l_fake, l_test, fault) - m * n / 2.0) / np.sqrt(m * n * (m + n + 1) / 12.0)


def ref_zu_cells(l_fake, l_test, cells, min_cell, fault=None):
    cf, cs, ct = cells
    z, w = [], []
    for c in np.unique(ct):
        if (cf == c).sum() >= min_cell and (cs == c).sum() >= min_cell:
            z.append(ref_zu(l_fake[cf == c], l_test[cs == c], fault))
            w.append(float((ct == c).sum()))
    assert z, "no cell kept"
    return float(np.dot(z, w) / np.sum(w))


def check_rank_gaps(l_fake, l_test):
    v = np.sort(np.concatenate([l_fake, l_test]))
    rel = np.diff(v) / v[1:]
    rel = rel[rel != 0.0]
    assert rel.size == 0 or rel.min() >= MIN_RANK_GAP, f"two distances {rel.min():.3e} apart: the ranks are not decided"


# ------------------------------------------------------------------------------------------ the three sets of the copying test
MIN_CELL = 10


@functools.lru_cache(maxsize=None)
def copying_sets(case):
    """(fake, test, train, cells): the real set of the case split into train (the first two thirds) and test; four generated rows
    are exact copies of test rows, so L has ties between the two samples.  Cells: the first feature against the training set's
    median and its 97th percentile -- two large cells and a small one that min_cell = 10 drops."""
    real, fake = MC.sets_of(case)
    n_train = 2 * len(real) // 3
    train, test = real[:n_train], real[n_train:]
    fake = np.array(fake)
    fake[:4] = test[:4]
    lo, hi = np.quantile(train[:, 0], [0.5, 0.97])
    cells = tuple(((s[:, 0] > lo).astype(np.int64) + (s[:, 0] > hi)) for s in (fake, test, train))
    for a in (fake, test, train):
        a.setflags(write=False)
    return fake, test, train, cells


# ------------------------------------------------------------------------------------------ edge cases
DUP_COLUMNS = ((5, 130, 300), (129, 144, 240))


@functools.lru_cache(maxsize=None)
def duplicate_bank():
    """(queries [24, 64], bank [301, 64]): the bank holds two groups of three bit-equal rows.  Columns 5, 130, 300 lie in three
    different column tiles; 129, 144, 240 lie in one, where the insertion path meets them as 144, 240, 129.  The first twelve
    queries sit next to one of the duplicated rows, so the group leads their neighbour lists."""
    real, fake = MC.make_sets(21, 301, 24, 64)
    bank, q = np.array(real), np.array(fake)
    for group in DUP_COLUMNS:
        for c in group[1:]:
            bank[c] = bank[group[0]]
    rng = np.random.default_rng(5)
    for i in range(12):
        q[i] = bank[DUP_COLUMNS[i % 2][0]] + (0.01 * rng.standard_normal(64)).astype(np.float32)
    bank.setflags(write=False)
    q.setflags(write=False)
    return q, bank


@functools.lru_cache(maxsize=None)
def edge_cases():
    """{name: (x, y, k, index_base, self_base)}"""
    out = {}
    a, b = MC.make_sets(31, 40, 33, 64)
    out["ny_below_k"] = (b[:5], a[:3], 5, 0, -1)
    out["ny_1"] = (b, a[:1], 2, 0, -1)
    out["nx_1"] = (b[:1], a, 3, 0, -1)
    a1, b1 = MC.make_sets(32, 30, 20, 1)
    out["F_1"] = (b1, a1, 3, 0, -1)
    a3, b3 = MC.make_sets(12, 40, 33, 3)
    out["F_3"] = (b3, a3, 2, 0, -1)
    a66, b66 = MC.make_sets(33, 40, 33, 66)
    out["F_66"] = (b66, a66, 4, 7, -1)
    real = MC.sets_of(MC.CASES[0])[0]
    out["self_on_a_shard"] = (real[128:200], real[100:300], 3, 100, 128)          # row i of x is column 28 + i of y
    out["self_whole_set"] = (real, real, 16, 0, 0)
    for v in out.values():
        for t in v[:2]:
            t.setflags(write=False)
    return out


def exact_copy_case():
    """(queries, bank, copies): query i is bit-equal to bank row copies[i] for the first len(copies) queries."""
    real, fake = MC.sets_of(MC.CASES[0])
    q = np.array(fake[:70])
    copies = (0, 127, 128, 299, 64)
    for i, j in enumerate(copies):
        q[i] = real[j]
    return q, real, copies


# ------------------------------------------------------------------------------------------ the points in the plane
# train T0 (0,0)  T1 (4,0)  T2 (0,10)  T3 (10,10);  nearest other training sample, squared: T0 16 (T1), T1 16 (T0), T2 100 (T0 or T3:
# index 0 wins), T3 100 (T2)
HAND_TRAIN = np.array([[0, 0], [4, 0], [0, 10], [10, 10]], np.float32)
# generated G0 (1,0): nearest T0 at 1 <= 16, a copy-like sample;  G1 (4,5): T1 at 25 > 16, authentic;  G2 (0,10): T2 at 0, an exact
# copy;  G3 (10,21): T3 at 121 > 100, authentic;  G4 (2,0): T0 and T1 both at 4, index 0 wins, not authentic
HAND_FAKE = np.array([[1, 0], [4, 5], [0, 10], [10, 21], [2, 0]], np.float32)
# held-out real H0 (0,2): T0 at 4;  H1 (7,0): T1 at 9;  H2 (10,5): T3 at 25
HAND_TEST = np.array([[0, 2], [7, 0], [10, 5]], np.float32)
HAND_L_FAKE, HAND_L_TEST = [1.0, 25.0, 0.0, 121.0, 4.0], [4.0, 9.0, 25.0]
# pairs L(fake) > L(test): G1 over H0, H1 (2) and tied with H2 (1/2); G3 over all three (3); G4 tied with H0 (1/2) -> U = 6
HAND_U = 6.0
