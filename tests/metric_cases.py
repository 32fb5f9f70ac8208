"""Shared by tests/test_metric_cases.py (CPU) and tests/test_gpu_metrics.py (GPU); a helper, not a test: the inputs, the
float64 numpy references, the planted faults and the bounds of the feature-set metrics (uspace_amd/tools/feature_metrics.py).

Bounds (derived, not fitted; u = 2^-53):
  distances   |got - ref| <= 8 F u (|x|^2 + |y|^2) of the pair that attains the value (the tests use the largest such pair of the
              row).  The products of fp32 values are exact in fp64; a sum of F terms in any order errs by at most
              F u sum|x_i y_i| <= F u (|x|^2 + |y|^2) / 2, the norms likewise; the factor 8 covers the three terms with room for
              the MFMA's unspecified internal order.
              Measured on one MI355X over CASES, worst ratio to this ceiling: radius2 8.3e-3, min_d2 6.8e-3 (both in case 0;
              1.2e-3 to 1.6e-3 at F = 2048; tests/test_gpu_metrics.py::test_distances prints them).
  counts, booleans, the four PRDC numbers: exact equality.  What allows it: no case has a decision d^2 <= r^2 with a relative gap
              below 1e-6 (test_metric_cases.py::test_no_near_ties), four orders of magnitude above the distance ceiling.
  KID sums    |got - ref| <= 64 F u sum (|gamma| sum_i |a_i b_i| + |coef0|)^degree, the absolute-value majorant of the same sum
              (the dot product errs by F u sum|a_i b_i|, the power multiplies a relative error by `degree` <= 8, the summation of
              m^2 terms adds its own; 64 covers them with room).  Measured worst ratio on one MI355X: 5.2e-4 (case 0, m = 17,
              degree 3; test_kid prints them).
  KID mean, std: the per-subset MMD^2 bound is Bxx / (m (m - 1)) + Byy / (m (m - 1)) + 2 Bxy / m^2; the mean moves by at most the mean
              of these, the standard deviation by at most their maximum (|std(a) - std(b)| <= |a - b|_2 / sqrt(n) <= max|a_i - b_i|).
"""
import functools

import numpy as np

U = 2.0 ** -53
DIST_FACTOR = 8.0
KID_FACTOR = 64.0
MIN_DECISION_GAP = 1e-6

# (seed, n_real, n_fake, F, k): several row and column tiles, ragged tails in both directions, every dims of the Inception
# blocks, k = 1 and k = 16
CASES = [
    (0, 300, 257, 64, 3),
    (1, 300, 257, 2048, 5),
    (2, 129, 64, 192, 1),
    (3, 65, 130, 768, 5),
    (4, 17, 17, 64, 16),
    (6, 64, 64, 64, 5),
    (7, 200, 131, 2048, 3),
]
KID_CASES = [CASES[0], CASES[1], CASES[3]]

PRDC_FAULTS = ("self_in_radius", "radius_of_wrong_set", "rows_columns_swapped", "density_over_n_real")
KID_FAULTS = ("diagonal_included", "gamma_one", "idx_y_for_x")


def make_sets(seed, n_real, n_fake, F):
    """Clusters in a 6-dimensional subspace; the fake set misses two clusters and a fifth of it is shifted off the manifold; the
    common offset of 1 makes |x|^2 >> d^2, which stresses the cancellation in D2."""
    rng = np.random.default_rng(seed)
    basis = rng.standard_normal((6, F)) / np.sqrt(6.0)
    centers = 3.0 * rng.standard_normal((8, 6))

    def draw(n, which, spread):
        c = rng.choice(which, n)
        lat = centers[c] + spread * rng.standard_normal((n, 6))
        return (lat @ basis + 0.05 * rng.standard_normal((n, F)) + 1.0).astype(np.float32)

    real = draw(n_real, np.arange(0, 8), 1.0)
    fake = draw(n_fake, np.arange(2, 8), 0.6)
    fake[: n_fake // 5] += (2.0 * rng.standard_normal((1, 6)) @ basis).astype(np.float32)
    return real, fake


@functools.lru_cache(maxsize=None)
def sets_of(case):
    real, fake = make_sets(*case[:4])
    real.setflags(write=False)
    fake.setflags(write=False)
    return real, fake


# ------------------------------------------------------------------------------------------ float64 references
def ref_d2(x, y):
    """[nx, ny] float64: ((a - b)^2).sum() from the fp32 values."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    out = np.empty((len(x), len(y)))
    for i in range(len(x)):
        out[i] = ((x[i][None, :] - y) ** 2).sum(1)
    return out


def ref_norms2(x):
    return (np.asarray(x, np.float64) ** 2).sum(1)


def ref_radius2(d_self, k, include_self=False):
    """k-th smallest of every row of a set's own distance matrix, self excluded by index."""
    d = np.array(d_self)
    if not include_self:
        d[np.arange(len(d)), np.arange(len(d))] = np.inf
    return np.sort(d, axis=1)[:, k - 1]


def ref_parts(real, fake, k, fault=None):
    """Everything the PRDC numbers are made of: distance matrices, radii, counts, nearest distances."""
    d_rr, d_ff, d_fr = ref_d2(real, real), ref_d2(fake, fake), ref_d2(fake, real)      # d_fr[j, i] = D2(fake_j, real_i)
    r_real = ref_radius2(d_rr, k, include_self=fault == "self_in_radius")
    r_fake = ref_radius2(d_ff, k, include_self=fault == "self_in_radius")
    if fault == "radius_of_wrong_set":          # the radius of the row's own point instead of the column's
        count_f = (d_fr <= r_fake[:, None]).sum(1)
        count_r = (d_fr.T <= r_real[:, None]).sum(1)
    elif fault == "rows_columns_swapped":       # counted along the other axis
        count_f = (d_fr <= r_real[None, :]).sum(0)
        count_r = (d_fr.T <= r_fake[None, :]).sum(0)
    else:
        count_f = (d_fr <= r_real[None, :]).sum(1)        # per generated sample: the real balls it falls into
        count_r = (d_fr.T <= r_fake[None, :]).sum(1)      # per real sample: the generated balls it falls into
    return dict(d_rr=d_rr, d_ff=d_ff, d_fr=d_fr, r_real=r_real, r_fake=r_fake, count_f=count_f.astype(np.int64),
                count_r=count_r.astype(np.int64), min_r=d_fr.min(0))


def prdc_from_parts(p, k, fault=None):
    n_fake, n_real = p["d_fr"].shape
    covered = p["min_r"] <= p["r_real"]
    return dict(precision=int((p["count_f"] > 0).sum()) / n_fake, recall=int((p["count_r"] > 0).sum()) / n_real,
                density=int(p["count_f"].sum()) / (k * (n_real if fault == "density_over_n_real" else n_fake)),
                coverage=int(covered.sum()) / n_real)


def ref_prdc(real, fake, k, fault=None):
    return prdc_from_parts(ref_parts(real, fake, k, fault), k, fault)


@functools.lru_cache(maxsize=None)
def parts_of(case):
    real, fake = sets_of(case)
    return ref_parts(real, fake, case[4])


def min_decision_gap(p):
    """The smallest relative gap |d^2 - r^2| / r^2 of any membership or coverage decision."""
    g1 = np.abs(p["d_fr"] - p["r_real"][None, :]) / p["r_real"][None, :]
    g2 = np.abs(p["d_fr"].T - p["r_fake"][None, :]) / p["r_fake"][None, :]
    g3 = np.abs(p["min_r"] - p["r_real"]) / p["r_real"]
    return float(min(g1.min(), g2.min(), g3.min()))


def dist_ceiling(nx2, ny2, F):
    """Per-row ceiling of a distance of a row with squared norm nx2 (array) against a set with squared norms ny2: the largest
    pair of the row."""
    return DIST_FACTOR * F * U * (np.asarray(nx2) + np.max(ny2))


# ------------------------------------------------------------------------------------------ KID
def draw_subsets_ref(n_fake, n_real, subsets, m, seed):
    rng = np.random.RandomState(seed)
    idx_f, idx_r = [], []
    for _ in range(subsets):
        idx_f.append(rng.choice(n_fake, m, replace=False))
        idx_r.append(rng.choice(n_real, m, replace=False))
    return np.array(idx_f, np.int32), np.array(idx_r, np.int32)


def ref_poly_sums(x, y, idx_x, idx_y, degree, gamma, coef0, fault=None):
    """(sums, majorant), float64 [n_subsets, 3]: (Sxx without p == q, Syy without p == q, Sxy) and the same sums of
    (|gamma| sum_i |a_i b_i| + |coef0|)^degree."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    if fault == "gamma_one":
        gamma = 1.0
    sums, major = np.zeros((len(idx_x), 3)), np.zeros((len(idx_x), 3))
    for s in range(len(idx_x)):
        a = x[idx_y[s] % len(x) if fault == "idx_y_for_x" else idx_x[s]]       # (the modulus keeps the planted fault in bounds)
        b = y[idx_y[s]]
        for w, (p, q, off) in enumerate(((a, a, True), (b, b, True), (a, b, False))):
            kmat = (gamma * (p @ q.T) + coef0) ** degree
            mmat = (abs(gamma) * (np.abs(p) @ np.abs(q).T) + abs(coef0)) ** degree
            if off and fault != "diagonal_included":
                np.fill_diagonal(kmat, 0.0)
                np.fill_diagonal(mmat, 0.0)
            sums[s, w], major[s, w] = kmat.sum(), mmat.sum()
    return sums, major


def mmd2(sums, m):
    return sums[:, 0] / (m * (m - 1)) + sums[:, 1] / (m * (m - 1)) - 2 * sums[:, 2] / (m * m)


def ref_kid(fake, real, subsets, m, degree=3, gamma=None, coef0=1.0, seed=2020, fault=None):
    """dict(mean, std, sums, sum_bound, mean_bound, std_bound) of the float64 reference."""
    F = fake.shape[1]
    g = 1.0 / F if gamma is None else gamma
    idx_f, idx_r = draw_subsets_ref(len(fake), len(real), subsets, m, seed)
    sums, major = ref_poly_sums(fake, real, idx_f, idx_r, degree, g, coef0, fault)
    sum_bound = KID_FACTOR * F * U * major
    v = mmd2(sums, m)
    vb = mmd2(np.stack([sum_bound[:, 0], sum_bound[:, 1], -sum_bound[:, 2]], 1), m)
    return dict(mean=float(np.mean(v)), std=float(np.std(v)), sums=sums, sum_bound=sum_bound, mean_bound=float(np.mean(vb)),
                std_bound=float(np.max(vb)), idx=(idx_f, idx_r))


# ------------------------------------------------------------------------------------------ the six points in the plane
HAND_REAL = np.array([[0, 0], [3, 0], [0, 4]], np.float32)
HAND_FAKE = np.array([[1, 0], [3, 1], [10, 10]], np.float32)
