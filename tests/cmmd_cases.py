"""Shared by tests/test_cmmd_cases.py (CPU), tests/test_cmmd_host.py (CPU) and tests/test_gpu_cmmd.py (GPU); a helper, not a
test: the inputs, the float64 numpy reference, the planted faults and the bounds of the RBF-kernel MMD behind CMMD
(uspace_amd/tools/cmmd.py, uspace_metric_rbf_sums of uspace_amd/csrc/metrics.hip).

Definition (gamma = 1 / (2 sigma^2), K(a, b) = exp(-gamma D2(a, b)), D2 = ((a - b)^2).sum() in float64 from the fp32 values, between
a / |a| and b / |b| under ``normalize``; a zero row is the zero vector):
  Sxx = sum_{i != j} K(x_i, x_j), Syy likewise, Sxy = sum_{i, j} K(x_i, y_j); the diagonal is left out by index
  V = (Sxx + nx) / nx^2 + (Syy + ny) / ny^2 - 2 Sxy / (nx ny)            U = Sxx / (nx (nx - 1)) + Syy / (ny (ny - 1)) - 2 Sxy / (nx ny)
  score = scale * V (CMMD: sigma = 10, scale = 1000, normalised).

Bounds (derived, not fitted; u = 2^-53).  Per sum, N the number of pairs in it:
  |got - ref| <= 64 u sum_pairs (gamma F (|a|^2 + |b|^2) + 1) + (N - 1) u N
    D2 errs by at most 8 F u (|a|^2 + |b|^2), the distance bound of tests/metric_cases.py (|a|^2 = |b|^2 = 1 under normalisation,
    where the division by the norms adds a few u of a value <= 2); |dK / dD2| <= gamma because K <= 1; the product gamma D2 and the
    device exp add a few ulps of a value <= 1 (an argument error of |t| u moves exp(-t) by t exp(-t) u <= u / e); the factor 64 covers
    these with room, as KID_FACTOR does.  The last term is the worst-case bound of summing N values <= 1 in any order.
  A score: scale (Bxx / dx + Byy / dy + 2 Bxy / (nx ny)) with dx = nx^2 (V) or nx (nx - 1) (U), dy likewise.
  Measured on one MI355X over CASES x normalize (tests/test_gpu_cmmd.py::test_sums_and_scores prints them), worst ratio to the
  bound: sums 2.19e-2 (Sxy of case 4, normalised: five pairs; 8.0e-4 in case 3, <= 2.5e-4 in cases 0 - 2; 1.46e-3 without
  normalisation, case 4, <= 2.1e-5 elsewhere), V score 9.23e-3 (case 4; <= 1.9e-4 elsewhere), U score 1.83e-4 (case 3).  The device exp
  was not measured on its own: the sums stay that far inside a bound that grants it a few ulps.

The score is small against the sums: on these sets, normalised at sigma = 10, score = 0.37 .. 1.5 while every K >= 0.982, so
the planted faults are judged against 1000 x the score's bound (tests/test_cmmd_cases.py).
"""
import functools

import numpy as np

from tests.metric_cases import make_sets

U = 2.0 ** -53
RBF_FACTOR = 64.0
SIGMA = 10.0
SCALE = 1000.0
FAULT_MARGIN = 1000.0

# (seed, nx, ny, F): the smallest shapes that reach every path of the 64 x 128 x 32 tile engine
CASES = [
    (0, 129, 257, 48),       # three row blocks with a one-row tail, three column tiles with a one-column tail, a partial K step
    (1, 257, 129, 768),      # nx > ny, the embedding width
    (2, 64, 64, 64),         # exactly one block and half a tile
    (3, 17, 130, 67),        # the scalar-load path (F % 4 != 0), rows < 64
    (4, 1, 5, 8),            # a one-row set: Sxx = 0 exactly
]
NORMALIZE = (1, 0)
TILE_COLUMNS = 128

FAULTS = ("diagonal_in_offdiag_sums", "gamma_is_1_over_sigma2", "not_normalised", "xy_counted_once", "padding_columns_included",
          "v_statistic_without_diagonal")


def fault_applies(fault, case, normalize):
    """Whether the fault must show in the V-statistic score of this run.  ``not_normalised`` is a fault only where normalisation
    is asked for.  ``padding_columns_included`` adds pad * sum_i exp(-gamma |a_i|^2) to each sum: under normalisation that is
    pad * n * exp(-gamma), which cancels in the V-statistic exactly when nx == ny (case 2), so there the fault is judged on the
    three sums instead (``fault_moves_sums``); without normalisation its size is a property of the data's norms (e^-38 at
    F = 768, where it vanishes), not of the code, whose column guard is the same for both settings -- judged under
    normalisation only.  Every other fault applies to every run."""
    if fault == "not_normalised":
        return bool(normalize)
    if fault == "padding_columns_included":
        return bool(normalize) and case[1] != case[2]
    return True


def fault_moves_sums(fault, normalize):
    """Faults that must (also) show in each of the three sums of every case: see ``fault_applies``."""
    return fault == "padding_columns_included" and bool(normalize)


@functools.lru_cache(maxsize=None)
def sets_of(case):
    """(x, y) fp32, read-only: make_sets' (real, fake) of sizes (nx, ny)."""
    x, y = make_sets(*case)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


def unit_rows(a):
    a = np.asarray(a, np.float64)
    n = np.sqrt((a * a).sum(1, keepdims=True))
    return np.divide(a, n, out=np.zeros_like(a), where=n > 0)


def ref_kernel(a, b, gamma):
    """[na, nb] float64: exp(-gamma ((a_i - b_j)^2).sum())."""
    out = np.empty((len(a), len(b)))
    for i in range(len(a)):
        out[i] = ((a[i][None, :] - b) ** 2).sum(1)
    return np.exp(-gamma * out)


def ref_sums(x, y, sigma=SIGMA, normalize=True, fault=None):
    """(sums, bounds, kmin): float64 [3] (Sxx, Syy, Sxy), their bounds, and the smallest kernel value met."""
    F = np.shape(x)[1]
    gamma = 1.0 / (sigma * sigma) if fault == "gamma_is_1_over_sigma2" else 1.0 / (2.0 * sigma * sigma)
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    if normalize and fault != "not_normalised":
        x, y = unit_rows(x), unit_rows(y)
    nx2, ny2 = (x * x).sum(1), (y * y).sum(1)
    sums, bounds, kmin = np.zeros(3), np.zeros(3), 1.0
    for w, (a, b, na2, nb2, off) in enumerate(((x, x, nx2, nx2, True), (y, y, ny2, ny2, True), (x, y, nx2, ny2, False))):
        k = ref_kernel(a, b, gamma)
        kmin = min(kmin, float(k.min()))
        norms = na2[:, None] + nb2[None, :]
        if off and fault != "diagonal_in_offdiag_sums":
            np.fill_diagonal(k, 0.0)
            np.fill_diagonal(norms, 0.0)
        n_pairs = k.size - (len(a) if off else 0)
        sums[w] = k.sum()
        if fault == "padding_columns_included":          # zero rows up to the tile's width: D2 = |a|^2, K > 0
            pad = -len(b) % TILE_COLUMNS
            sums[w] += pad * np.exp(-gamma * na2).sum()
        bounds[w] = RBF_FACTOR * U * (gamma * F * norms.sum() + n_pairs) + max(n_pairs - 1, 0) * U * n_pairs
    return sums, bounds, kmin


def mmd2(sums, nx, ny, unbiased=False, fault=None):
    cross = (1.0 if fault == "xy_counted_once" else 2.0) * sums[2] / (nx * ny)
    if unbiased:
        return sums[0] / (nx * (nx - 1)) + sums[1] / (ny * (ny - 1)) - cross
    if fault == "v_statistic_without_diagonal":
        return sums[0] / (nx * nx) + sums[1] / (ny * ny) - cross
    return (sums[0] + nx) / (nx * nx) + (sums[1] + ny) / (ny * ny) - cross


def mmd2_bound(bounds, nx, ny, unbiased=False):
    dx, dy = (nx * (nx - 1), ny * (ny - 1)) if unbiased else (nx * nx, ny * ny)
    return bounds[0] / dx + bounds[1] / dy + 2.0 * bounds[2] / (nx * ny)


def ref_score(x, y, sigma=SIGMA, normalize=True, unbiased=False, scale=SCALE, fault=None):
    """dict(score, bound, sums, sum_bounds, kmin) of the float64 reference (take the bounds from the run without a fault)."""
    sums, bounds, kmin = ref_sums(x, y, sigma, normalize, fault)
    nx, ny = len(x), len(y)
    return dict(score=scale * mmd2(sums, nx, ny, unbiased, fault), bound=scale * mmd2_bound(bounds, nx, ny, unbiased), sums=sums,
                sum_bounds=bounds, kmin=kmin)


@functools.lru_cache(maxsize=None)
def ref_of(case, normalize, unbiased=False, fault=None):
    """The reference of a case, computed once and shared (do not modify the arrays)."""
    x, y = sets_of(case)
    return ref_score(x, y, SIGMA, bool(normalize), unbiased, SCALE, fault)
