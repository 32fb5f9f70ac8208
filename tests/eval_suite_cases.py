"""Shared by tests/test_eval_suite_cases.py (CPU) and tests/test_gpu_eval_suite.py (GPU); a helper, not a test: the inputs, the
float64 references, the planted faults and the bounds of the Inception Score, the logits head and sFID's spatial features
(uspace_amd/tools/inception_score.py, sfid_score.py, eval_suite.py; csrc/inception_score.hip).

Bounds.  They are the project's own, from tests/test_gpu_inception.py:TOL, not fitted to the new code:
  stage = 2.5e-6   rel-L2 of one fp32 conv-GEMM stage against float64 (measured there on K up to 4032): the logits (one fp32 fma
                   chain over K <= 2048 per element, like a 1 x 1 convolution) and the spatial features (a slice of stage 14)
  stats = 1e-10    fp64 device reductions against numpy: every split score and their mean relative, their std absolute relative
                   to the mean
  fid_path = 1.6e-6  a Frechet distance through the whole path

Definitions restated here in float64.
  Inception Score: split k covers the rows [k N // splits, (k + 1) N // splits); p_i = softmax(logits_i), pbar = mean_i p_i over
  the split, score_k = exp(mean_i sum_c p_ic (log p_ic - log pbar_c)), terms with p_ic == 0 contributing 0; the result is
  (mean_k score_k, std_k score_k) with ddof = 0.
  Logits: pool @ W.T + b.
  Spatial features: stage 14 (Mixed_6d) as NHWC, [..., :7], flattened in (h, w, c) order."""
import functools

import numpy as np

TOL = dict(stage=2.5e-6, stats=1e-10, fid_path=1.6e-6)      # == tests/test_gpu_inception.py:TOL (asserted by the CPU test)

# (N, C, splits): ragged splits, one row per split, a single split, C below and above 1000
IS_CASES = [(1000, 1008, 7), (97, 1008, 10), (64, 40, 1), (301, 1008, 3), (10, 1008, 10)]
ZERO_CASE = (200, 1008, 4)          # 5 % of the entries at -1e4 and one class at -1e4 in every row: p = 0 and pbar = 0
IS_FAULTS = ("global_marginal", "truncate_1000", "kl_swapped", "mean_of_exp", "ceil_splits", "ddof1", "dropped_bias")
BIAS_STD = 0.5

# (B, K, C): one row, a ragged row tile, more than 128 rows, ragged columns, tiny shapes, the smallest K
LOGIT_CASES = [(1, 2048, 1008), (7, 2048, 1008), (130, 2048, 1008), (129, 2048, 65), (3, 64, 5), (2, 16, 1)]
LOGIT_FAULTS = ("relu", "no_bias", "k_truncated")

SPATIAL_FAULTS = ("stage_15", "last_channels", "chw_order")


# ------------------------------------------------------------------------------------------ Inception Score
def make_logits(N, C, seed=0, zeros=False):
    """fp32 [N, C]: 2.5 randn, +6 on a label that drifts with the row index, label_i = (i C // N + randint(C // 8)) % C, so the
    marginal of a split differs from the global one.  zeros: 5 % of the entries and the whole of class 3 set to -1e4."""
    rng = np.random.default_rng(1000 + seed)
    x = (2.5 * rng.standard_normal((N, C))).astype(np.float32)
    label = (np.arange(N) * C // N + rng.integers(0, max(C // 8, 1), N)) % C
    x[np.arange(N), label] += np.float32(6.0)
    if zeros:
        x[rng.random((N, C)) < 0.05] = np.float32(-1e4)
        x[:, 3] = np.float32(-1e4)
    return x


@functools.lru_cache(maxsize=None)
def logits_of(case, zeros=False):
    x = make_logits(case[0], case[1], seed=IS_CASES.index(case) if case in IS_CASES else 99, zeros=zeros)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def bias_of(C):
    return (BIAS_STD * np.random.default_rng(77).standard_normal(C)).astype(np.float32)


def split_bounds(N, splits, fault=None):
    if fault == "ceil_splits":
        m = -(-N // splits)
        return [(min(k * m, N), min((k + 1) * m, N)) for k in range(splits)]
    return [(k * N // splits, (k + 1) * N // splits) for k in range(splits)]


def softmax64(x):
    x = np.asarray(x, np.float64)
    e = np.exp(x - x.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def _xlogy_diff(p, q):
    """sum over classes of p (log p - log q) with 0 log 0 = 0, per row."""
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(p > 0, p * (np.log(p) - np.log(q)), 0.0)
    return t.sum(1)


def ref_split_scores(logits, splits, fault=None):
    """float64 [splits]: the score of every split as defined above (or with a planted fault)."""
    x = np.asarray(logits, np.float64)
    if fault == "truncate_1000":
        x = x[:, :1000]
    if fault == "dropped_bias":
        x = x - bias_of(x.shape[1]).astype(np.float64)
    p = softmax64(x)
    out = []
    for lo, hi in split_bounds(len(x), splits, fault):
        ps = p[lo:hi]
        pbar = (p if fault == "global_marginal" else ps).mean(0, keepdims=True)
        if fault == "kl_swapped":
            kl = _xlogy_diff(np.broadcast_to(pbar, ps.shape), ps)
        else:
            kl = _xlogy_diff(ps, pbar)
        out.append(np.exp(kl).mean() if fault == "mean_of_exp" else np.exp(kl.mean()))
    return np.array(out)


def ref_inception_score(logits, splits, fault=None):
    """(mean, std) over the splits, ddof = 0."""
    s = ref_split_scores(logits, splits, fault)
    return float(np.mean(s)), float(np.std(s, ddof=1 if fault == "ddof1" else 0))


def fault_exposed_by(fault, case):
    """Whether a case can show a fault at all: a single split has no split rule, marginal or spread to get wrong; with one row
    per split every p_i is its own marginal and every score is 1."""
    N, C, splits = case
    rows = N // splits
    if fault in ("global_marginal",):
        return splits > 1
    if fault == "truncate_1000":
        return C > 1000 and rows > 1
    if fault in ("kl_swapped", "mean_of_exp", "dropped_bias"):
        return rows > 1
    if fault == "ceil_splits":
        return splits > 1 and N % splits != 0
    if fault == "ddof1":
        return splits > 1 and rows > 1
    raise KeyError(fault)


def is_deviation(good, bad):
    """(relative change of the mean, change of the std relative to the mean): the two quantities the GPU test bounds."""
    return abs(bad[0] - good[0]) / good[0], abs(bad[1] - good[1]) / good[0]


# ------------------------------------------------------------------------------------------ logits
@functools.lru_cache(maxsize=None)
def logit_operands(case):
    """(pool |randn| [B, K], W std 2 / sqrt(K) [C, K], b std 0.5 [C]) fp32: logits of spread about 2 and of both signs, so a
    ReLU left in the epilogue is a gross error."""
    B, K, C = case
    rng = np.random.default_rng(2000 + LOGIT_CASES.index(case))
    pool = np.abs(rng.standard_normal((B, K))).astype(np.float32)
    W = (2.0 / np.sqrt(K) * rng.standard_normal((C, K))).astype(np.float32)
    b = (BIAS_STD * rng.standard_normal(C)).astype(np.float32)
    for a in (pool, W, b):
        a.setflags(write=False)
    return pool, W, b


def ref_logits(pool, W, b=None, fault=None):
    pool, W = np.asarray(pool, np.float64), np.asarray(W, np.float64)
    if fault == "k_truncated":                       # the last 16 of K left out
        pool, W = pool[:, :-16], W[:, :-16]
    out = pool @ W.T
    if b is not None and fault != "no_bias":
        out = out + np.asarray(b, np.float64)
    if fault == "relu":
        out = np.maximum(out, 0.0)
    return out


def worst_row_rel_l2(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float((np.linalg.norm(got - ref, axis=1) / np.linalg.norm(ref, axis=1)).max())


# ------------------------------------------------------------------------------------------ spatial features
def ref_spatial(stage_nchw, channels=7, fault=None):
    """[B, h * w * channels] from a stage output in NCHW (the layout of tests/inception_stages.py): NHWC, the first
    ``channels`` channels, flattened in (h, w, c) order."""
    a = np.asarray(stage_nchw)
    B = a.shape[0]
    if fault == "last_channels":
        a = a[:, -channels:]
    else:
        a = a[:, :channels]
    if fault == "chw_order":
        return a.reshape(B, -1)
    return a.transpose(0, 2, 3, 1).reshape(B, -1)


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))
