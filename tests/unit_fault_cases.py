"""Inputs, float64 references and bounds of the GPU unit tests that exclude the planted faults no block-level metric resolves (a
helper, not a test): a LayerNorm eps of 1e-6 and the tanh form of GELU move a block's update by 1e-5 ... 2e-4 (tests/uvit_stages.py::FAULTS,
tests/clip_stages.py::FAULTS), below the rounding noise of a block and too small a direction to project that noise onto.  They are
visible where the inputs are chosen for them:

  rows whose variance is of the order of eps (``ln_eps_rows``, ``folded_eps_case``): with var = eps the normalised row changes by
      sqrt(2 / 1.1) - 1 = 35 % between the two eps -- tests/test_gpu_ops.py::test_layernorm, ::test_layernorm_folded_through_gemms_rows_at_eps,
      tests/test_gpu_clip_parity.py::test_layernorm_kernels_at_d768;
  pre-activations on GELU's negative tail (``gelu_tail_case``): at z = -3 ... -4 the tanh form is 10 ... 45 % below the erf form, the
      bf16 rounding of the stored value 0.4 % -- tests/test_gpu_ops.py::test_gemm_epilogues.

The GPU tests build their inputs, references and bounds with the functions here; tests/test_uvit_faults_host.py and
tests/test_clip_faults_host.py build the faulty references from the same inputs and require them to lie FAULT_MARGIN bounds from
the true ones.  numpy float64 throughout; operands that the kernels read as bf16 are rounded here."""
import math

import numpy as np
import torch

from tests.util import bf16_round

BF16_EPS = 2.0 ** -8          # half-ulp relative rounding of a bf16 store (tests/test_gpu_ops.py)
LN_EPS = 1e-5
GELU_ABS = 4.1e-7             # the epilogue's erf-GELU against the exact one, absolute (the fit's own bound, uspace_amd/csrc/common.h)


def _rand(rng, *shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ LayerNorm
def layernorm_f64(x, g, b, eps=LN_EPS, unbiased=False):
    x = np.asarray(x, np.float64)
    mu = x.mean(-1, keepdims=True)
    var = x.var(-1, ddof=1 if unbiased else 0, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * np.asarray(g, np.float64) + np.asarray(b, np.float64)


def ln_eps_rows(M, D, seed):
    """(x [M, D], gamma, beta) fp32: row m is s_m (N(0, 1) + 0.5) with s_m log-spaced over [1e-3, 1e-2], so the row variances run from
    1e-6 to 1e-4, through eps = 1e-5 (row M // 2)."""
    rng = np.random.default_rng(seed)
    s = np.logspace(-3, -2, M).astype(np.float32)[:, None]
    x = (s * (_rand(rng, M, D) + 0.5)).astype(np.float32)
    return x, (_rand(rng, D) * 0.2 + 1.0).astype(np.float32), _rand(rng, D, scale=0.1)


LAYERNORM_SHAPES = [(5, 64), (1031, 512), (777, 1024), (9, 2048), (77, 768), (4928, 768)]      # test_layernorm's (M, D); eps rows: seed D + M
CLIP_LAYERNORM_M = (77, 4928)                                     # test_layernorm_kernels_at_d768's M at D = 768; eps rows: seed 1100 + M


def ln_bf16_bound(ref):
    """test_layernorm's element-wise bound on a bf16 LayerNorm output."""
    return BF16_EPS * np.abs(ref) * 1.01 + 2e-5


def ln_noise_scale(x, g, b, eps=LN_EPS):
    """test_layernorm_kernels_at_d768's fp32 noise scale of one element: 2^-24 (|gamma| (|x| + |mean|) / sigma + |beta|)."""
    xd = np.asarray(x, np.float64)
    sigma = np.sqrt(xd.var(-1, keepdims=True) + eps)
    return 2.0 ** -24 * (np.abs(np.asarray(g, np.float64)) * (np.abs(xd) + np.abs(xd.mean(-1, keepdims=True))) / sigma
                         + np.abs(np.asarray(b, np.float64)))


# ------------------------------------------------------------------------------------------------------------------ the folded path
FOLDED_EPS_CASES = [(515, 256, 128, 256), (4 * 257, 512, 2048, 1536), (8 * 257, 1024, 64, 4096)]   # (M, D, Kp, N2) of the unit test's own table
FOLDED_Y_TOL = 4e-3           # test_layernorm_folded_through_gemms's bound on the consumer's output, rel-L2


def folded_eps_case(M, D, Kp, N2):
    """The operands of test_layernorm_folded_through_gemms (producer x = A W^T + b + R, consumer LN(x) W2^T + b2 from the centred
    copy) with every fifth row, the first and the last among them, made a row whose variance is of the order of eps: A = 0 and
    R = -b + s_m N(0, 1), s_m log-spaced over [2e-3, 6e-3] (variance 4e-6 ... 3.6e-5), centred by c = 0.3 s_m -- close to the row's
    mean, not equal to it, as the constants of the other rows are.  -> dict of fp32 arrays and ``rows`` (the eps rows)."""
    rng = np.random.default_rng(M + D + N2 + 1)
    A = bf16_round(_rand(rng, M, Kp))
    W = bf16_round(_rand(rng, D, Kp) * 0.2)
    b = _rand(rng, D)
    R = (_rand(rng, M, D) * 1.5 + _rand(rng, M, 1) * 2.0).astype(np.float32)
    gam, bet = (_rand(rng, D) * 0.2 + 1.0).astype(np.float32), _rand(rng, D, scale=0.1)
    W2 = (_rand(rng, N2, D) * 0.05).astype(np.float32)
    b2 = _rand(rng, N2)
    c = R.mean(axis=1).astype(np.float32)
    rows = np.unique(np.concatenate([np.arange(0, M, 5), [M - 1]]))
    s = np.logspace(math.log10(2e-3), math.log10(6e-3), rows.size).astype(np.float32)
    A[rows] = 0.0
    R[rows] = (-b[None, :] + s[:, None] * _rand(rng, rows.size, D)).astype(np.float32)
    c[rows] = 0.3 * s
    return dict(A=A, W=W, b=b, R=R, gam=gam, bet=bet, W2=W2, b2=b2, c=c, rows=rows)


def folded_reference(case, rows, eps=LN_EPS):
    """float64 (x, y) of the rows ``rows``: x = A W^T + b + R and y = LN(x; gamma, beta, eps) W2^T + b2 from the fp32 operands."""
    f = lambda k: case[k].astype(np.float64)
    x = f("A")[rows] @ f("W").T + f("b") + f("R")[rows]
    return x, layernorm_f64(x, case["gam"], case["bet"], eps) @ f("W2").T + f("b2")


# ------------------------------------------------------------------------------------------------------------------ GELU
def gelu_f64(z, form="erf"):
    z = torch.from_numpy(np.asarray(z, np.float64))
    if form == "tanh":
        return (0.5 * z * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (z + 0.044715 * z ** 3)))).numpy()
    return (0.5 * z * torch.special.erfc(-z / math.sqrt(2.0))).numpy()           # erfc: no cancellation on the negative tail


def gelu_tail_case(M, N, K, seed):
    """Operands of a bias + GELU -> bf16 launch whose pre-activations sit on GELU's negative tail: A ~ N(0, 1) and W ~ 0.05 N(0, 1),
    both bf16, bias -3.4 + 0.3 N(0, 1): z = -3.4 +- 0.5, most of it in [-4.5, -2.5].  -> (A, W, b, rows): ``rows`` the rows the float64
    reference is taken on (the first and last 300 and 600 more)."""
    rng = np.random.default_rng(seed)
    A = bf16_round(_rand(rng, M, K))
    W = bf16_round(_rand(rng, N, K) * 0.05)
    b = (-3.4 + 0.3 * rng.standard_normal(N)).astype(np.float32)
    rows = np.unique(np.concatenate([rng.integers(0, M, 600), np.arange(min(M, 300)), np.arange(max(M - 300, 0), M)]))
    return A, W, b, rows


EPILOGUE_SHAPES = {False: (515, 256, 192), True: (4099, 4096, 64)}      # test_gemm_epilogues's two launches (big: 256x256 tiles)


def epilogue_gelu_tail_case(big):
    return gelu_tail_case(*EPILOGUE_SHAPES[bool(big)], seed=7 + int(big))


def gelu_tail_reference(A, W, b, rows, form="erf"):
    """(GELU(z) in float64, the element-wise bound) on ``rows``, z = A W^T + b.  The bound is test_gemm_epilogues's bf16 term, and
    instead of that test's flat 1e-4 (which is the size of the values here) what the fp32 arithmetic can do: the epilogue's GELU
    to GELU_ABS, and the fp32 accumulation of z, at most (K + 2) 2^-24 (sum_k |a_k w_k| + |b|), times GELU's slope -- below 0.13 in
    magnitude for z < -0.76, below 1.13 everywhere."""
    a, w, bb = A[rows].astype(np.float64), W.astype(np.float64), b.astype(np.float64)
    z = a @ w.T + bb
    dz = (A.shape[1] + 2) * 2.0 ** -24 * (np.abs(a) @ np.abs(w).T + np.abs(bb))
    ref = gelu_f64(z, form)
    return ref, BF16_EPS * np.abs(gelu_f64(z)) * 1.01 + GELU_ABS + np.where(z < -0.76, 0.13, 1.13) * dz
