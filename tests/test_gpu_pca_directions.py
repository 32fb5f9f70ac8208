"""PCA and attribute-direction kernels (csrc/pca.hip, direction_accum_kernel and the broadcast add of csrc/rowops.hip)
against float64 numpy references at the workflow's shapes: F = 4 096 (latent tap) and 257 x 1024 = 263 168 (U-ViT-L mid
block), N up to a few thousand, n_components = 50.  Every reference is computed from the exact fp32 data the kernel saw,
copied back to the host.  Each check states an analytic bound and a measured one (about 3x the largest error seen on an
MI355X, stated as a fraction of the analytic bound); it asserts the tighter of the two.  Large inputs are generated on the
device and only the slices a check needs come back."""
import numpy as np
import pytest
import torch

from oracle import attr_oracle
from tests.util import bf16_round

pytestmark = pytest.mark.gpu

U32, U64 = 2.0 ** -24, 2.0 ** -53          # unit roundoff of fp32 / fp64
F_MID = 257 * 1024                          # U-ViT-L mid-block tap
N_BIG = 1280


@pytest.fixture(scope="module")
def hip():
    from uspace_amd import _hip
    _hip.lib()
    return _hip


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _check_ratio(name, err, bound, measured):
    """err, bound: arrays (or scalars) of the same shape.  Asserts err <= bound * min(1, measured)."""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    ratio = float(np.max(err / bound)) if err.size else 0.0
    print(f"[{name}] max err / analytic bound = {ratio:.3g}  (max err {float(err.max()) if err.size else 0.0:.3g})")
    assert ratio <= min(1.0, measured), (name, ratio, measured)
    return ratio


# ------------------------------------------------------------------------------------------------ uspace_center_cols_f32
# xc = fp32(x - mu) with the mean and the difference in fp64: |xc - (x - mu)| <= 1/2 ulp(xc) plus the fp64 sum's, scaling's
# and difference's (N + 2) 2^-53 (mean|x| + |x|); so also <= 1 ulp32 of max(|x|, |mu|).  Measured: the full half ulp (the
# rounding is exact to nearest), so the analytic bound is the tighter one.
MEAS_CENTER = 1.0


def _center(hip, x, N, F):
    xc = torch.full_like(x, float("nan"))
    assert hip.lib().uspace_center_cols_f32(hip.ptr(x), hip.ptr(xc), N, F, hip.stream_ptr()) == 0
    return xc


def _center_check(name, x, xc):
    x64 = x.astype(np.float64)
    mu = x64.mean(axis=0)
    err = np.abs(xc.astype(np.float64) - (x64 - mu))
    bound = 0.5 * np.spacing(np.abs(xc)) + (len(x) + 2) * U64 * (np.abs(x64).mean(axis=0) + np.abs(x64))
    _check_ratio(name, err, bound, MEAS_CENTER)
    ulps = float((err / np.spacing(np.maximum(np.abs(x), np.abs(mu).astype(np.float32)))).max())
    print(f"[{name}] in ulp32 of max(|x|, |mu|): {ulps:.3g}")
    assert ulps <= 1.0, (name, ulps)


@pytest.mark.parametrize("N,F", [(1, 4), (63, 260), (200, 4096)])
def test_center_cols_small(hip, N, F):
    g = _gen(N * 7 + F)
    off = (torch.rand(F, device="cuda", generator=g) * 2 - 1) * 1e3
    off[: F // 4] *= 1e-3                                              # some columns with offsets near 0: both signs
    x = torch.randn(N, F, device="cuda", generator=g) + off
    xc = _center(hip, x, N, F)
    _center_check(f"center {N}x{F}", x.cpu().numpy(), xc.cpu().numpy())
    if N == 1:
        assert not xc.any()


@pytest.fixture(scope="module")
def big(hip):
    """[1280, 263 168] with column offsets up to 1e3 on unit-variance data, and its device-centred copy (2.7 GB)."""
    g = _gen(11)
    off = (torch.rand(F_MID, device="cuda", generator=g) * 2 - 1) * 1e3
    x = torch.randn(N_BIG, F_MID, device="cuda", generator=g)
    x += off
    xc = _center(hip, x, N_BIG, F_MID)
    yield x, xc
    del x, xc
    torch.cuda.empty_cache()


def _sample_cols(F, n, seed, block=128):
    rng = np.random.default_rng(seed)
    edges = [0, 1, 2, 3, block - 1, block, F - block - 1, F - block, F - 4, F - 3, F - 2, F - 1]
    cols = np.concatenate([[c for c in edges if 0 <= c < F], rng.choice(F, n, replace=False)])
    return torch.from_numpy(np.unique(cols)).cuda()


def test_center_cols_mid_block(big):
    x, xc = big
    cols = _sample_cols(F_MID, 4000, 1)
    _center_check("center 1280x263168", x[:, cols].cpu().numpy(), xc[:, cols].cpu().numpy())


# ----------------------------------------------------------------------------------------------------- uspace_gram_f64
# Products of fp32 data are exact in fp64; the k sum (the kernel's and numpy's) errs by at most F * 2^-53 * sum|x_i x_j|
# each.  Measured: 0.015 of that (N <= 200, F ~ 1 000), 0.0026 at 1280 x 263 168.
MEAS_GRAM = 0.05


def _gram(hip, x, N, F):
    G = torch.full((N, N), float("nan"), dtype=torch.float64, device="cuda")
    assert hip.lib().uspace_gram_f64(hip.ptr(x), hip.ptr(G), N, F, hip.stream_ptr()) == 0
    return G


def _gram_check(name, xr, Gsel, F):
    x64 = xr.astype(np.float64)
    ref = x64 @ x64.T
    bound = 2 * F * U64 * (np.abs(x64) @ np.abs(x64).T)
    assert np.isfinite(Gsel).all(), name
    return _check_ratio(name, np.abs(Gsel - ref), bound, MEAS_GRAM)


@pytest.mark.parametrize("N", [1, 17, 64, 65, 128, 129, 200])
def test_gram_tiles_and_feature_tail(hip, N):
    for F in (1024, 1028, 1032, 1036):                                # F % 16 = 0, 4, 8, 12
        g = _gen(N * 131 + F)
        x = torch.randn(N, F, device="cuda", generator=g) + 0.25
        G = _gram(hip, x, N, F).cpu().numpy()
        assert np.array_equal(G, G.T), (N, F)
        _gram_check(f"gram N={N} F={F}", x.cpu().numpy(), G, F)


def _edge_rows(N):
    rows = {0, 1, 15, 16, 31, 32, 33, N - 1, N - 2}
    for t in range(64, N, 64):
        rows |= {t - 1, t, t + 1}
    return np.array(sorted(r for r in rows if 0 <= r < N))


def test_gram_mid_block(hip, big):
    _x, xc = big
    G = _gram(hip, xc, N_BIG, F_MID).cpu().numpy()
    assert np.array_equal(G, G.T)
    rows = _edge_rows(N_BIG)
    assert len(rows) >= 48
    xr = xc[torch.from_numpy(rows).cuda()].cpu().numpy()
    _gram_check("gram 1280x263168 edge rows", xr, G[np.ix_(rows, rows)], F_MID)


# --------------------------------------------------------------------------------------------- uspace_project_rows_f64
# out = fp32(sum_k Ut[i, k] x[k, j]) with fp64 products and sums: |out - ref| <= 2^-24 |ref| + N 2^-52 sum|Ut||x| (and the
# fp32 rounding of that error).  Measured: 0.999 of that (the fp32 rounding of the output dominates): the analytic bound.
MEAS_PROJ = 1.0


def _project(hip, ut, x, n, N, F):
    out = torch.full((n, F), float("nan"), device="cuda")
    assert hip.lib().uspace_project_rows_f64(hip.ptr(ut), hip.ptr(x), hip.ptr(out), n, N, F, hip.stream_ptr()) == 0
    return out


def _project_check(name, ut, xcols, got):
    ref = ut @ xcols.astype(np.float64)
    acc = np.abs(ut) @ np.abs(xcols.astype(np.float64))
    bound = U32 * np.abs(ref) + (1 + U32) * ut.shape[1] * 2 * U64 * acc + np.finfo(np.float32).tiny
    assert np.isfinite(got).all(), name
    return _check_ratio(name, np.abs(got.astype(np.float64) - ref), bound, MEAS_PROJ)


@pytest.mark.parametrize("F", [4, 33, 4100])
def test_project_rows_small(hip, F):
    worst = 0.0
    for n in (1, 16, 17, 50):
        for N in (1, 3, 4, 5, 200):
            rng = np.random.default_rng(n * 1000 + N * 10 + F)
            ut = rng.standard_normal((n, N))
            x = (rng.standard_normal((N, F)) + 0.5).astype(np.float32)
            got = _project(hip, torch.from_numpy(ut).cuda(), torch.from_numpy(x).cuda(), n, N, F).cpu().numpy()
            worst = max(worst, _project_check(f"project n={n} N={N} F={F}", ut, x, got))
    print(f"[project F={F}] worst ratio {worst:.3g}")


def test_project_rows_mid_block(hip, big):
    _x, xc = big
    n = 50
    ut = np.random.default_rng(3).standard_normal((n, N_BIG)) / np.sqrt(N_BIG)
    out = _project(hip, torch.from_numpy(ut).cuda(), xc, n, N_BIG, F_MID)
    cols = _sample_cols(F_MID, 1500, 2)
    _project_check("project n=50 N=1280 F=263168", ut, xc[:, cols].cpu().numpy(), out[:, cols].cpu().numpy())
    assert bool(torch.isfinite(out).all())                          # every column block and both row blocks stored


# ---------------------------------------------------------------------------------------- uspace_normalize_rows_signed
def _normalize(hip, v):
    n, F = v.shape
    out = v.clone()
    assert hip.lib().uspace_normalize_rows_signed(hip.ptr(out), n, F, hip.stream_ptr()) == 0
    return out


def _normalize_check(name, vin, got):
    """Unit norm, sklearn's svd_flip sign (first index of argmax |v| positive) and the magnitudes of v / ||v||."""
    v64 = vin.astype(np.float64)
    nrm = np.linalg.norm(v64, axis=1)
    idx = np.argmax(np.abs(vin), axis=1)
    for r in range(len(vin)):
        if nrm[r] == 0:
            assert not got[r].any(), (name, r)
            continue
        assert got[r, idx[r]] > 0, (name, r, int(idx[r]), float(got[r, idx[r]]))
        assert abs(np.linalg.norm(got[r].astype(np.float64)) - 1.0) < 1e-6, (name, r)
        want = v64[r] / nrm[r] * np.sign(v64[r, idx[r]])
        assert np.all(np.abs(got[r] - want) <= 3 * U32 * np.abs(want) + 1e-45), (name, r)


def _tie_row(F, pairs, seed):
    row = np.random.default_rng(seed).uniform(-0.5, 0.5, F).astype(np.float32)
    for i, val in pairs:
        row[i] = val
    return row


@pytest.mark.parametrize("F,pairs", [
    (2048, [(64, -1.0), (1024, 1.0)]),         # across waves: index 64 is wave 1, index 1024 is thread 0 of wave 0
    (2048, [(64, 1.0), (1024, -1.0)]),
    (F_MID, [(1023, -3.0), (262144, 3.0)]),    # wave 15 against wave 0, 256 strides apart
    (2048, [(5, -1.0), (1029, 1.0)]),          # within one thread's stride
    (2048, [(3, 1.0), (60, -1.0)]),            # within one wave
    (100, [(10, -1.0), (90, 1.0)]),            # row shorter than the block
    (4099, [(700, -2.0), (3000, 2.0), (1500, 2.0)]),
], ids=["cross-wave", "cross-wave-pos", "cross-wave-long", "one-thread", "one-wave", "short", "three-way"])
def test_normalize_rows_ties(hip, F, pairs):
    v = np.stack([_tie_row(F, pairs, 0), -_tie_row(F, pairs, 0), _tie_row(F, pairs[::-1], 1)])
    got = _normalize(hip, torch.from_numpy(v).cuda()).cpu().numpy()
    _normalize_check(f"normalize ties F={F}", v, got)


def test_normalize_rows_random_and_zero(hip):
    g = _gen(5)
    for F in (F_MID, 4099, 17):
        v = torch.randn(50, F, device="cuda", generator=g) * torch.logspace(-3, 3, 50, device="cuda")[:, None]
        v[7] = 0.0                                                     # all-zero row stays zero
        got = _normalize(hip, v)
        assert bool(torch.isfinite(got).all())
        _normalize_check(f"normalize random F={F}", v.cpu().numpy(), got.cpu().numpy())


# ------------------------------------------------------------------------------------------------ pca_components end to end
def _host_top_directions(xc64, n, k_sub, iters=3, seed=0):
    """fp64 top-n right singular vectors of xc64 by subspace iteration + Rayleigh-Ritz (exact where the spectrum beyond
    k_sub is negligible, as for the planted data below), sklearn's svd_flip sign; and the singular values."""
    q = np.random.default_rng(seed).standard_normal((xc64.shape[1], k_sub))
    for _ in range(iters):
        q, _r = np.linalg.qr(xc64.T @ (xc64 @ q))
    _u, s, wt = np.linalg.svd(xc64 @ q, full_matrices=False)
    v = (q @ wt.T).T[:n]
    idx = np.argmax(np.abs(v), axis=1)
    return v * np.sign(v[np.arange(n), idx])[:, None], s


def _planted(N, F, k, s0, seed):
    """mean + U diag(s) V^T with zero-mean orthonormal U and s_i = s0 * 0.9^i, on the device."""
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((N, k))
    u, _r = np.linalg.qr(u - u.mean(axis=0))
    g = _gen(seed)
    vt = torch.randn(k, F, device="cuda", generator=g, dtype=torch.float64) / np.sqrt(F)
    mean = 2.0 + 0.5 * torch.randn(F, device="cuda", generator=g, dtype=torch.float64)
    us = torch.from_numpy(u * (s0 * 0.9 ** np.arange(k))).cuda()
    return (us @ vt + mean).to(torch.float32)


# Measured: 1 - cos <= 7.0e-14, |V V^T - I| <= 1.02e-7.
MEAS_PCA_COS, MEAS_PCA_ORTH = 2.1e-13, 3.1e-7


@pytest.mark.parametrize("N,shape,n,k,s0", [
    (640, (257, 1024), 50, 60, 1e4),          # the U-ViT-L mid-block tap, the reference's default n_components
    (4200, (4, 32, 32), 20, 30, 1e4),          # N > F: a rank-deficient Gram matrix (latent tap)
    (300, (3, 37, 23), 20, 30, 1e3),           # F % 4 == 1: padded to 16-byte feature groups
], ids=["mid-block", "rank-deficient", "padded"])
def test_pca_components_planted_spectrum(hip, N, shape, n, k, s0):
    from uspace_amd.tools.utils_pca import pca_components
    F = int(np.prod(shape))
    x = _planted(N, F, k, s0, seed=N + F)
    got = pca_components(x.view((N,) + shape), n).reshape(n, F).cpu().numpy().astype(np.float64)
    x64 = x.cpu().numpy().astype(np.float64)
    del x
    mu = x64.mean(axis=0)
    xc64 = x64 - mu
    del x64
    want, s = _host_top_directions(xc64, n, k + 16)
    # Only the fp32 rounding of the centred data perturbs the device's directions measurably: ||E||_F <= 2^-24 ||xc||_F
    # (plus the fp64 centring's 2^-51 (|xc| + |mu|)); by Wedin, sin(theta_i) <= ||E|| / (gap_i - ||E||), gap_i the distance
    # from sigma_i to its neighbours, and 1 - cos <= sin^2.  The fp32 output and its normalisation (entries within 3 2^-24
    # relative) add at most (3 2^-24)^2.
    e = U32 * float(np.linalg.norm(xc64)) + 2.0 ** -51 * float(np.sqrt(
        sum(((np.abs(xc64[r:r + 64]) + np.abs(mu)) ** 2).sum() for r in range(0, N, 64))))
    gaps = np.minimum(np.r_[np.inf, s[:n - 1] - s[1:n]], s[:n] - s[1:n + 1])
    assert np.all(gaps > 10 * e), (gaps.min(), e)
    eps = (e / (gaps - e)) ** 2 + (3 * U32) ** 2
    cos = np.sum(got * want, axis=1) / np.linalg.norm(got, axis=1)       # signed: same direction and same sign
    print(f"[pca N={N} F={F} n={n}] max(1 - cos) {float((1 - cos).max()):.3g}, eps in [{eps.min():.3g}, {eps.max():.3g}]")
    assert np.all(1 - cos <= np.minimum(eps, MEAS_PCA_COS)), (int(np.argmax(1 - cos - eps)), float((1 - cos).max()))
    idx = np.argmax(np.abs(got), axis=1)
    assert np.all(got[np.arange(n), idx] > 0)                            # svd_flip on the device's own output
    # fp32 unit rows within 3 2^-24 relative of directions that are orthogonal to within sin(theta_i) + sin(theta_j)
    orth = np.abs(got @ got.T - np.eye(n)).max()
    print(f"[pca N={N} F={F} n={n}] orthonormality {orth:.3g}")
    assert orth <= min(6 * U32 + 2 * float(np.sqrt(eps.max())), MEAS_PCA_ORTH)


# --------------------------------------------------------------------------- uspace_direction_accumulate / DirectionAccumulator
# Device summation: per call, chunks of 16 samples are summed in fp32 from zero, then each chunk sum is added once to the
# running fp32 sum.  Bound on the sum: u * sum_c [(m_c - 1) A_c + P_c] over chunks with m_c > 0 matches, A_c their sum of
# |feat|, P_c the running sum of A up to chunk c; then the division by the count and the difference each add one rounding.
# Measured: 0.19 of that (0.10 in the offset stress case).
MEAS_ACC = 0.6


def _acc_bound(batches, attrs, feats64, A):
    """Analytic bound [A, F] on |device direction - fp64 truth| for the given call sequence."""
    F = feats64.shape[1]
    out = []
    means = []
    for side in (1, 0):
        mask = (attrs == side).astype(np.float64)
        run = np.zeros((A, F))
        bound = np.zeros((A, F))
        lo = 0
        for b in batches:
            for c0 in range(lo, lo + b, 16):
                c1 = min(c0 + 16, lo + b)
                m = mask[c0:c1]
                a_c = m.T @ np.abs(feats64[c0:c1])
                cnt = m.sum(axis=0)[:, None]
                run += a_c
                bound += np.where(cnt > 0, np.maximum(cnt - 1, 0) * a_c + run, 0.0)
            lo += b
        count = mask.sum(axis=0)[:, None]
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = (mask.T @ feats64) / count
            out.append(U32 * bound / count + U32 * np.abs(mean))
        means.append(mean)
    return (out[0] + out[1]) * (1 + 1e-6) + U32 * np.abs(means[0] - means[1]), means[0] - means[1]


def _acc_run(batches, A, F, seed, offset=0.0, signal=0.0):
    from uspace_amd.tools.utils_attr import DirectionAccumulator
    rng = np.random.default_rng(seed)
    B = sum(batches)
    attrs = rng.choice([-1, 0, 1], size=(B, A)).astype(np.int32)
    attrs[:, 7] = rng.choice([-1, 0], size=B)                           # no positive example: NaN direction
    g = _gen(seed)
    feats = torch.randn(B, F, device="cuda", generator=g) + offset
    if signal:
        feats += signal * torch.from_numpy((attrs == 1).astype(np.float32)).cuda() @ torch.randn(A, F, device="cuda",
                                                                                                  generator=g)
    acc = DirectionAccumulator(A)
    lo = 0
    for b in batches:
        acc.update("0.50", feats[lo:lo + b], attrs[lo:lo + b])
        lo += b
    return acc.directions("0.50").reshape(A, F), feats, attrs


def _acc_check(name, got, feats_cols, attrs, batches):
    A = attrs.shape[1]
    bound, truth = _acc_bound(batches, attrs, feats_cols.astype(np.float64), A)
    assert np.isnan(got[7]).all() and np.isnan(truth[7]).all()
    keep = np.arange(A) != 7
    assert np.isfinite(got[keep]).all(), name
    err = np.abs(got[keep] - truth[keep])
    ratio = _check_ratio(name, err, bound[keep], MEAS_ACC)
    ref = attr_oracle.delta_directions(attrs, feats_cols)            # the reference formula, in fp32
    ref_err = np.abs(ref[keep] - truth[keep])
    print(f"[{name}] device max err {float(err.max()):.3g}, reference formula in fp32 {float(ref_err.max()):.3g}")
    return float(err.max()), float(ref_err.max()), ratio


@pytest.mark.parametrize("A", [40, 11])
@pytest.mark.parametrize("F", [4096, F_MID])
def test_direction_accumulator_ragged_batches(hip, A, F):
    batches = [1, 15, 16, 17, 64, 3, 33]
    got, feats, attrs = _acc_run(batches, A, F, seed=A + F, offset=0.5)
    cols = _sample_cols(F, 2000, 4, block=1024) if F > 4096 else torch.arange(F, device="cuda")
    _acc_check(f"accumulate A={A} F={F}", got[:, cols.cpu().numpy()], feats[:, cols].cpu().numpy(), attrs, batches)


def test_direction_accumulator_offset_stress(hip):
    """5 000 samples on a common offset of 100 with a small attribute signal: the running sums reach 2.5e5 per side."""
    batches = [64] * 78 + [8]
    got, feats, attrs = _acc_run(batches, 40, 4096, seed=9, offset=100.0, signal=0.05)
    dev, ref, _ratio = _acc_check("accumulate stress", got, feats.cpu().numpy(), attrs, batches)
    assert dev <= ref, (dev, ref)               # no worse than the reference's own fp32 means


# ------------------------------------------------------------------------------------------------ uspace_add_broadcast_rows
@pytest.mark.parametrize("B,per", [(1024, 4096), (700, 4099), (16, F_MID)])
@pytest.mark.parametrize("rows", [False, True], ids=["scale", "row_scale"])
@pytest.mark.parametrize("with_bf16", [False, True], ids=["f32", "bf16"])
def test_add_broadcast_rows(hip, B, per, rows, with_bf16):
    """x[b] += fp32(scale * row_scale[b]) * delta over a grid-stride loop that wraps (B * per > 2 M); within 1 ulp of the
    fp64 result (an FMA rounds once; measured: 0.5 ulp), the bf16 copy the round-to-nearest-even of the fp32 result."""
    g = _gen(B + per)
    x = torch.randn(B, per, device="cuda", generator=g) * 3
    d = torch.randn(per, device="cuda", generator=g)
    scale = 0.7
    rs = None
    if rows:
        rs = torch.rand(B, device="cuda", generator=g) * 4 - 2
        rs[0], rs[-1] = 0.0, -1.5
    xb = torch.empty(B, per, dtype=torch.bfloat16, device="cuda") if with_bf16 else None
    x0 = x.cpu().numpy().astype(np.float64)
    hip.add_broadcast(x, d, scale, x_bf16=xb, row_scale=rs)
    got = x.cpu().numpy()
    sc = (np.float32(scale) * rs.cpu().numpy()).astype(np.float64) if rows else np.full(B, np.float32(scale), np.float64)
    exact = x0 + sc[:, None] * d.cpu().numpy().astype(np.float64)[None, :]
    r32 = exact.astype(np.float32)
    ulps = np.abs(got.astype(np.float64) - exact) / np.spacing(np.abs(r32))
    print(f"[broadcast B={B} per={per} rows={rows}] max {float(ulps.max()):.3g} ulp")
    assert float(ulps.max()) <= 1.0
    if with_bf16:
        want = torch.from_numpy(bf16_round(got)).to(torch.bfloat16)
        assert torch.equal(xb.cpu().view(torch.int16), want.view(torch.int16))
