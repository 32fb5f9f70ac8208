"""The ODE state kernels against fp64 on the host at the sizes the workflow runs them: uspace_ode_combine (y + sum c_i k_i) and
uspace_ode_error_norm (RMS of err / (atol + rtol max(|y0|, |y1|)), plus the raw sum of squares a sharded solve all-reduces).

The state of a U-ViT solve is B * 4 * 32 * 32 floats.  The norm launches at most 1024 blocks of 256 threads (262 144 elements per
lap): B = 64 is exactly one lap, B = 65 and the nine-scale sweep (9 * 32 rows) take a second and a fifth.  The fp64 side always
uses the fp32-rounded coefficients, rtol and atol the wrapper passes (ctypes c_float), so the bounds below are the kernels' own
round-off and nothing else.  ``ShadowOps`` checks every call a real solve issues -- the stage rows, c_sol, c_err, c_mid, the
dense-output weights, _neg's [-2.0] and the initial-step probes, with the driver's aliasing (y0 both as y and as a k)."""
import math

import numpy as np
import pytest
import torch


pytestmark = pytest.mark.gpu

U = 2.0 ** -24
ROWS = 4 * 32 * 32
SIZES = [b * ROWS for b in (1, 2, 4, 16, 32, 63, 64, 65, 9 * 32)] + [1, 3, 255, 257, 4097, 262143, 262145]
# Largest |error| / bound seen per check, printed at the end of the module (-s).  MI355X-measured: combine 0.64, combine in a solve
# 0.72, combine aliasing y 0.48; norm 0.069, norm in a solve 0.058, atol-dominated 0.018, one dominant element 0.12, poisoned
# scratch 0.033 -- the bounds are the kernels' worst-case round-off, 1.4x to 57x above what they reach.
WORST = {}


def _note(key, ratio):
    WORST[key] = max(WORST.get(key, 0.0), float(ratio))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nworst error / bound:", {k: f"{v:.3g}" for k, v in sorted(WORST.items())})


@pytest.fixture(scope="module")
def hip():
    from uspace_amd import _hip
    return _hip


def f32(c):
    return float(np.float32(c))


def combine_bound_check(out, y, ks, coefs, key):
    """|out - ref| <= (n_k + 1) u (|y| + sum |c_i| |k_i|), ref in fp64 from the fp32 operands and fp32-rounded coefficients."""
    y = np.asarray(y, np.float64)
    ref, mag = y.copy(), np.abs(y)
    for k, c in zip(ks, coefs):
        k = np.asarray(k, np.float64)
        ref += f32(c) * k
        mag += abs(f32(c)) * np.abs(k)
    bound = (len(ks) + 1) * U * mag
    err = np.abs(np.asarray(out, np.float64) - ref)
    bad = err > bound
    assert not bad.any(), (key, int(np.argmax(bad)), float(err.max()), float(bound[np.argmax(bad)]))
    nz = bound > 0
    if nz.any():
        _note(key, (err[nz] / bound[nz]).max())
    else:
        assert (err == 0).all()


def norm_reference(y0, y1, ks, coefs, rtol, atol):
    """fp64 (rms, sum of squares) and a bound on the fp32 kernel's error in the sum of squares: each ratio carries the round-off
    of err (n_k terms), of tol and of the division; the sum of n non-negative terms adds at most its tree depth in ulps."""
    y0, y1 = np.asarray(y0, np.float64), np.asarray(y1, np.float64)
    e, mag = np.zeros_like(y0), np.zeros_like(y0)
    for k, c in zip(ks, coefs):
        k = np.asarray(k, np.float64)
        e += f32(c) * k
        mag += abs(f32(c)) * np.abs(k)
    tol = f32(atol) + f32(rtol) * np.maximum(np.abs(y0), np.abs(y1))
    r = e / tol
    dr = ((len(ks) + 1) * U * mag + 4 * U * np.abs(e)) / tol
    sq = float(np.sum(r * r))
    n = y0.size
    laps = -(-n // (1024 * 256))
    depth = laps + 6 + 2 + 4 + 8 + 2              # lap sum, wave / block reduction, finish: 4 partials per thread, wave, block
    bound = float(np.sum(2 * np.abs(r) * dr + dr * dr)) + depth * U * sq
    return math.sqrt(sq / n), sq, bound


def check_norm(result, y0, y1, ks, coefs, rtol, atol, key):
    rms, sq, bound = norm_reference(y0, y1, ks, coefs, rtol, atol)
    got_rms, got_sq = (float(v) for v in result.cpu().tolist())
    n = np.asarray(y0).size
    assert abs(got_sq - sq) <= bound, (key, got_sq, sq, bound)
    # rms = sqrt(sq / n) in fp32: half the relative error of sq plus the division, the square root and the count's rounding
    rb = 0.5 * bound / max(sq, 1e-300) + 4 * U
    assert abs(got_rms - rms) <= rb * rms + 1e-38, (key, got_rms, rms)
    # result[1] == result[0]^2 * n up to the rounding of the finish kernel's divide and square root
    if got_sq > 0:
        assert abs(got_rms * got_rms * n / got_sq - 1.0) <= 8 * U, key
    if bound > 0:
        _note(key, abs(got_sq - sq) / bound)
    return got_rms, got_sq


def _operands(rng, n, nk):
    y = rng.standard_normal(n).astype(np.float32)
    ks = [(rng.standard_normal(n) * 10.0 ** rng.uniform(-2, 1)).astype(np.float32) for _ in range(nk)]
    return y, ks


# dopri5's error weights at dt = 0.05 and a mixed set: the coefficient lists a solve passes are of this size and sign pattern
C_ERR = [0.05 * c for c in (71 / 57600, 0.0, -71 / 16695, 71 / 1920, -17253 / 339200, 22 / 525, -1 / 40)]
C_MIX = [0.3, -1.2, 0.0, 2.5, 1e-3, -0.7, 0.11, -7.25]


@pytest.mark.parametrize("n", SIZES)
def test_ode_combine_against_fp64(hip, n):
    rng = np.random.default_rng(n)
    y, ks = _operands(rng, n, 8)
    dy, dks = torch.from_numpy(y).cuda(), [torch.from_numpy(k).cuda() for k in ks]
    for nk in range(0, 9):
        coefs = (C_MIX if nk % 2 else C_ERR + [0.5])[:nk]
        out = torch.full((n + 64,), float("nan"), device="cuda")         # a guard tail that must stay untouched
        hip.ode_combine(out[:n], dy, dks[:nk], coefs)
        o = out.cpu().numpy()
        assert np.isnan(o[n:]).all(), "ode_combine wrote past n"
        combine_bound_check(o[:n], y, ks[:nk], coefs, "combine")
    # out aliasing y (the header allows it)
    yy = dy.clone()
    hip.ode_combine(yy, yy, dks[:3], C_MIX[:3])
    combine_bound_check(yy.cpu().numpy(), y, ks[:3], C_MIX[:3], "combine_alias")


@pytest.mark.parametrize("n", SIZES)
def test_ode_error_norm_against_fp64(hip, n):
    rng = np.random.default_rng(100 + n)
    y0, ks = _operands(rng, n, 8)
    y1 = (y0 + rng.standard_normal(n).astype(np.float32) * 1e-2).astype(np.float32)
    dy0, dy1 = torch.from_numpy(y0).cuda(), torch.from_numpy(y1).cuda()
    dks = [torch.from_numpy(k).cuda() for k in ks]
    scratch = torch.empty(1024, device="cuda")
    res = torch.empty(2, device="cuda")
    for nk in range(1, 9):
        coefs = (C_ERR + [0.5])[:nk] if nk % 2 else C_MIX[:nk]
        for rtol, atol in ((1e-5, 1e-5), (1e-3, 1e-4)):
            hip.ode_error_norm(dy0, dy1, dks[:nk], coefs, rtol, atol, scratch, res)
            check_norm(res, y0, y1, ks[:nk], coefs, rtol, atol, "norm")


def test_ode_error_norm_atol_dominated_half(hip):
    """Half the state near 0: there tol is atol and the ratios reach ~1e5; the other half is O(1) with ratios ~1."""
    n = 9 * 32 * ROWS
    rng = np.random.default_rng(3)
    y0 = rng.standard_normal(n).astype(np.float32)
    y0[::2] = (rng.standard_normal(n // 2) * 1e-9).astype(np.float32)
    y1 = y0.copy()
    k = rng.standard_normal(n).astype(np.float32)
    res, scratch = torch.empty(2, device="cuda"), torch.empty(1024, device="cuda")
    hip.ode_error_norm(torch.from_numpy(y0).cuda(), torch.from_numpy(y1).cuda(), [torch.from_numpy(k).cuda()], [1.0], 1e-5, 1e-5,
                       scratch, res)
    rms, _ = check_norm(res, y0, y1, [k], [1.0], 1e-5, 1e-5, "norm_atol")
    assert rms > 1e4


@pytest.mark.parametrize("n,where", [
    (262145, [0, 255, 256, 262143, 262144]),
    (9 * 32 * ROWS, [0, 256 * 1023, 256 * 1024 - 1, 262143, 262144, 2 * 262144 + 17, 9 * 32 * ROWS - 1]),
    (64 * ROWS, [0, 255 * 256, 256 * 1023 + 255, 64 * ROWS - 1]),
    (4097, [0, 4095, 4096]),
])
def test_ode_error_norm_one_element_dominates(hip, n, where):
    """One element carries > 99 % of the sum: a lap, block, wave or partial that the reduction dropped would show at once."""
    rng = np.random.default_rng(n)
    y0 = rng.standard_normal(n).astype(np.float32)
    k = (rng.standard_normal(n) * 1e-5).astype(np.float32)
    dy0 = torch.from_numpy(y0).cuda()
    res, scratch = torch.empty(2, device="cuda"), torch.empty(1024, device="cuda")
    for i in where:
        kk = k.copy()
        kk[i] = np.float32(1e-5 * 100.0 * math.sqrt(n))        # its squared ratio ~1e4 n against ~n for the rest
        hip.ode_error_norm(dy0, dy0, [torch.from_numpy(kk).cuda()], [1.0], 1e-5, 1e-5, scratch, res)
        _, sq = check_norm(res, y0, y0, [kk], [1.0], 1e-5, 1e-5, "norm_dominant")
        r_i = float(kk[i]) / (f32(1e-5) + f32(1e-5) * abs(float(y0[i])))
        assert r_i * r_i > 0.99 * sq, (i, r_i * r_i, sq)


def test_ode_error_norm_never_reads_stale_partials(hip):
    """After a call that filled all 1024 partials, the scratch is poisoned with NaN: smaller calls use only their own blocks."""
    rng = np.random.default_rng(9)
    scratch, res = torch.empty(1024, device="cuda"), torch.empty(2, device="cuda")
    big = 9 * 32 * ROWS
    y = rng.standard_normal(big).astype(np.float32)
    k = rng.standard_normal(big).astype(np.float32)
    dy, dk = torch.from_numpy(y).cuda(), torch.from_numpy(k).cuda()
    hip.ode_error_norm(dy, dy, [dk], [1e-4], 1e-5, 1e-5, scratch, res)
    check_norm(res, y, y, [k], [1e-4], 1e-5, 1e-5, "norm")
    for n in (1, 3, 255, 257, 4097, 262143, 262144, big):
        scratch.fill_(float("nan"))
        hip.ode_error_norm(dy[:n], dy[:n], [dk[:n]], [1e-4], 1e-5, 1e-5, scratch, res)
        check_norm(res, y[:n], y[:n], [k[:n]], [1e-4], 1e-5, 1e-5, "norm_stale")


@pytest.mark.parametrize("slot", ["y0", "y1", "k0", "k_last"])
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")], ids=["nan", "inf", "-inf"])
@pytest.mark.parametrize("n,i", [(262145, 262144), (64 * ROWS, 12345), (257, 0)])
def test_ode_error_norm_non_finite_input_gives_non_finite_norm(hip, slot, bad, n, i):
    """A NaN or Inf in y0, y1 or a k with a non-zero coefficient must not yield a finite norm: the solver would accept the step.
    (Before the kernel fix fmaxf dropped a NaN y1 and an infinite y0 / y1 gave tol = Inf, ratio 0.)"""
    rng = np.random.default_rng(11)
    y0 = rng.standard_normal(n).astype(np.float32)
    y1 = y0.copy()
    ks = [rng.standard_normal(n).astype(np.float32) for _ in range(3)]
    target = {"y0": y0, "y1": y1, "k0": ks[0], "k_last": ks[2]}[slot]
    target[i] = bad
    res, scratch = torch.empty(2, device="cuda"), torch.empty(1024, device="cuda")
    hip.ode_error_norm(torch.from_numpy(y0).cuda(), torch.from_numpy(y1).cuda(), [torch.from_numpy(k).cuda() for k in ks],
                       [1e-3, -2e-3, 5e-4], 1e-5, 1e-5, scratch, res)
    got = res.cpu().numpy()
    assert not np.isfinite(got[0]) and not np.isfinite(got[1]), (slot, bad, got)


def test_ode_state_ops_refuse_mismatched_operands(hip):
    y = torch.zeros(8, device="cuda")
    with pytest.raises(hip.UspaceHipError):
        hip.ode_combine(torch.empty_like(y), y, [y, y], [1.0])
    with pytest.raises(hip.UspaceHipError):
        hip.ode_error_norm(y, y, [y], [1.0, 2.0], 1e-5, 1e-5, torch.empty(1024, device="cuda"), torch.empty(2, device="cuda"))
    with pytest.raises(hip.UspaceHipError):
        hip.ode_error_norm(y, y, [y], [1.0], 1e-5, 1e-5, torch.empty(1023, device="cuda"), torch.empty(2, device="cuda"))


# ------------------------------------------------------------------------------------------------------ calls of real solves
def shadow_ops_class():
    from uspace_amd.odeint import HipStateOps

    class ShadowOps(HipStateOps):
        """HipStateOps that re-checks every call against fp64 on the host (operands copied after the kernel ran: nothing here
        writes them, and out never aliases an operand in the driver)."""
        calls = None

        def combine(self, y, ks, coefs):
            out = super().combine(y, ks, coefs)
            combine_bound_check(out.cpu().numpy().ravel(), y.cpu().numpy().ravel(), [k.cpu().numpy().ravel() for k in ks], coefs,
                                "solve_combine")
            ShadowOps.calls.append(("combine", len(ks), tuple(coefs)))
            return out

        def scaled_norm(self, y0, y1, ks, coefs, rtol, atol):
            v = super().scaled_norm(y0, y1, ks, coefs, rtol, atol)
            check_norm(self._result, y0.cpu().numpy().ravel(), y1.cpu().numpy().ravel(), [k.cpu().numpy().ravel() for k in ks],
                       coefs, rtol, atol, "solve_norm")
            ShadowOps.calls.append(("norm", len(ks), tuple(coefs)))
            return v

    ShadowOps.calls = []
    return ShadowOps


def _field(t, y):
    return -0.8 * y + float(np.sin(3.0 * t)) + 0.3 * torch.tanh(y)


@pytest.mark.parametrize("method", ["dopri5", "bosh3", "adaptive_heun"])
@pytest.mark.parametrize("span", [(0.0, 1.0), (1.0, 0.0)], ids=["forward", "reverse"])
def test_every_state_call_of_an_analytic_solve_against_fp64(method, span):
    from uspace_amd.odeint import Stats, odeint
    Shadow = shadow_ops_class()
    y0 = torch.from_numpy(np.random.default_rng(5).standard_normal((64, 4, 32, 32)).astype(np.float32)).cuda()
    st = Stats()
    out = odeint(_field, y0, *span, method=method, ops=Shadow(y0), stats=st)
    assert torch.isfinite(out).all() and st.accepted > 0
    kinds = {(c[0], c[1]) for c in Shadow.calls}
    assert ("norm", 1) in kinds and ("norm", 2) in kinds                    # the initial-step probes
    if span[0] > span[1]:
        assert ("combine", 1, (-2.0,)) in {c[:3] for c in Shadow.calls}     # _neg
    assert ("combine", 5) in kinds                                          # the dense output at t1


def test_every_state_call_of_a_uvit_s_adaptive_decode_against_fp64():
    """U-ViT-S-deep16, B = 64, the reference's default decode (adaptive dopri5, rtol = atol = 1e-5)."""
    from uspace_amd.flow_matching import CNF
    from uspace_amd.tools.utils_uvit import get_nnet
    Shadow = shadow_ops_class()
    torch.manual_seed(1234)
    net = get_nnet("uvit", img_size=32, patch_size=2, in_chans=4, embed_dim=512, depth=16, num_heads=8, mlp_ratio=4,
                   qkv_bias=False, mlp_time_embed=False, num_classes=-1).cuda().eval()
    cnf = CNF(net)
    cnf.state_ops_factory = Shadow
    z = torch.randn(64, 4, 32, 32, generator=torch.Generator().manual_seed(7)).cuda()
    x1 = cnf.decode(z, None, dissect_name="none", edit_loc=None, solver_kwargs=dict(solver="adaptive", solver_adaptive="dopri5"))
    st = cnf.last_stats
    assert torch.isfinite(x1).all() and st.accepted > 0
    assert len([c for c in Shadow.calls if c[0] == "norm"]) == 3 + st.accepted + st.rejected
    print(f"\nU-ViT-S B=64 adaptive decode: nfe={st.nfe} accepted={st.accepted} rejected={st.rejected}, {len(Shadow.calls)} state calls")
