"""Adaptive-solver guards without a GPU: a field or a state that stops being finite, and a dt that stops moving t, end the
solve with an error at once -- in the product's control loop (uspace_amd/odeint.py) and in the oracle (oracle/odeint_oracle.py)
alike, as torchdiffeq's published _adaptive_step does ("underflow in dt", "non-finite values in state").  Before these guards a
NaN error ratio made every rejection grow dt tenfold (min(10, max(0.9 / nan, 0.2)) is 10) until max_num_steps, about 600 000
network evaluations at the default limit, and an infinite one shrank dt forever."""
import numpy as np
import pytest

from oracle import odeint_oracle as OO

METHODS = ("dopri5", "bosh3", "adaptive_heun")


class KernelOps:
    """numpy state arithmetic with the error-norm semantics of uspace_ode_error_norm: a non-finite y0[i] or y1[i] makes that
    element's ratio NaN (tests/test_gpu_ode_state.py checks the kernel for it)."""

    def prepare(self, y):
        return np.asarray(y, np.float32)

    def combine(self, y, ks, coefs):
        out = np.asarray(y, np.float32).copy()
        with np.errstate(invalid="ignore", over="ignore"):
            for k, c in zip(ks, coefs):
                out += np.float32(c) * k
        return out

    def scaled_norm(self, y0, y1, ks, coefs, rtol, atol):
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            err = np.zeros_like(y0)
            for k, c in zip(ks, coefs):
                err += np.float32(c) * k
            a0, a1 = np.abs(y0), np.abs(y1)
            r = err / (np.float32(atol) + np.float32(rtol) * np.fmax(a0, a1))
            r = np.where(np.isfinite(a0) & np.isfinite(a1), r, np.float32(np.nan))
            return float(np.sqrt(np.mean(np.square(r), dtype=np.float32)))


class Watched:
    """dy/dt = -0.8 y + sin(3t) + 0.3 tanh(y); past t = 0.5 one element of the derivative turns ``bad`` (NaN or Inf).

    Records the solver's rejection count at the first evaluation that returns or receives a non-finite value, and stops a
    solver that keeps going long after it (the loop before the guards would otherwise spin to its step limit)."""

    def __init__(self, bad, rejected):
        self.bad, self.rejected = bad, rejected
        self.nfe = 0
        self.first = None                  # (evaluation index, rejections so far) at the first non-finite evaluation

    def __call__(self, t, y):
        self.nfe += 1
        f = (-0.8 * y + np.float32(np.sin(3.0 * t)) + 0.3 * np.tanh(y)).astype(np.float32)
        if self.bad is not None and t > 0.5:
            f.reshape(-1)[5] = self.bad
        if self.first is None and not (np.isfinite(f).all() and np.isfinite(y).all()):
            self.first = (self.nfe, self.rejected())
        if self.first is not None:
            assert self.nfe - self.first[0] < 100, "the solver kept stepping after the state stopped being finite"
        return f


def _y0(nan_state=False):
    y0 = np.random.default_rng(2).standard_normal((2, 4, 4, 4)).astype(np.float32)
    if nan_state:
        y0[1, 2, 3, 0] = np.nan
    return y0


CASES = [("nan_past_half", np.nan, False), ("inf_past_half", np.inf, False), ("neg_inf_past_half", -np.inf, False),
         ("nan_initial_state", None, True)]


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("case,bad,nan_state", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("span", [(0.0, 1.0), (1.0, 0.0)], ids=["forward", "reverse"])
def test_product_solver_stops_on_a_non_finite_state(method, case, bad, nan_state, span):
    from uspace_amd.odeint import Stats, odeint
    st = Stats()
    f = Watched(bad, lambda: st.rejected)
    with pytest.raises(RuntimeError, match="non-finite values in state"):
        odeint(f, _y0(nan_state), *span, method=method, ops=KernelOps(), stats=st, max_num_steps=2000)
    assert f.first is not None
    assert st.rejected - f.first[1] <= 2, (st.rejected, f.first)
    assert st.nfe == f.nfe


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("case,bad,nan_state", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("span", [(0.0, 1.0), (1.0, 0.0)], ids=["forward", "reverse"])
def test_oracle_solver_stops_on_a_non_finite_state(method, case, bad, nan_state, span):
    cnt = {}
    f = Watched(bad, lambda: cnt.get("rejected", 0))
    with pytest.raises(RuntimeError, match="non-finite values in state"):
        OO.solve(f, _y0(nan_state), *span, method=method, counters=cnt)
    assert f.first is not None
    assert cnt.get("rejected", 0) - f.first[1] <= 2, (cnt, f.first)


def test_both_solvers_stop_at_the_same_evaluation():
    """The oracle and the product loop walk the same attempts up to the failing one (the equality tests of finite fields hold
    unchanged in test_host_logic.py)."""
    from uspace_amd.odeint import Stats, odeint
    for method in METHODS:
        st, cnt = Stats(), {}
        fp, fo = Watched(np.nan, lambda: st.rejected), Watched(np.nan, lambda: cnt.get("rejected", 0))
        with pytest.raises(RuntimeError):
            odeint(fp, _y0(), 0.0, 1.0, method=method, ops=KernelOps(), stats=st)
        with pytest.raises(RuntimeError):
            OO.solve(fo, _y0(), 0.0, 1.0, method=method, counters=cnt)
        assert (st.nfe, st.accepted, st.rejected) == (cnt["nfe"], cnt["accepted"], cnt["rejected"]), method
        assert st.accepted > 0                               # the solve got past 0.5 with accepted steps first


class _Rejecting(KernelOps):
    """Every attempt is rejected with a finite ratio: dt shrinks by DFACTOR per attempt until t + dt == t."""

    def scaled_norm(self, y0, y1, ks, coefs, rtol, atol):
        if len(ks) == 1 or (len(coefs) == 2 and coefs == [1.0, -1.0]):      # the initial-step probes
            return super().scaled_norm(y0, y1, ks, coefs, rtol, atol)
        return 1e3


@pytest.mark.parametrize("span", [(0.3, 1.0), (1.0, 0.3)])
def test_product_solver_stops_when_dt_underflows(span):
    from uspace_amd.odeint import Stats, odeint
    st = Stats()
    f = Watched(None, lambda: st.rejected)
    with pytest.raises(RuntimeError, match="underflow in dt"):
        odeint(f, _y0(), *span, method="dopri5", ops=_Rejecting(), stats=st, max_num_steps=2000)
    assert st.accepted == 0 and 20 < st.rejected < 60        # 0.2 per attempt from dt ~ 1e-2 down to ulp(0.3) ~ 5.6e-17


def test_finite_fields_are_untouched_by_the_guards():
    """The guards never fire on a finite solve and change no step: same NFE and end state as the oracle."""
    from uspace_amd.odeint import Stats, odeint
    for method in METHODS:
        st, cnt = Stats(), {}
        got = odeint(Watched(None, lambda: 0), _y0(), 0.0, 1.0, method=method, ops=KernelOps(), stats=st)
        ref = OO.solve(Watched(None, lambda: 0), _y0(), 0.0, 1.0, method=method, counters=cnt)
        np.testing.assert_allclose(got, ref, rtol=2e-5, atol=2e-6)
        assert (st.nfe, st.accepted, st.rejected) == (cnt["nfe"], cnt["accepted"], cnt["rejected"])


def test_state_wrappers_refuse_mismatched_operands_without_a_gpu():
    """ctypes zero-fills an array built from fewer values than its length: a coefficient list shorter than the operand list would
    drop terms silently, and a scratch smaller than the norm's 1024 partials would be written past its end."""
    import torch
    from uspace_amd import _hip
    y = torch.zeros(8)
    with pytest.raises(_hip.UspaceHipError, match="coefficients"):
        _hip.ode_combine(torch.empty_like(y), y, [y, y], [1.0])
    with pytest.raises(_hip.UspaceHipError, match="coefficients"):
        _hip.ode_error_norm(y, y, [y], [1.0, 2.0], 1e-5, 1e-5, torch.empty(1024), torch.empty(2))
    with pytest.raises(_hip.UspaceHipError, match="scratch"):
        _hip.ode_error_norm(y, y, [y], [1.0], 1e-5, 1e-5, torch.empty(1023), torch.empty(2))
