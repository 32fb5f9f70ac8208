"""CPU-only: every planted fault of tests/clip_stages.py::FAULTS stands clear of the bound of the test that is named for it, in the
three kinds of tests/test_uvit_faults_host.py: plain (FAULT_MARGIN bounds of tests/test_gpu_clip_parity.py::TOL, imported, layers one
by one from the true previous state), projection (c_f of tests/util.py::fault_projection within PROJECTION_HOST of 0 without and of 1
with the fault, the tight model in the GPU's place) and unit (FAULT_MARGIN bounds on the inputs of the named unit test).

The model: CLIP-L width (768 / 12 heads), two layers of the workflow parameters -- the first two layers of the GPU test's own model
(same seed) -- and prompts of ragged length: the empty prompt, one that fills the context and two between."""
import functools

import numpy as np
import pytest
import torch

from tests import clip_stages as S
from tests import unit_fault_cases as U
from tests.test_gpu_clip_parity import TOL
from tests.util import fault_projection, rel_l2

LAYERS = 2


@pytest.fixture(scope="module", autouse=True)
def _threads():
    n = S.cpu_threads()
    yield
    torch.set_num_threads(n)
    _case.cache_clear()


@functools.lru_cache(maxsize=None)
def _case(kind="workflow"):
    sd = S.clip_params(kind, seed=101, **dict(S.CLIP_L, num_hidden_layers=LAYERS))
    n, seed, rows = S.FAULT_IDS
    ids = S.prompt_ids(n, seed=seed)[list(rows)]
    lengths = (ids != S.EOS).sum(1).tolist()
    assert len(set(lengths)) == len(lengths) and min(lengths) == 1 and max(lengths) == 76, lengths      # ragged
    out, T = S.forward(ids, sd, "loose")
    tight = [S.layer(T[i], sd, i, "tight") for i in range(LAYERS)]
    return sd, T, out, tight


def _plain(name, metric):
    sd, T, out, _tight = _case()
    if name == "eps_1e-6":          # layer 0 of the tiny set, whose rows have a variance of the order of eps; layer 0 grows them
        sd, T, out, _tight = _case("tiny")
        assert float(T[0].var(-1).max()) < 1e-5
        d = float((S.layer(T[0], sd, 0, "loose", fault=name) - T[1]).norm() / (T[1] - T[0]).norm())
    elif metric == "final_ln":
        d = rel_l2(S.final_norm(T[-1], sd, fault=name).numpy(), out.numpy())
    else:
        assert metric == "update_tight", metric
        d = min(float((S.layer(T[i], sd, i, "loose", fault=name) - T[i + 1]).norm() / (T[i + 1] - T[i]).norm()) for i in range(LAYERS))
    return d > S.FAULT_MARGIN * TOL[metric], d


def _projection(name, _metric):
    sd, T, _out, tight = _case()
    c0, c1 = [], []
    for i in range(LAYERS):
        bad = S.layer(T[i], sd, i, "loose", fault=name)
        c0.append(fault_projection(tight[i], T[i + 1], bad, T[i + 1]))
        c1.append(fault_projection(S.layer(T[i], sd, i, "tight", fault=name), T[i + 1], bad, T[i + 1]))
    ok = max(abs(c) for c in c0) <= S.PROJECTION_HOST and max(abs(c - 1) for c in c1) <= S.PROJECTION_HOST
    return ok, (min(c0), max(c0), min(c1), max(c1))


def _unit(name, _metric):
    """test_layernorm_kernels_at_d768's rows at eps, in its own units (the element's fp32 noise scale) over its bound."""
    assert name == "eps_1e-6" and S.UNIT_TESTS[name] == ("tests/test_gpu_clip_parity.py::test_layernorm_kernels_at_d768",)
    worst = np.inf
    for M in U.CLIP_LAYERNORM_M:
        x, g, b = U.ln_eps_rows(64, 768, seed=1100 + M)
        ref = U.layernorm_f64(x, g, b)
        d = np.abs(U.layernorm_f64(x, g, b, eps=1e-6) - ref)
        ulp = np.exp2(np.floor(np.log2(np.maximum(np.abs(ref), 2.0 ** -126))) - 7)        # the bf16 output is given one ulp besides
        worst = min(worst, float((np.maximum(d - ulp, 0.0) / U.ln_noise_scale(x, g, b)).max()) / TOL["ln_err"])
    return worst > S.FAULT_MARGIN, worst


@functools.lru_cache(maxsize=None)
def _measure(name):
    metric = S.FAULTS[name][0]
    ok, seen = (_projection if metric == "projection" else _plain)(name, metric)
    if name in S.UNIT_TESTS:                   # pinned at the layer level and in the kernels' own test
        ok2, seen2 = _unit(name, metric)
        ok, seen = ok and ok2, (seen, seen2)
    return ok, seen


def _of(*metrics):
    return [f for f, (m, _what) in S.FAULTS.items() if m in metrics]


def test_the_table_names_what_exists():
    import os
    assert S.FAULT_MARGIN == 10.0 and set(S.UNIT_TESTS) <= set(S.FAULTS)
    assert {m for m, _ in S.FAULTS.values()} == {"update_tight", "final_ln", "projection"}
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_clip_parity.py")).read()
    for fn in ("test_layernorm_kernels_at_d768", "test_no_planted_fault_explains_the_gpu_error", "test_layer_0_normalises_rows_at_eps"):
        assert f"def {fn}(" in src, fn


@pytest.mark.parametrize("name", _of("update_tight", "final_ln"))
def test_plain_fault_stands_clear_of_the_gpu_bound(name):
    metric = S.FAULTS[name][0]
    ok, d = _plain(name, metric)
    print(f"{name}: {metric} {d:.2e}  (needs {S.FAULT_MARGIN * TOL[metric]:.1e})")
    assert ok, (name, d)


@pytest.mark.parametrize("name", _of("projection"))
def test_projection_fault_separates_from_the_rounding_noise(name):
    ok, (a, b, c, d) = _projection(name, "projection")
    far = _plain(name, "update_tight")
    print(f"{name}: c_f without [{a:+.3f}, {b:+.3f}] with [{c:+.3f}, {d:+.3f}]; smallest update distance {far[1]:.2e}")
    assert ok, (name, a, b, c, d)
    assert not far[0], (name, far)                  # else it would be a plain fault


@pytest.mark.parametrize("name", list(S.UNIT_TESTS))
def test_unit_fault_is_excluded_by_its_unit_test(name):
    ok, d = _unit(name, "unit")
    print(f"{name}: {S.UNIT_TESTS[name][0]} {d:.3g} bounds")
    assert ok, (name, d)


def test_mask_faults_need_ragged_prompts():
    """With the mask one diagonal too wide a query reads the token behind it: prompts that differ only in length then differ where they
    should not."""
    sd, T, _out, _tight = _case()
    x = T[0][:1, :40]
    a = S.layer(x, sd, 0, "loose", fault="mask_allows_next_token")
    b = S.layer(x[:, :20], sd, 0, "loose", fault="mask_allows_next_token")
    far = lambda u, v: float((u - v).abs().max())
    assert far(S.layer(x, sd, 0, "loose")[:, :20], S.layer(x[:, :20], sd, 0, "loose")) < 1e-10
    assert far(a[:, :19], b[:, :19]) < 1e-10 and far(a[:, 19], b[:, 19]) > 1e-3


def test_no_fault_is_without_a_passing_metric():
    failed = {name: _measure(name)[1] for name in S.FAULTS if not _measure(name)[0]}
    print(f"{len(S.FAULTS)} faults: " + ", ".join(f"{n} -> {m}" for n, (m, _w) in S.FAULTS.items()))
    assert not failed, failed
