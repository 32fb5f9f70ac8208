"""CPU-only: every planted fault of tests/uvit_stages.py::FAULTS stands clear of the bound of the test that is named for it.

plain       (``update_tight``, ``embed``, ``head``: entries of tests/test_gpu_uvit_parity.py::TOL, imported) the faulty float64 model
            lies FAULT_MARGIN bounds from the true one in that metric, measured as the GPU test measures it: blocks one by one from
            the true previous state, the worst (smallest) block the fault acts in counting.
projection  the fault moves a block by less than that.  With the tight model (its roundings on) in the GPU's place, in both tight
            modes and on every block the fault acts in, the coefficient c_f of tests/util.py::fault_projection is within
            PROJECTION_HOST of 0 without the fault and of 1 with it; the GPU test bounds |c_f| by PROJECTION_GPU, the midpoint.
            ``projection_head``: the same for the head, the decoder_pred operands split into two bf16 halves standing in for the GPU's
            hi + lo head.
unit        neither resolves it.  On the inputs, reference and bound of the unit tests UNIT_TESTS names (tests/unit_fault_cases.py,
            tests/attention_cases.py) the faulty reference lies FAULT_MARGIN bounds from the true one.

Every distance and coefficient is printed; the last test requires a passing metric for every entry of the table."""
import functools

import numpy as np
import pytest
import torch

from tests import attention_cases as AC
from tests import unit_fault_cases as U
from tests import uvit_stages as S
from tests.test_gpu_uvit_parity import TOL
from tests.util import fault_projection, rel_l2

TIGHT = ("tight_sep", "tight_fold")


@pytest.fixture(scope="module", autouse=True)
def _threads():
    n = S.cpu_threads()
    yield
    torch.set_num_threads(n)
    _case.cache_clear()


@functools.lru_cache(maxsize=None)
def _case(name):
    """One sample of one of S.FAULT_NETS (the sample the GPU test takes): the loose stages, every block's true output from the true
    previous stage, and the same from the two tight models (the fold's centring constants chained as the GPU test chains them)."""
    _net, sd, spec, hooks, B = S.fault_net(name)
    seed, rows = S.fault_case(name)
    x, t, kw = S.inputs(spec, B, hooks, seed)
    x, t, kw = x[rows], t[rows], S.select_rows(kw, rows)
    out, T = S.forward(spec, sd, x, t, "loose", **kw)
    skw = {k: kw[k] for k in ("key_scale", "mid") if k in kw}
    true = [S.step(spec, sd, T, i, "loose", **skw)[0] for i in range(spec.nblocks)]
    assert all(torch.equal(a, b) for a, b in zip(true, T[1:]))
    tight, consts = {}, {}
    for mode in TIGHT:
        c, cskip, outs, cs = None, [None] * spec.half, [], []
        for i in range(spec.nblocks):
            cs.append((c, list(cskip)))
            h, c = S.step(spec, sd, T, i, mode, c=c, cskip=cskip, **skw)
            if i < spec.half:
                cskip[i] = c
            outs.append(h)
        tight[mode], consts[mode] = outs, cs
    return dict(sd=sd, spec=spec, x=x, t=t, kw=kw, skw=skw, T=T, out=out, tight=tight, consts=consts)


def _update(a, b, prev):
    return float((a - b).norm() / (b - prev).norm())


def _split_head(spec, sd, x, fault=None):
    """The head with the decoder_pred operands (the LayerNorm output, taken from S.head's tap, and the weight) each as the sum of
    two bf16 halves: the GPU's stand-in, for the LayerNorm faults."""
    two = lambda v: v.to(torch.bfloat16).double() + (v - v.to(torch.bfloat16).double()).to(torch.bfloat16).double()
    taps = {}
    S.head(spec, sd, x, taps=taps, fault=fault)
    h = two(taps["norm"]) @ two(sd["decoder_pred.weight"].double()).T + sd["decoder_pred.bias"].double()
    h = h[:, spec.extras:]
    B, p, C = h.shape[0], spec.patch_size, spec.in_chans
    g = spec.img_size // p
    img = h.reshape(B, g, g, p, p, C).permute(0, 5, 1, 3, 2, 4).reshape(B, C, g * p, g * p)
    return torch.nn.functional.conv2d(img, sd["final_layer.weight"].double(), sd["final_layer.bias"].double(), padding=1)


# ------------------------------------------------------------------------------------------------------------------ the three kinds
def _plain(name, metric):
    """-> (passes, {net: distance})."""
    seen = {}
    for net in S.fault_nets(name):
        k = _case(net)
        sd, spec, T = k["sd"], k["spec"], k["T"]
        if metric == "update_tight":
            d = min(_update(S.step(spec, sd, T, i, "loose", fault=name, **k["skw"])[0], T[i + 1], T[i]) for i in S.fault_blocks(spec, name))
        elif metric == "embed":
            ekw = {n: k["kw"][n] for n in ("y", "context") if n in k["kw"]}
            d = rel_l2(S.embed(spec, sd, k["x"], k["t"], tight=True, fault=name, **ekw).numpy(),
                       S.embed(spec, sd, k["x"], k["t"], tight=True, **ekw).numpy())
        else:
            assert metric == "head", metric
            d = rel_l2(S.head(spec, sd, T[-1], fault=name).numpy(), k["out"].numpy())
        seen[net] = d
    return all(d > S.FAULT_MARGIN * TOL[metric] for d in seen.values()), seen


def _projection(name, metric):
    """-> (passes, {net: (c_f without the fault: lowest, highest; with it: lowest, highest)})."""
    seen = {}
    for net in S.fault_nets(name):
        k = _case(net)
        sd, spec, T = k["sd"], k["spec"], k["T"]
        c0, c1 = [], []
        if metric == "projection_head":
            ref, bad = k["out"], S.head(spec, sd, T[-1], fault=name)
            c0.append(fault_projection(_split_head(spec, sd, T[-1]), ref, bad, ref))
            c1.append(fault_projection(_split_head(spec, sd, T[-1], fault=name), ref, bad, ref))
        else:
            for i in S.fault_blocks(spec, name):
                bad = S.step(spec, sd, T, i, "loose", fault=name, **k["skw"])[0]
                for mode in TIGHT:
                    c, cskip = k["consts"][mode][i]
                    c0.append(fault_projection(k["tight"][mode][i], T[i + 1], bad, T[i + 1]))
                    got = S.step(spec, sd, T, i, mode, c=c, cskip=cskip, fault=name, **k["skw"])[0]
                    c1.append(fault_projection(got, T[i + 1], bad, T[i + 1]))
        seen[net] = (min(c0), max(c0), min(c1), max(c1))
    ok = all(max(abs(a), abs(b)) <= S.PROJECTION_HOST and max(abs(c - 1), abs(d - 1)) <= S.PROJECTION_HOST for a, b, c, d in seen.values())
    return ok, seen


def _unit(name, metric):
    """-> (passes, {unit test: the faulty reference's distance in units of that test's bound})."""
    seen = {}
    if name == "eps_1e-6":
        worst = np.inf
        for M, D in U.LAYERNORM_SHAPES:
            x, g, b = U.ln_eps_rows(64, D, seed=D + M)
            ref = U.layernorm_f64(x, g, b)
            worst = min(worst, float((np.abs(U.layernorm_f64(x, g, b, eps=1e-6) - ref) / U.ln_bf16_bound(ref)).max()))
        seen["test_layernorm"] = worst
        worst = np.inf
        for shape in U.FOLDED_EPS_CASES:
            case = U.folded_eps_case(*shape)
            y = U.folded_reference(case, case["rows"])[1]
            worst = min(worst, rel_l2(U.folded_reference(case, case["rows"], eps=1e-6)[1], y) / U.FOLDED_Y_TOL)
        seen["test_layernorm_folded_through_gemms_rows_at_eps"] = worst
    elif name == "tanh_gelu":
        worst = np.inf
        for big in (False, True):
            A, W, b, rows = U.epilogue_gelu_tail_case(big)
            ref, bound = U.gelu_tail_reference(A, W, b, rows)
            worst = min(worst, float((np.abs(U.gelu_tail_reference(A, W, b, rows, "tanh")[0] - ref) / bound).max()))
        seen["test_gemm_epilogues"] = worst
    else:
        assert name == "scale_1/sqrt65", name
        # The scale is one constant that every instantiation of the kernel shares (c_exp of attention.hip), so the cases that show it
        # best decide: the worst head against float64 with the kernel's roundings on the 'workflow' and 'edges' sets without
        # key_scale at L >= 160 (four heads of each; more heads can only raise the worst).  The other cases see it by 1 ... 4 bounds:
        # 'flat' scales the logits away, on 'sharp' a few keys carry a row whatever the scale, short rows have few keys to
        # re-weight, and under key_scale the bound is four times wider.
        bad_fn = lambda qkv, H, rnd, ks=None: S.attention(qkv, H, rnd, ks, fault=name)
        dists = []
        for B, L, H, scaled, data in AC.CASES:
            if scaled or data not in ("workflow", "edges") or L < 160:
                continue
            qkv = AC.make_qkv(B, L, H, data)
            heads = list(range(min(4, B * H)))
            d = AC.head_err(AC.reference(qkv, H, heads, True, fn=bad_fn).numpy(), AC.reference(qkv, H, heads, True).numpy())
            dists.append(d / AC.tol("att_tight", False))
        assert len(dists) >= 4, dists
        seen["test_every_head_against_float64"] = min(dists)
    assert len(seen) == len(S.UNIT_TESTS[name]) and all(any(t.endswith("::" + n) for t in S.UNIT_TESTS[name]) for n in seen)
    return all(d > S.FAULT_MARGIN for d in seen.values()), seen


@functools.lru_cache(maxsize=None)
def _measure(name):
    metric = S.FAULTS[name][0]
    kind = _projection if metric.startswith("projection") else _unit if metric == "unit" else _plain
    ok, seen = kind(name, metric)
    if name in S.UNIT_TESTS and metric != "unit":          # pinned at the block level and in the kernels' own tests
        ok2, seen2 = _unit(name, metric)
        ok, seen = ok and ok2, dict(seen, **seen2)
    return ok, seen


def _of(*metrics):
    return [f for f, (m, _what) in S.FAULTS.items() if m in metrics]


# ------------------------------------------------------------------------------------------------------------------ tests
def test_the_table_names_what_exists():
    assert S.FAULT_MARGIN == 10.0
    assert {m for m, _ in S.FAULTS.values()} <= {"update_tight", "embed", "head", "projection", "projection_head", "unit"}
    assert set(_of("unit")) <= set(S.UNIT_TESTS) <= set(S.FAULTS) and set(S.FAULT_ON) <= set(S.FAULTS)
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for tests in S.UNIT_TESTS.values():
        for t in tests:
            path, fn = t.split("::")
            assert f"def {fn}(" in open(os.path.join(root, path)).read(), t
    src = open(os.path.join(root, "tests", "test_gpu_uvit_parity.py")).read()
    assert "def test_no_planted_fault_explains_the_gpu_error(" in src
    # a fault leaves the model alone where it is not planted
    k = _case("u1024")
    assert torch.equal(S.step(k["spec"], k["sd"], k["T"], 0, "loose", fault="skip_fifo")[0], k["T"][1])


@pytest.mark.parametrize("name", _of("update_tight", "embed", "head"))
def test_plain_fault_stands_clear_of_the_gpu_bound(name):
    metric = S.FAULTS[name][0]
    ok, seen = _plain(name, metric)
    print(f"{name}: {metric} " + ", ".join(f"{n} {d:.2e}" for n, d in seen.items()) + f"  (needs {S.FAULT_MARGIN * TOL[metric]:.1e})")
    assert ok, (name, seen)


@pytest.mark.parametrize("name", _of("projection", "projection_head"))
def test_projection_fault_separates_from_the_rounding_noise(name):
    ok, seen = _measure(name)
    print(f"{name}: c_f " + ", ".join(f"{n} without [{a:+.3f}, {b:+.3f}] with [{c:+.3f}, {d:+.3f}]" for n, (a, b, c, d) in seen.items()))
    assert ok, (name, seen)


@pytest.mark.parametrize("name", list(S.UNIT_TESTS))
def test_unit_fault_is_excluded_by_its_unit_test(name):
    ok, seen = _unit(name, "unit")
    print(f"{name}: " + ", ".join(f"{n} {d:.1f} bounds" for n, d in seen.items()))
    assert ok, (name, seen)


def test_projection_faults_really_need_the_projection():
    """A projection fault that the plain bound excluded by the margin would be a plain fault; and the noise the projection has to
    see through is of the size the GPU shows (TOL's 'measured 1.8e-3')."""
    for name in _of("projection"):
        ok, seen = _plain(name, "update_tight")
        print(f"{name}: smallest update distance " + ", ".join(f"{n} {d:.2e}" for n, d in seen.items()))
        assert not ok, (name, seen)
    for net in ("u512", "t2i512", "u1024"):
        k = _case(net)
        noise = max(_update(k["tight"][m][i], k["T"][i + 1], k["T"][i]) for m in TIGHT for i in range(k["spec"].nblocks))
        print(f"{net}: tight against loose {noise:.2e}")
        assert 1e-3 < noise < TOL["update_loose"]


def test_no_fault_is_without_a_passing_metric():
    failed = {name: _measure(name)[1] for name in S.FAULTS if not _measure(name)[0]}
    print(f"{len(S.FAULTS)} faults: " + ", ".join(f"{n} -> {m}" for n, (m, _w) in S.FAULTS.items()))
    assert not failed, failed
