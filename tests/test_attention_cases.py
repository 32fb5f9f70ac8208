"""tests/attention_cases.py pinned on the CPU: its mirror of the attention launch dispatch against the kernels the built library
holds, the coverage of its case list, and the sensitivity of every bound of tests/test_gpu_attention_parity.py -- each faulty
reference must lie at least twice the bound away from the true one, in the metric the GPU test uses."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from tests import attention_cases as AC
from tests import uvit_stages as S
from tests.attention_cases import BRANCH_BH, FORM_BATCHES, RAGGED_L, TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTOR = 2.0


# ------------------------------------------------------------------------------------------------------------------ coverage
def test_cases_reach_every_launch_and_every_kernel():
    reached = {AC.case_launch(c) for c in AC.CASES}
    assert reached == set(AC.all_launches()) and len(reached) == 38
    forms = {AC.launch_form(*c[:4]) for c in AC.CASES}
    assert forms == AC.all_forms() and len(forms) == 36              # NT = 6: 'small' and 'two' are both QS = 2
    assert len(set(AC.CASES)) == len(AC.CASES)
    assert set(AC.REQUIRED_L) <= {c[1] for c in AC.CASES}
    assert set(AC.REQUIRED_BH_334) <= {c[0] * c[2] for c in AC.CASES if c[1] == 334 and not c[3]}
    # several heads per workgroup with a last round that is not full, for both counts
    uneven = {AC.launch_branch(*c[:4]) for c in AC.CASES if c[0] * c[2] % AC.launch_grid(*c[:4])}
    assert {"hpw2", "hpw4"} <= uneven
    assert (37, 334, 16, False) in {c[:4] for c in AC.CASES}
    # three and four rounds of the four-heads form, and L = 334 beyond it, plain and with key_scale
    rounds = {-(-c[0] * c[2] // 256) for c in AC.CASES if AC.launch_branch(*c[:4]) == "hpw4"}
    assert rounds == {3, 4}
    assert {c[3] for c in AC.CASES if c[1] == 334 and c[0] * c[2] > 1024} == {False, True}
    assert {c[4] for c in AC.CASES} == set(AC.DATA_SETS)
    # every launch with key_scale has a case with the all-zero row
    assert {AC.case_launch(c) for c in AC.CASES if c[3] and c[0] >= 2} == {l for l in AC.all_launches() if l[2]}


def test_gpu_test_batches_take_the_forms_they_are_meant_to():
    for L, batches in FORM_BATCHES.items():
        for scaled in (False, True):
            br = {AC.launch_branch(B, L, H, scaled) for B, H in batches}
            assert {"small", "two", "one"} <= br
            assert scaled or L != 334 or {"hpw2", "hpw4"} <= br
    for NT, LC, scaled, br in AC.all_launches():
        for B, H in BRANCH_BH[br]:
            assert AC.case_launch((B, RAGGED_L[(NT, LC)], H, scaled, "")) == (NT, LC, scaled, br)
    assert all(L % 16 for L in RAGGED_L.values())


def test_mirror_boundaries():
    f = AC.launch_form
    assert f(1, 96, 1, False)[:3] == (6, 0, 4) and f(1, 97, 1, False)[:3] == (10, 0, 4) and f(1, 160, 1, True)[:3] == (10, 0, 4)
    assert f(1, 161, 1, False)[:3] == (17, 0, 4) and f(1, 272, 1, False)[:3] == (17, 0, 4) and f(1, 273, 1, False)[:3] == (21, 0, 8)
    assert f(1, 257, 1, False)[:3] == (17, 257, 4) and f(1, 334, 1, False)[:3] == (21, 334, 8) and f(1, 336, 1, False)[:3] == (21, 0, 8)
    assert [f(1, L, 1, False)[4] for L in (16, 97, 257, 300)] == [2, 3, 5, 3]
    assert [AC.launch_branch(b, 334, 1, False) for b in (64, 65, 128, 129, 256, 257, 512, 513, 768, 769, 1024, 1025)] == \
        ["small", "two", "two", "one", "one", "hpw2", "hpw2", "hpw4", "hpw4", "hpw4", "hpw4", "one"]
    assert [AC.launch_branch(b, 334, 1, True) for b in (64, 65, 128, 129, 257, 513)] == ["small", "two", "two", "one", "one", "one"]
    assert AC.launch_branch(300, 257, 1, False) == "one" and AC.launch_branch(300, 300, 1, False) == "one"
    assert [AC.launch_grid(b, 334, 1, False) for b in (3, 70, 200, 257, 592, 769)] == [9, 140, 200, 129, 198, 193]
    with pytest.raises(ValueError):
        f(1, 337, 1, False)


def test_mirror_matches_the_kernels_of_the_built_library():
    """The non-causal product instantiations of attention_kernel in libuspace_hip.so (template arguments NT, LC, SCALED, NW, CAUSAL,
    QS, HPW, W4 read from the mangled names) are exactly the forms the mirror can return: a launch added to or removed from
    att_plan / att_dispatch_form without its mirror fails here."""
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"):
        pytest.skip("llvm-objdump not available")
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    pat = re.compile(r"16attention_kernelILi(\d+)ELi(\d+)ELb([01])ELi(\d+)ELb([01])ELi(\d+)ELi(\d+)ELb([01])EE")
    found = [pat.search(k["name"]) for k in kr.kernels() if "attention_kernel" in k["name"]]
    assert found and all(found)
    args = [tuple(int(x) for x in m.groups()) for m in found]
    assert sum(1 for a in args if a[4]) == 2                                              # causal: CLIP, 6 and 10 tiles
    lib = {(NT, LC, NW, bool(SC), QS, HPW) for NT, LC, SC, NW, CAUSAL, QS, HPW, W4 in args if not CAUSAL and NW != 6 and not W4}
    assert len(lib) == len([a for a in args if not a[4]]), "a lab instantiation (NW = 6 / W4) in the product library"
    assert lib == AC.all_forms(), (sorted(lib - AC.all_forms()), sorted(AC.all_forms() - lib))


# B * H on both sides of every switch of att_plan (64, 128, rounds of 256 heads up to four) and beyond
PLAN_BH = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 767, 768, 769, 1023, 1024, 1025, 1040, 2048)
USPACE_ERR_ARG = -1


def test_mirror_matches_the_plan_of_the_built_library():
    """uspace_attention_plan (the att_plan that uspace_attention_bf16 launches from; host-side, no GPU) against the mirror for every
    L the kernel takes, both key_scale settings and B * H around every switch, as B x 1 head and as B / 16 x 16 heads: kernel form and
    grid from the mirror, block and dynamic LDS bytes from the kernel's layout (K rows, V rows, key scales).  A boundary moved in
    attention.hip without its mirror fails here."""
    from uspace_amd import _hip
    plan = _hip.lib().uspace_attention_plan
    out = (ctypes.c_int * 8)()
    shapes = [(bh, 1) for bh in PLAN_BH] + [(bh // 16, 16) for bh in PLAN_BH if bh % 16 == 0]
    assert len(shapes) > len(PLAN_BH)
    seen = set()
    for L in range(1, 337):
        for scaled in (0, 1):
            for B, H in shapes:
                assert plan(B, L, H, scaled, out) == 0, (B, L, H, scaled)
                NT, LC, NW, QS, HPW, grid, block, lds = out
                where = (B, L, H, scaled, list(out))
                assert (NT, LC, NW, bool(scaled), QS, HPW) == AC.launch_form(B, L, H, scaled), where
                assert grid == AC.launch_grid(B, L, H, scaled), where
                assert block == 64 * NW, where
                assert lds == NT * 16 * 128 + -(-NT // 2) * 32 * 128 + (NT * 16 * 4 if scaled else 0) and lds <= 160 * 1024, where
                seen.add((NT, LC, NW, bool(scaled), QS, HPW))
    assert seen == AC.all_forms()
    for scaled in (0, 1):
        for B, L, H in ((1, 337, 1), (64, 337, 16), (1, 0, 1), (0, 257, 1), (0, 334, 16)):
            assert plan(B, L, H, scaled, out) == USPACE_ERR_ARG, (B, L, H, scaled)


# ------------------------------------------------------------------------------------------------------------------ data
def test_data_sets_are_what_they_say():
    n = S.cpu_threads()
    try:
        B, L, H = 2, 300, 2
        P = {}
        for d in AC.DATA_SETS:
            x = AC.make_qkv(B, L, H, d)
            assert x.dtype == torch.bfloat16 and x.shape == (B, L, 3 * H * 64)
            assert torch.equal(x, AC.make_qkv(B, L, H, d))                               # seeded
            q, k, _ = x.to(torch.float64).reshape(B, L, 3, H, 64).permute(2, 0, 3, 1, 4)
            P[d] = torch.softmax(q @ k.transpose(-1, -2) / 8.0, -1)
        assert float(P["flat"].amax(-1).max()) < 1.05 / L                                 # near-uniform
        assert float(P["sharp"].amax(-1).mean()) > 0.7
        v = AC.make_qkv(B, L, H, "voff").float().reshape(B, L, 3, H, 64)[:, :, 2]
        assert abs(float(v.mean()) - 4.0) < 0.05
        e = P["edges"].reshape(B * H, L, L)
        assert float(e[0::2, 1::3, 0].mean()) > 0.95 and float(e[0::2, 2::3, 0].mean()) > 0.95   # sink heads: key 0
        assert float(e[:, 0::6, L - 1].min()) > 0.8                                             # dominant last key
        assert 0.25 < float(e[:, 3::6, L - 1].min()) and float(e[:, 3::6, L - 1].max()) < 0.75  # half of the row
        ks = AC.make_key_scale(3, L)
        assert ks.dtype == torch.float32 and bool((ks[2] == 0).all()) and bool((ks[:2] == 40.0).any(1).all())
        assert bool((ks[:2] == 0.0).any(1).all()) and float(ks[:2].min()) == 0.0
        odd = (ks[:2] != 1.0).float().mean()
        assert 0.25 < float(odd) < 0.42
        lg = torch.log(ks[:2][(ks[:2] != 1.0) & (ks[:2] != 0.0) & (ks[:2] != 40.0)])
        assert float(lg.min()) > -2.3 and float(lg.max()) < 2.3 and float(lg.std()) > 1.0
    finally:
        torch.set_num_threads(n)


def test_perturbed_references_reduce_to_the_true_one_where_the_fault_is_void():
    x = AC.make_qkv(2, 40, 2, "workflow").to(torch.float64)
    true = S.attention(x, 2, True)
    ones = torch.ones(2, 40, dtype=torch.float64)
    assert torch.equal(AC.key_scale_shifted(x, 2, True, ones), S.attention(x, 2, True, ones))
    assert torch.equal(AC.scaled_sum_norm(x, 2, True, ones), true)
    bad = AC.tile_from_next_head(x, 2, True, tile=1, head=2).reshape(2, 40, 2, 64)
    t = true.reshape(2, 40, 2, 64)
    assert torch.equal(bad[:, :16], t[:, :16]) and torch.equal(bad[:, 32:], t[:, 32:]) and torch.equal(bad[0], t[0])
    assert torch.equal(bad[1, :, 1], t[1, :, 1]) and not torch.equal(bad[1, 16:32, 0], t[1, 16:32, 0])
    # a last key nobody looks at: masking it changes nothing beyond float64 rounding
    y = x.clone().reshape(2, 40, 3, 2, 64)
    y[:, :, 0, :, 0], y[:, :39, 1, :, 0], y[:, 39, 1, :, 0] = 8.0, 0.0, -100.0      # a logit of -100 on top of the others
    y = y.reshape(2, 40, -1)
    assert float((S.attention(y, 2, False) - AC.last_key_masked(y, 2, False)).abs().max()) < 1e-12
    assert float((S.attention(x, 2, False) - AC.last_key_masked(x, 2, False)).abs().max()) > 1e-2
    assert AC.pad_key_visible(x, 2, True).shape == true.shape and AC.last_key_masked(x, 2, True).shape == true.shape


# ------------------------------------------------------------------------------------------------------------------ sensitivity
def _distances(fault, data, L, env, with_ks):
    fn = AC.PERTURBED[fault][0]
    B, H = 3, 2
    qkv = AC.make_qkv(B, L, H, data)
    ks = AC.make_key_scale(B, L) if with_ks else None                 # the set the GPU cases use
    heads = list(range((B - 1) * H))                                  # (not the sample whose key_scale row is 0)
    out = {}
    for rnd in (True, False):
        true = AC.reference(qkv, H, heads, rnd, ks).numpy()
        bad = AC.reference(qkv, H, heads, rnd, ks, fn=fn).numpy()
        if rnd and env:
            ksh = None if ks is None else ks[torch.as_tensor(heads) // H]
            a = TOL["env_a"] * AC.envelope_a(AC.head_qkv(qkv, H, heads), ksh)
            out["envelope"] = AC.envelope_excess(bad, true, TOL["env_k"], a)          # the bound is 1
        elif rnd:
            sfx = "_ks" if with_ks else ""
            out["att_tight" + sfx] = AC.head_err(bad, true) / AC.tol("att_tight", with_ks)
            out["row_tight" + sfx] = AC.row_err(bad, true) / AC.tol("row_tight", with_ks)
        elif not env:
            out["att_loose" + ("_ks" if with_ks else "")] = AC.head_err(bad, true) / AC.tol("att_loose", with_ks)
    return out


@pytest.mark.parametrize("L", [257, 300, 334])
@pytest.mark.parametrize("fault", sorted(AC.PERTURBED))
def test_every_bound_separates_every_fault(fault, L):
    """distance(faulty reference, true reference) >= 2 x bound, per bound of TOL, in the GPU test's metric, on the data sets meant to
    expose the fault, on the key_scale set the GPU cases use; the faults that do not need key_scale are tried without and with it.
    Smallest ratio at the bounds in TOL: 4.8 (row_tight, a visible padding key, 'flat', L = 334); for the envelope 17 (the same fault,
    'edges', L = 257); see the printed lines (pytest -s)."""
    n = S.cpu_threads()
    try:
        _, needs_ks, rel_sets, env_sets, ks_sets = AC.PERTURBED[fault]
        runs = [(False, d, needs_ks) for d in rel_sets] + [(True, d, needs_ks) for d in env_sets]
        runs += [(env, d, True) for d in ks_sets for env in (False, True)]
        ratios = {}
        for env, data, with_ks in runs:
            for k, v in _distances(fault, data, L, env, with_ks).items():
                ratios[(k, data, "ks" if with_ks else "plain")] = v
        print(f"\n[sensitivity {fault} L={L}] " + " ".join(f"{k}/{d}/{w}={v:.3g}" for (k, d, w), v in sorted(ratios.items())))
        rel = {k for k in TOL if not k.startswith("env")}
        assert {k for k, _, _ in ratios} == ({k for k in rel if k.endswith("_ks")} if needs_ks else rel) | {"envelope"}
        assert min(ratios.values()) >= FACTOR, ratios
    finally:
        torch.set_num_threads(n)


def test_metrics():
    ref = np.ones((2, 32, 64))
    got = ref.copy()
    got[1, 16:32] = 2.0                                               # one 16-query tile of one head wrong by its own size
    assert AC.head_err(got, ref) == pytest.approx(np.sqrt(0.5)) and AC.row_err(got, ref) == pytest.approx(1.0)
    assert AC.envelope_excess(got, ref, 2.0, 0.0) == pytest.approx(128.0)
    assert AC.envelope_excess(ref, ref, 2.0, 0.0) == 0.0 and AC.head_err(ref * 0, ref * 0) == 0.0
    got[0, 0, 0] = np.nan
    assert AC.head_err(got, ref) == np.inf and AC.row_err(got, ref) == np.inf and AC.envelope_excess(got, ref, 2.0, 1.0) == np.inf
