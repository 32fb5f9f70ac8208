"""tests/gemm_cases.py pinned on the CPU: every case launches the form it is listed under (the host planner of the built library
answers), the case list covers every form, role, epilogue and layout, the float32 stand-in passes every check of
tests/test_gpu_gemm_parity.py through the same guarded windows, and every perturbed stand-in fails one."""
import ctypes

import numpy as np
import pytest

from tests import gemm_cases as GC
from tests.gemm_cases import B_, C_, F_, G_, H_, L_, R_, CASES, PERTURBED, STANDIN_CASES


@pytest.fixture(scope="module")
def lib():
    from uspace_amd import _hip
    return _hip.lib()


# ------------------------------------------------------------------------------------------------------------------ planner
@pytest.mark.parametrize("c", CASES, ids=GC.case_id)
def test_case_launches_the_form_it_is_listed_under(lib, c):
    p = GC.plan_of(lib, c)
    M, N, K = c.M, c.N, GC.full_k(c)
    ex = dict(c.expect)
    assert p[0] == c.form, p
    assert M % p[2] != 0                                               # ragged rows everywhere
    if "strip" in ex:
        assert (p[6] > 0) == ex["strip"], p
    if "per_round" in ex:
        assert p[7] == ex["per_round"], p
    if "split_rows" in ex:
        assert p[1] == ex["split_rows"] and 0 < p[1] < M, p
    if "tiles" in ex:                                                  # form 2 as dispatched: too many tiles for the 64x64 form
        assert -(-M // 128) * -(-N // 128) >= ex["tiles"] > 160
    sk = lib.uspace_gemm_sk_ws_bytes(M, N, K)
    if c.form == 6:
        assert p[1] == ex["S"] and sk > 0, p
        if "n_dp" in ex:
            assert p[7] == ex["n_dp"], p
    else:
        assert sk == 0 or c.role in ("consumer", "slabs")              # (asked without a role: a size for epilogues that take the tail)
    split = lib.uspace_gemm_split_ws_bytes(M, N, K)
    if "ksplit" in ex:
        assert GC.is_producer(c) and N > 512 and split == ex["ksplit"] * M * N * 4
    elif GC.is_producer(c):
        assert p[0] != 2 or split == 0                                 # no other producer case takes the two-kernel split
    if GC.is_producer(c):
        assert lib.uspace_gemm_part_slots_k(M, N, K) == p[5] == -(-N // p[3])
    g = GC.geometry(c, p, split if "ksplit" in ex else 0)
    assert g["finish"] == ("ksplit" in ex) and g["S"] == ex.get("S", ex.get("ksplit", 1))


def test_case_list_covers_every_form_role_epilogue_and_layout():
    assert len(set(CASES)) == len(CASES)
    what = {c.what for c in CASES}
    assert set(GC.REQUIRED) <= what, set(GC.REQUIRED) - what
    by = lambda pred: {c.form for c in CASES if pred(c)}
    assert by(lambda c: c.role == "producer") >= {0, 1, 2, 4, 5, 6}
    assert by(lambda c: c.role == "consumer") == {0, 1, 2, 3, 4, 5}
    assert by(lambda c: c.role == "plain") == {0, 1, 2, 3, 4, 5, 6}
    assert {dict(c.expect).get("per_round") for c in CASES if c.role == "consumer" and c.form == 5} == {512, 1024}
    assert {dict(c.expect).get("S") for c in CASES if c.form == 6} == {2, 3, 4}
    assert any(c.form == 6 and dict(c.expect).get("n_dp", 0) > 0 for c in CASES)
    assert {c.role for c in CASES if "ksplit" in dict(c.expect)} == {"producer", "two-slab-producer"}
    assert any(c.role == "slabs" for c in CASES) and len(GC.SLAB_SHIFTS) == 9 and sum(s != 0 for s in GC.SLAB_SHIFTS) == 8
    # every epilogue dispatch_flags accepts, on every form its role reaches
    assert len(set(GC.PLAIN_FLAGS)) == 8 and len(set(GC.PRODUCER_FLAGS)) == 4 and len(set(GC.CONSUMER_FLAGS)) == 2
    assert set(GC.SK_PLAIN_FLAGS) < set(GC.PLAIN_FLAGS)
    for c in CASES:
        assert {f for f, _ in GC.launches(c)} == set(GC.case_flags(c))
        assert all(GC.layout_applies(l, f) for f, l in GC.launches(c))
    # every layout on every form, the in-place and the separate residual on every form with a residual epilogue
    for form in range(7):
        lays = {l for c in CASES if c.form == form for _, l in GC.launches(c)}
        assert lays == set(GC.LAYOUTS), (form, lays)
        res = {l in ("a", "c") for c in CASES if c.form == form for f, l in GC.launches(c) if f & R_}
        assert res == {True, False}, form
    # the finish kernel with the residual in place and in its own buffer, with and without the raw bf16 copy
    fin = {(f, l in ("a", "c")) for c in CASES if "ksplit" in dict(c.expect) for f, l in GC.launches(c) if f & R_}
    assert fin == {(f, ip) for f in (C_ | B_ | R_ | F_, C_ | B_ | R_ | F_ | H_) for ip in (True, False)}


def test_layouts_are_what_they_are_named():
    for N in (64, 132, 260, 516, 640, 3072):
        pad, col0 = GC.bf16_layout("b", N)
        assert (N + pad) % 8 == 0 and col0 == 0 and pad > 0
        pad, col0 = GC.bf16_layout("c", N)
        assert (N + pad) % 8 == 4 and col0 == 0 and pad > 0
        pad, col0 = GC.bf16_layout("d", N)
        w = GC.Win("bf16", 3, N, pad=pad, col0=col0)
        assert w.ld % 8 == 0 and (w.off * 2) % 16 == 8 and pad > 0
    c, g = STANDIN_CASES[0]
    d = GC.make_data(c, "lattice")
    for lay in GC.LAYOUTS:
        o = GC.build_ops(c, B_ | R_ | F_ | H_, lay, d, g)
        assert o.w["A"].ld % 8 == 0 and o.w["W"].ld % 8 == 0 and all(o.w[k].ld % 4 == 0 for k in ("out_f32", "out_bf16"))
        assert (o.resid == "out_f32") == (lay in ("a", "c"))
        if o.resid == "resid":
            assert o.w["resid"].ld != o.w["out_f32"].ld
        assert (o.w["A"].ld == c.K) == (lay == "a")
        assert all(w.guard >= 272 for w in o.w.values() if w.rows > 1)


# ------------------------------------------------------------------------------------------------------------------ preconditions
@pytest.mark.parametrize("c", [c for c in CASES if GC.is_producer(c)], ids=GC.case_id)
def test_lattice_data_is_exact_for_every_producer(lib, c):
    """reference asserts, on float64 alone, that every sum a producer forms on lattice data stays an integer below 2^24."""
    p = GC.plan_of(lib, c)
    g = GC.geometry(c, p, lib.uspace_gemm_split_ws_bytes(c.M, c.N, c.K) if "ksplit" in dict(c.expect) else 0)
    rows = GC.sample_rows(c, g, dict(c.expect).get("n_dp", 0))
    R = GC.reference(c, GC.make_data(c, "lattice"), GC.PRODUCER_FLAGS[-1], g, rows)
    assert R["exact"] and np.array_equal(R["part"], np.rint(R["part"]))


# ------------------------------------------------------------------------------------------------------------------ stand-ins
_PRODUCTS = {}      # (case, data set) -> the float64 matrix products of the reference, computed once and left unchanged


def run_standin(c, g, dataset, flags, layout, fault=None):
    d = GC.make_data(c, dataset)
    o = GC.build_ops(c, flags, layout, d, g)
    GC.standin(o, fault)
    return o, GC.check(o, GC.reference(c, d, flags, g, cache=_PRODUCTS.setdefault((c, dataset), {})))


@pytest.mark.parametrize("dataset", GC.DATA_SETS)
@pytest.mark.parametrize("i", range(len(STANDIN_CASES)), ids=[c.role for c, _ in STANDIN_CASES])
def test_standin_passes_every_check(i, dataset):
    """No bound is tighter than fp32 arithmetic done right, no exactness precondition fails, every layout is stored through correctly."""
    c, g = STANDIN_CASES[i]
    seen = set()
    for flags, layout in GC.launches(c):
        o, (fails, worst) = run_standin(c, g, dataset, flags, layout)
        assert not fails, (GC.flag_name(flags), layout, fails)
        assert all(not w.untouched() for n, w in o.w.items() if n.startswith("out") or n in ("part_out", "c_out"))
        seen.add(flags)
    assert seen == set(GC.case_flags(c))
    assert {f for c, _ in STANDIN_CASES for f in GC.case_flags(c)} == set(GC.PLAIN_FLAGS + GC.PRODUCER_FLAGS + GC.CONSUMER_FLAGS)


# which launches a fault shows in: (case, geometry, flags, layout) -> bool
APPLIES = dict(
    out_stride_n=lambda c, g, f, l: bool(f & F_) and l in ("b", "d"),
    resid_ld_f32=lambda c, g, f, l: bool(f & R_) and l in ("b", "d", "e"),
    a2_through_a=lambda c, g, f, l: c.role.startswith("two-slab"),
    drop_k_tile=lambda c, g, f, l: True,
    strip_wrong_part=lambda c, g, f, l: g["S"] > 1 and g["m_main"] < c.M,
    bf16_trunc=lambda c, g, f, l: bool(f & B_) and bool(f & (H_ | C_)),
    bf16_before_resid=lambda c, g, f, l: f & (R_ | H_) == R_ | H_,
    slot_neighbour=lambda c, g, f, l: bool(f & C_) and g["slots"] > 1 and not g["finish"],
    part_in_no_offset=lambda c, g, f, l: bool(f & L_) and g["split_rows"] > 0,
    store_past_n=lambda c, g, f, l: True,
    bias_after_gelu=lambda c, g, f, l: bool(f & G_),
    rstd_neighbour=lambda c, g, f, l: bool(f & L_),
)


@pytest.mark.parametrize("fault", sorted(PERTURBED))
def test_every_perturbed_standin_fails_a_check(fault):
    """A kernel with this fault would not pass tests/test_gpu_gemm_parity.py: on every launch the fault shows in, on each data set."""
    assert set(APPLIES) == set(PERTURBED)
    for dataset in PERTURBED[fault][1]:
        n = 0
        for c, g in STANDIN_CASES:
            if fault == "bf16_trunc" and GC.is_producer(c) and c.K >= 1024:
                continue            # (this producer keeps lattice values below 256, where bf16 holds every integer: nothing to round)
            for flags, layout in GC.launches(c):
                if not APPLIES[fault](c, g, flags, layout):
                    continue
                _, (fails, _) = run_standin(c, g, dataset, flags, layout, fault)
                assert fails, (fault, dataset, c.role, GC.flag_name(flags), layout)
                n += 1
        assert n > 0, (fault, dataset)


def test_guarded_windows_see_what_they_must():
    w = GC.Win("f32", 5, 8, pad=4)
    assert w.strays() == 0 and w.untouched() and np.isnan(w.get()).all()
    w.put(np.arange(40).reshape(5, 8))
    assert w.strays() == 0 and not w.untouched() and w.get()[4, 7] == 39.0
    w.flat()[w.off + 8] = 0                                            # one pad column
    assert w.strays() == 1
    w.flat()[w.off - w.ld] = np.uint32(GC.CANARY_F32 ^ 1)              # one bit of one guard row
    assert w.strays() == 2
    h = GC.Win("bf16", 2, 4, pad=4, col0=4)
    assert np.isnan(h.get()).all() and h.off == 272 * 12 + 4
    x = np.array([1.0, 1.00390625, 1.01171875, -3.0e38], np.float32)   # ties to even, both ways
    assert GC.bf16_value(GC.bf16_bits(x)).tolist()[:3] == [1.0, 1.0, 1.015625] and GC.bf16_value(GC.bf16_trunc_bits(x))[2] == 1.0078125
