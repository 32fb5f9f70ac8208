"""The non-causal attention kernel (uspace_amd/csrc/attention.hip) on its own, on every launch form the host dispatch can take
(tests/attention_cases.py: 38 launches = 36 kernels), against the float64 attention of tests/uvit_stages.py.

A  per head: the worst rel-L2 over (b, h) against the reference that rounds where the kernel rounds (``att_tight``) and against the
   plain float64 softmax (``att_loose``).  A global norm dilutes one wrong head by the whole batch; this does not.
B  per query row: the worst rel-L2 over (b, h, query) against the tight reference (``row_tight``), and an element-wise envelope
   |got - tight| <= 2 x 2^-8 |tight| + a  with the analytic, per-element a of attention_cases.envelope_a.
C  the same head's data placed at different positions of batches that take different forms (ceil(NT / NW) or two workgroups per
   head, one workgroup per head, two / four heads per workgroup, first / middle / last workgroup round) gives the same bits, with
   and without key_scale: every form runs the same per-tile arithmetic over the whole K and V.
D  ``out`` as a view inside a buffer of sentinel NaN patterns with 64-row guards: guards untouched, ``out`` fully written, on
   every launch at a ragged L.
E  a sample whose whole key_scale row is 0 comes out exactly 0.

The GPU runs whole batches and the float64 references run on every head of every case (1040 heads at L = 334 take a few seconds on
16 threads).  tests/test_attention_cases.py shows on the CPU that each bound below separates the true reference from five faulty ones by at least 2x.

Bounds (attention_cases.TOL) are 3x the worst value an MI355X measured over all cases, or analytic where that is tighter."""
import pytest
import torch

from tests import attention_cases as AC
from tests import uvit_stages as S

pytestmark = pytest.mark.gpu

TOL = AC.TOL
REF_CHUNK = 48              # heads per float64 call (the score matrix of 48 heads at L = 334 is 43 MB)


@pytest.fixture(scope="module")
def hip():
    from uspace_amd import _hip
    _hip.lib()
    n = S.cpu_threads()
    yield _hip
    torch.set_num_threads(n)


def _gpu(hip, qkv, B, L, H, ks=None):
    out = hip.attention(qkv.cuda().reshape(B * L, -1), B, L, H, key_scale=None if ks is None else ks.cuda())
    return out.reshape(B, L, H * 64).cpu()


_FIGURES = {}


def _measure(hip, case):
    """Run one case once; the figures of A, B and E over EVERY head of the batch (the float64 references in chunks of heads)."""
    if case in _FIGURES:
        return _FIGURES[case]
    B, L, H, scaled, data = case
    qkv = AC.make_qkv(B, L, H, data)
    ks = AC.make_key_scale(B, L) if scaled else None
    got_all = _gpu(hip, qkv, B, L, H, ks)
    fig = dict(att_tight=0.0, att_loose=0.0, row_tight=0.0, env=0.0)
    for i in range(0, B * H, REF_CHUNK):
        heads = list(range(i, min(B * H, i + REF_CHUNK)))
        got = AC.head_out(got_all, H, heads).numpy()
        tight = AC.reference(qkv, H, heads, True, ks).numpy()
        loose = AC.reference(qkv, H, heads, False, ks).numpy()
        ksh = None if ks is None else ks[torch.as_tensor(heads) // H]
        a = TOL["env_a"] * AC.envelope_a(AC.head_qkv(qkv, H, heads), ksh)
        for k, v in dict(att_tight=AC.head_err(got, tight), att_loose=AC.head_err(got, loose), row_tight=AC.row_err(got, tight),
                         env=AC.envelope_excess(got, tight, TOL["env_k"], a)).items():
            fig[k] = max(fig[k], v)
    fig.update(finite=bool(torch.isfinite(got_all.float()).all()),
               zero_row=float(got_all[B - 1].float().abs().max()) if scaled and B >= 2 else None, heads=B * H)
    print(f"\n[attention {AC.case_id(case)} {AC.case_launch(case)}] " + " ".join(
        f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in fig.items()))
    _FIGURES[case] = fig
    return fig


# ------------------------------------------------------------------------------------------------------------------ A
@pytest.mark.parametrize("case", AC.CASES, ids=AC.case_id)
def test_every_head_against_float64(hip, case):
    f = _measure(hip, case)
    assert f["finite"]
    assert f["att_tight"] < AC.tol("att_tight", case[3]) and f["att_loose"] < AC.tol("att_loose", case[3]), f


# ------------------------------------------------------------------------------------------------------------------ B
@pytest.mark.parametrize("case", AC.CASES, ids=AC.case_id)
def test_every_query_row_against_float64(hip, case):
    f = _measure(hip, case)
    assert f["row_tight"] < AC.tol("row_tight", case[3]) and f["env"] <= 1.0, f


# ------------------------------------------------------------------------------------------------------------------ C
# (B, H) per form: attention_cases.FORM_BATCHES; the probe heads sit at the first, middle and last head and around every workgroup-round
# boundary
FORM_BATCHES = AC.FORM_BATCHES


def _positions(B, L, H, scaled):
    BH = B * H
    grid = AC.launch_grid(B, L, H, scaled) if AC.launch_branch(B, L, H, scaled) in ("hpw2", "hpw4") else BH
    pos = {0, BH // 2, BH - 1}
    for r in range(1, -(-BH // grid)):
        pos.update((r * grid - 1, r * grid, min(BH - 1, r * grid + 1)))
    return sorted(pos)


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "ks"])
@pytest.mark.parametrize("L", sorted(FORM_BATCHES))
def test_one_head_is_bit_equal_across_forms_and_positions(hip, L, scaled):
    g = torch.Generator().manual_seed(4242 + L)
    probes = [AC.make_qkv(1, L, 1, d, salt=5)[0].reshape(L, 3, 64) for d in ("workflow", "flat", "edges")]
    pks = AC.make_key_scale(3, L, salt=5)
    pks[2] = AC.make_key_scale(1, L, salt=6)[0]                    # (row 2 of a 3-sample set is the all-zero one)
    seen = {}
    for B, H in FORM_BATCHES[L]:
        qkv = (torch.randn(B, L, 3, H, 64, generator=g) * 1.5).to(torch.bfloat16)
        ks = None
        if scaled:
            ks = torch.exp((torch.rand(B, L, generator=g) * 2 - 1) * 2.3).float()
        placed = []
        for i, p in enumerate(_positions(B, L, H, scaled)):
            b, h = divmod(p, H)
            j = b % 3 if scaled else i % 3                           # key_scale belongs to the sample: one probe per sample then
            qkv[b, :, :, h] = probes[j]
            if scaled:
                ks[b] = pks[j]
            placed.append((p, j))
        out = AC.head_out(_gpu(hip, qkv.reshape(B, L, -1), B, L, H, ks).float(), H, [p for p, _ in placed])
        for (p, j), o in zip(placed, out):
            if j in seen:
                assert torch.equal(o, seen[j][0]), (f"L={L} probe {j}: head {p} of (B, H) = {(B, H)} {AC.launch_form(B, L, H, scaled)} "
                                                    f"differs from {seen[j][1]}")
            else:
                seen[j] = (o, f"head {p} of (B, H) = {(B, H)}")
    assert len(seen) == 3
    nbranch = {AC.launch_branch(B, L, H, scaled) for B, H in FORM_BATCHES[L]}
    assert {"small", "two", "one"} <= nbranch and (scaled or L != 334 or {"hpw2", "hpw4"} <= nbranch)


# ------------------------------------------------------------------------------------------------------------------ D
RAGGED_L, BRANCH_BH = AC.RAGGED_L, AC.BRANCH_BH
SENTINEL = 0x7FA5                                                    # a bf16 NaN pattern


@pytest.mark.parametrize("launch", AC.all_launches() + [(21, 334, False, "beyond"), (21, 334, True, "beyond")], ids=str)
def test_out_is_fully_written_and_nothing_around_it(hip, launch):
    NT, LC, scaled, br = launch
    L = RAGGED_L[(NT, LC)]
    for B, H in ([(65, 16)] if br == "beyond" else BRANCH_BH[br]):
        assert AC.case_launch((B, L, H, scaled, "")) == (NT, LC, scaled, "one" if br == "beyond" else br)
        g = torch.Generator(device="cuda").manual_seed(B + L + H)
        qkv = (torch.randn(B * L, 3 * H * 64, device="cuda", generator=g) * 1.5).to(torch.bfloat16)
        ks = torch.exp(torch.rand(B, L, device="cuda", generator=g) * 2 - 1) if scaled else None
        n, guard = B * L * H * 64, 64 * H * 64
        big = torch.full((n + 2 * guard,), SENTINEL, dtype=torch.int16, device="cuda")
        out = big[guard:guard + n].view(torch.bfloat16)
        hip.check(hip.lib().uspace_attention_bf16(hip.ptr(qkv), hip.ptr(ks), hip.ptr(out), B, L, H, hip.stream_ptr()),
                  "uspace_attention_bf16")
        torch.cuda.synchronize()
        assert bool((big[:guard] == SENTINEL).all()) and bool((big[guard + n:] == SENTINEL).all()), (launch, B, H)
        assert bool(torch.isfinite(out.float()).all()), (launch, B, H)
        assert torch.equal(out.view(B * L, H * 64), hip.attention(qkv, B, L, H, key_scale=ks)), (launch, B, H)


# ------------------------------------------------------------------------------------------------------------------ E
@pytest.mark.parametrize("case", [c for c in AC.CASES if c[3] and c[0] >= 2], ids=AC.case_id)
def test_zero_key_scale_row_gives_exactly_zero(hip, case):
    f = _measure(hip, case)
    assert f["finite"] and f["zero_row"] == 0.0, f
