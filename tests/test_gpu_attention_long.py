"""The long-sequence attention kernel (uspace_amd/csrc/attention_long.hip: K and V streamed in key tiles, online softmax) on its own,
on every case of tests/attention_long_cases.py, against the PLAIN float64 softmax of tests/uvit_stages.py:

A  per head: worst rel-L2 over (b, h) within the project's ``att_loose`` / ``att_loose_ks``.
B  per query row: worst rel-L2 over (b, h, query) within 3 x the row error of the streamed float64 model (ROW_MODEL, measured on the
   CPU), and the analytic element-wise envelope of attention_cases.envelope_a.
C  a sample whose key_scale row is 0 comes out exactly 0; nothing is NaN or Inf.
D  bit-equality: one sample at B = 1 and inside B = 5, two runs of one call, one head under both branches of the plan at a ragged L.
E  ``out`` inside a buffer of sentinels: fully written, nothing around it touched, under both branches of the plan.
F  at L = 17, 334 and 336 the resident kernel meets the same bounds on the same cases; L = 337 through it still returns -1.

tests/test_attention_long_cases.py shows on the CPU that each bound separates six faulty references from the true one by at least 2x.
Measured on an MI355X over the cases: attention_long_cases.GPU_MEASURED."""
import pytest
import torch

from tests import attention_cases as AC
from tests import attention_long_cases as LC
from tests import uvit_stages as S

pytestmark = pytest.mark.gpu

TOL = AC.TOL
REF_CHUNK = 32


@pytest.fixture(scope="module")
def hip():
    from uspace_amd import _hip
    _hip.lib()
    n = S.cpu_threads()
    yield _hip
    torch.set_num_threads(n)


def _gpu(fn, qkv, B, L, H, ks=None):
    out = fn(qkv.cuda().reshape(B * L, -1), B, L, H, key_scale=None if ks is None else ks.cuda())
    return out.reshape(B, L, H * 64).cpu()


_FIGURES = {}


def _measure(hip, case, kernel="long"):
    """Run one case once through ``kernel``; the figures of A, B and C over EVERY head of the batch."""
    if (case, kernel) in _FIGURES:
        return _FIGURES[(case, kernel)]
    B, L, H, scaled, data = case
    qkv = AC.make_qkv(B, L, H, data)
    ks = AC.make_key_scale(B, L) if scaled else None
    got_all = _gpu(hip.attention_long if kernel == "long" else hip.attention, qkv, B, L, H, ks)
    fig = dict(head=0.0, row=0.0, env=0.0)
    for i in range(0, B * H, REF_CHUNK):
        heads = list(range(i, min(B * H, i + REF_CHUNK)))
        got = AC.head_out(got_all, H, heads).numpy()
        plain = AC.reference(qkv, H, heads, False, ks).numpy()
        ksh = None if ks is None else ks[torch.as_tensor(heads) // H]
        a = TOL["env_a"] * AC.envelope_a(AC.head_qkv(qkv, H, heads), ksh)
        for k, v in dict(head=AC.head_err(got, plain), row=AC.row_err(got, plain),
                         env=AC.envelope_excess(got, plain, TOL["env_k"], a)).items():
            fig[k] = max(fig[k], v)
    fig.update(finite=bool(torch.isfinite(got_all.float()).all()),
               zero_row=float(got_all[B - 1].float().abs().max()) if scaled and B >= 2 else None, heads=B * H)
    print(f"\n[attention_{kernel} {AC.case_id(case)} QB={LC.plan(B, L, H, scaled)[1]}] " + " ".join(
        f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in fig.items()))
    _FIGURES[(case, kernel)] = fig
    return fig


def _check(f, scaled):
    assert f["finite"], f
    assert f["head"] <= AC.tol("att_loose", scaled), f
    assert f["env"] <= 1.0, f
    assert f["row"] <= LC.row_bound(scaled), f


# ------------------------------------------------------------------------------------------------------------------ A, B, C
@pytest.mark.parametrize("case", LC.CASES, ids=AC.case_id)
def test_every_head_and_query_row_against_float64(hip, case):
    f = _measure(hip, case)
    _check(f, case[3])
    if case[3]:
        assert f["zero_row"] == 0.0, f


# ------------------------------------------------------------------------------------------------------------------ F
@pytest.mark.parametrize("case", [c for c in LC.CASES if c[1] in LC.SHARED_L], ids=AC.case_id)
def test_resident_kernel_meets_the_same_bounds_where_both_run(hip, case):
    _check(_measure(hip, case, "resident"), case[3])
    _check(_measure(hip, case, "long"), case[3])


def test_resident_kernel_still_refuses_337_tokens(hip):
    qkv = torch.zeros(337, 192, dtype=torch.bfloat16, device="cuda")
    out = torch.empty(337, 64, dtype=torch.bfloat16, device="cuda")
    assert hip.lib().uspace_attention_bf16(hip.ptr(qkv), None, hip.ptr(out), 1, 337, 1, hip.stream_ptr()) == -1
    with pytest.raises(hip.UspaceHipError):
        hip.attention(qkv, 1, 337, 1)
    assert hip.lib().uspace_attention_long_bf16(hip.ptr(qkv), None, hip.ptr(out), 1, 337, 1, hip.stream_ptr()) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ D
@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "ks"])
def test_a_sample_is_bit_equal_alone_and_inside_a_batch_and_from_run_to_run(hip, scaled):
    L, H = 1102, 2
    g = torch.Generator().manual_seed(77 + scaled)
    qkv = (torch.randn(5, L, 3 * H * 64, generator=g) * 1.5).to(torch.bfloat16)
    ks = torch.exp((torch.rand(5, L, generator=g) * 2 - 1) * 2.3).float() if scaled else None
    qkv[3] = AC.make_qkv(1, L, H, "edges", salt=3)[0]
    whole = _gpu(hip.attention_long, qkv, 5, L, H, ks)
    again = _gpu(hip.attention_long, qkv, 5, L, H, ks)
    alone = _gpu(hip.attention_long, qkv[3:4], 1, L, H, None if ks is None else ks[3:4])
    assert torch.equal(whole.view(torch.int16), again.view(torch.int16))
    assert torch.equal(whole[3].view(torch.int16), alone[0].view(torch.int16))


RAGGED_L = 401              # 4 blocks of 128 queries: QB = 128 from B * H = 128 on


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "ks"])
def test_one_head_is_bit_equal_under_both_branches_of_the_plan(hip, scaled):
    L = RAGGED_L
    g = torch.Generator().manual_seed(4242 + scaled)
    probes = [AC.make_qkv(1, L, 1, d, salt=5)[0].reshape(L, 3, 64) for d in ("workflow", "flat", "edges")]
    pks = AC.make_key_scale(3, L, salt=5)
    pks[2] = AC.make_key_scale(1, L, salt=6)[0]                    # (row 2 of a 3-sample set is the all-zero one)
    seen, branches = {}, set()
    for B, H in ((3, 1), (1, 16), (127, 1), (128, 1), (8, 16), (9, 16)):
        branches.add(LC.plan(B, L, H, scaled)[1])
        qkv = (torch.randn(B, L, 3, H, 64, generator=g) * 1.5).to(torch.bfloat16)
        ks = torch.exp((torch.rand(B, L, generator=g) * 2 - 1) * 2.3).float() if scaled else None
        placed = []
        for i, p in enumerate(sorted({0, B * H // 2, B * H - 1})):
            b, h = divmod(p, H)
            j = b % 3 if scaled else i % 3                           # key_scale belongs to the sample: one probe per sample then
            qkv[b, :, :, h] = probes[j]
            if scaled:
                ks[b] = pks[j]
            placed.append((p, j))
        out = AC.head_out(_gpu(hip.attention_long, qkv.reshape(B, L, -1), B, L, H, ks).float(), H, [p for p, _ in placed])
        for (p, j), o in zip(placed, out):
            if j in seen:
                assert torch.equal(o, seen[j][0]), f"probe {j}: head {p} of (B, H) = {(B, H)} differs from {seen[j][1]}"
            else:
                seen[j] = (o, f"head {p} of (B, H) = {(B, H)}")
    assert len(seen) == 3 and branches == {64, 128}


# ------------------------------------------------------------------------------------------------------------------ E
SENTINEL = 0x7FA5                                                    # a bf16 NaN pattern


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "ks"])
@pytest.mark.parametrize("B,H", [(2, 3), (8, 16)], ids=["QB64", "QB128"])
def test_out_is_fully_written_and_nothing_around_it(hip, B, H, scaled):
    L = RAGGED_L
    g = torch.Generator(device="cuda").manual_seed(B + L + H)
    qkv = (torch.randn(B * L, 3 * H * 64, device="cuda", generator=g) * 1.5).to(torch.bfloat16)
    ks = torch.exp(torch.rand(B, L, device="cuda", generator=g) * 2 - 1) if scaled else None
    n, guard = B * L * H * 64, 64 * H * 64
    big = torch.full((n + 2 * guard,), SENTINEL, dtype=torch.int16, device="cuda")
    out = big[guard:guard + n].view(torch.bfloat16)
    hip.check(hip.lib().uspace_attention_long_bf16(hip.ptr(qkv), hip.ptr(ks), hip.ptr(out), B, L, H, hip.stream_ptr()),
              "uspace_attention_long_bf16")
    torch.cuda.synchronize()
    assert bool((big[:guard] == SENTINEL).all()) and bool((big[guard + n:] == SENTINEL).all())
    assert bool(torch.isfinite(out.float()).all())
    assert torch.equal(out.view(B * L, H * 64), hip.attention_long(qkv, B, L, H, key_scale=ks))
