"""The wide single-head attention kernel (uspace_amd/csrc/attention_wide.hip) on the GPU against float64 softmax(q k^T scale) v on the
same bf16 operands: every case of tests/attention_wide_cases.py, with ld > C and NaN in the padding, canary rows behind ``out``, and
the bit-equalities the kernel promises -- an image alone against the same image inside a batch, every branch of the plan, two runs.
Bounds and their derivation: tests/attention_wide_cases.py."""
import pytest
import torch

from tests import attention_wide_cases as WC

pytestmark = pytest.mark.gpu

run = WC.run             # ld = C + 16 with NaN padding, canaries behind ``out``: shared with tests/attention_stream_cases.py


def _threads():
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 16))
    return n


_WORST = {}


@pytest.mark.parametrize("case", WC.CASES, ids=WC.case_id)
def test_against_float64_softmax(case):
    """rel-L2 and max |err| / max_j |v_j| against the plain float64 softmax, under 3 x what an MI355X measured for the width
    (WC.GPU_MEASURED; printed here: pytest -s) and, whatever was measured, under the analytic ceiling 2^-8 max_j |v_j|."""
    B, N, C, data, nrows = case
    n = _threads()
    try:
        q, k, v, scale = WC.make_qkv(B, N, C, data)
        rows = WC.sample_rows(N, nrows) if nrows else None
        ref, peak = WC.reference(q, k, v, B, N, C, scale, rows)
        got = run(q, k, v, B, N, C, scale).to(torch.float64).reshape(B, N, C)
        assert bool(torch.isfinite(got).all())
        if rows is not None:
            got = got[:, rows]
        rel, ma = WC.rel_l2(got, ref), WC.max_abs(got, ref, v, B, N, C)
        w = _WORST.setdefault(C, [0.0, 0.0])
        w[0], w[1] = max(w[0], rel), max(w[1], ma)
        print(f"\n[wide {WC.case_id(case)}] rel={rel:.3e} maxabs={ma:.3e} peak={float(peak.max()):.3f} | worst C={C}: "
              f"rel={w[0]:.3e} maxabs={w[1]:.3e}")
        assert N == 1 or float(peak.median()) > 0.3
        # measured on an MI355X, worst per width C = 64 / 128 / 256 / 512: rel 1.692e-3 / 1.725e-3 / 1.675e-3 / 1.664e-3 -> bounds (3 x)
        # 5.08e-3 / 5.18e-3 / 5.03e-3 / 4.99e-3; maxabs 3.334e-3 / 3.380e-3 / 3.473e-3 / 3.500e-3 -> bound 2^-8 = 3.906e-3, the ceiling
        # (3 x would lie above it).  WC.GPU_MEASURED holds them; profiles/vae_anysize.md lists the cases.
        b_rel, b_ma = WC.bounds(C)
        assert ma <= WC.CEILING, (rel, ma)
        assert rel <= b_rel and ma <= b_ma, (rel, ma, b_rel, b_ma)
    finally:
        torch.set_num_threads(n)


@pytest.mark.parametrize("C", WC.WIDTHS)
def test_constant_v_is_returned_bit_for_bit(C):
    """The 'constv' set: every V row of an image is u, so the answer is u exactly iff P.V and the row sum use the same rounded P
    (WC.make_qkv, WC bounds: the one bound that is 0)."""
    B, N = 3, 65
    q, k, v, scale = WC.make_qkv(B, N, C, "constv")
    assert torch.equal(run(q, k, v, B, N, C, scale), v)


@pytest.mark.parametrize("C", WC.WIDTHS)
def test_rows_do_not_depend_on_batch_plan_branch_or_run(C):
    """N = 129 (nine 16-query tiles, the last with one query; five key tiles, the last with one key).  Image b alone == image b inside
    B = 3; the same three images repeated to the batch sizes that take 2 and 4 waves per workgroup == B = 3 (one wave); tight
    operands (ld = C) == padded ones; a second run == the first."""
    N = 129
    q, k, v, scale = WC.make_qkv(3, N, C, "last")
    base = run(q, k, v, 3, N, C, scale)
    assert WC.plan(3, N, C)[2] == 1
    assert torch.equal(run(q, k, v, 3, N, C, scale), base)
    assert torch.equal(run(q, k, v, 3, N, C, scale, pad=0), base)
    for b in range(3):
        sl = slice(b * N, (b + 1) * N)
        assert torch.equal(run(q[sl], k[sl], v[sl], 1, N, C, scale), base[sl]), b
    for nw, B in ((2, WC.branch_batches(N)[2]), (4, WC.branch_batches(N)[4])):
        assert WC.plan(B, N, C)[2] == nw
        rep = lambda x: x.reshape(3, N, C).repeat(-(-B // 3), 1, 1)[:B].reshape(B * N, C).contiguous()
        got = run(rep(q), rep(k), rep(v), B, N, C, scale)
        assert torch.equal(got[: 3 * N], base), nw
        assert torch.equal(got[(B - 1) * N:], base[((B - 1) % 3) * N: ((B - 1) % 3 + 1) * N]), nw
