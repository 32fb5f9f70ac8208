"""The few-keys / many-queries attention (uspace_amd/csrc/attention_kv.hip) on the GPU, alone:

A  every head and every query row of tests/attention_kv_cases.cases() against the float64 model (the bounds are the resident
   kernel's, see attention_kv_cases);
B  bit-equal to ``uspace_attention_bf16`` wherever both take a shape (Lq == Lk): a row's arithmetic is the resident kernel's;
C  a head's rows are bit-equal whatever the chunking, the batch, the head's place in it and the number of queries behind it;
D  strided rows: q, kv and out as the leading columns of wider tensors, the rest of ``out`` untouched;
E  337 keys are refused."""
import numpy as np
import pytest
import torch

from tests import attention_kv_cases as K

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", K.cases(), ids=K.case_id)
def test_every_head_and_row_against_float64(case):
    from uspace_amd import _hip
    B, Lq, Lk, H, data = case
    q, kv = K.make_q_kv(B, Lq, Lk, H, data)
    got_t = _hip.attention_kv(q.cuda(), kv.cuda(), H).cpu()
    assert got_t.shape == (B, Lq, H * 64) and bool(torch.isfinite(got_t.float()).all())
    got = K.per_head(got_t, H)
    tight, loose = (K.per_head(K.attention_kv_f64(q, kv, H, r), H) for r in (True, False))
    fig = dict(att_tight=K.head_err(got, tight), att_loose=K.head_err(got, loose), row_tight=K.row_err(got, tight))
    print(f"\nATTKV-MEASURE {K.case_id(case)} plan {_hip.attention_kv_plan(B, Lq, Lk, H)}: "
          + " ".join(f"{k}={v:.3e} (bound {K.TOL[k]:.1e})" for k, v in fig.items()))
    for k, v in fig.items():
        assert v < K.TOL[k], (k, v)


@pytest.mark.parametrize("L,H,B", [(1, 1, 1), (15, 2, 3), (17, 3, 2), (96, 5, 2), (160, 8, 1), (256, 2, 3), (272, 1, 2), (300, 3, 1),
                                   (335, 2, 2), (336, 8, 1), (257, 2, 2), (334, 1, 3)])
def test_bit_equal_to_the_resident_kernel_at_equal_lengths(L, H, B):
    from uspace_amd import _hip
    g = torch.Generator().manual_seed(100 * L + H)
    qkv = (torch.randn(B, L, 3, H * 64, generator=g) * 1.5).to(torch.bfloat16).cuda()
    want = _hip.attention(qkv.reshape(B * L, 3 * H * 64), B, L, H).reshape(B, L, H * 64)
    got = _hip.attention_kv(qkv[:, :, 0].contiguous(), qkv[:, :, 1:].reshape(B, L, 2 * H * 64).contiguous(), H)
    assert torch.equal(got, want)


@pytest.mark.parametrize("Lk", [12, 256, 336])
def test_rows_do_not_depend_on_chunking_batch_or_position(Lk):
    """One head's q and k | v placed in batches whose plans differ (chunks of 4 .. 64 tiles, 1 .. 15 chunks per head, 4- and 8-wave
    workgroups), at different (sample, head) positions, with more or fewer queries behind the probe's: the probe's rows keep their
    bits.  (A prefix of the queries changes n_qt and with it the chunk boundaries.)"""
    from uspace_amd import _hip
    Lq = 960
    pq, pkv = K.make_q_kv(1, Lq, Lk, 1, "workflow", salt=9)
    seen, plans = None, set()
    for B, H, pos, nq in ((1, 1, 0, Lq), (3, 8, 13, Lq), (2, 5, 9, 825), (40, 8, 319, Lq), (1, 2, 1, 17), (3, 3, 4, 100)):
        g = torch.Generator().manual_seed(B * 10 + H)
        q = (torch.randn(B, nq, H, 64, generator=g) * 1.5).to(torch.bfloat16)
        kv = (torch.randn(B, Lk, 2, H, 64, generator=g) * 1.5).to(torch.bfloat16)
        b, h = divmod(pos, H)
        q[b, :, h] = pq[0, :nq]
        kv[b, :, :, h] = pkv[0].reshape(Lk, 2, 64)
        out = _hip.attention_kv(q.reshape(B, nq, H * 64).cuda(), kv.reshape(B, Lk, 2 * H * 64).cuda(), H)
        rows = out.reshape(B, nq, H, 64)[b, :, h].cpu()
        p = _hip.attention_kv_plan(B, nq, Lk, H)
        plans.add((p["chunk"], p["nchunks"]))
        if seen is None:
            seen = rows
        assert torch.equal(rows, seen[:nq]), (B, H, pos, nq, p)
    assert len(plans) >= 4, plans


def test_strided_rows_and_untouched_columns():
    from uspace_amd import _hip
    B, Lq, Lk, H = 2, 100, 37, 3
    q, kv = K.make_q_kv(B, Lq, Lk, H, "workflow")
    want = _hip.attention_kv(q.cuda(), kv.cuda(), H)
    qw = torch.full((B, Lq, H * 64 + 8), float("nan"), dtype=torch.bfloat16, device="cuda")
    kw = torch.full((B, Lk, 2 * H * 64 + 16), float("nan"), dtype=torch.bfloat16, device="cuda")
    qw[..., :H * 64], kw[..., :2 * H * 64] = q.cuda(), kv.cuda()
    out = torch.full((B, Lq, H * 64 + 4), 7.0, dtype=torch.bfloat16, device="cuda")
    _hip.attention_kv(qw, kw, H, out=out)
    assert torch.equal(out[..., :H * 64], want) and bool((out[..., H * 64:] == 7.0).all())


def test_more_than_336_keys_are_refused():
    from uspace_amd import _hip
    q = torch.zeros(1, 16, 64, dtype=torch.bfloat16, device="cuda")
    kv = torch.zeros(1, 337, 128, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(_hip.UspaceHipError, match="USPACE_ERR_ARG"):
        _hip.attention_kv(q, kv, 1)
    with pytest.raises(_hip.UspaceHipError):
        _hip.attention_kv_plan(1, 16, 337, 1)
    with pytest.raises(_hip.UspaceHipError):
        _hip.attention_kv(q.float(), kv[:, :336].contiguous(), 1)
