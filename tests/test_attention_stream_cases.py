"""tests/attention_stream_cases.py pinned on the CPU: the calls whose output bytes tests/test_gpu_attention_stream_bits.py compares
cover both streaming attention kernels and every branch of both of their plans."""
from tests import attention_long_cases as LC
from tests import attention_stream_cases as SC
from tests import attention_wide_cases as WC


def test_digested_calls_cover_both_forms_and_every_branch_of_both_plans():
    assert set(SC.CASES) == {"long", "wide"}
    assert {LC.plan(B, L, H, False)[1] for B, H, L in SC.LONG_CALLS} == {64, 128}
    assert {(B, H, L): LC.plan(B, L, H, True)[1] for B, H, L in SC.LONG_QB} == SC.LONG_QB
    lengths = {L for _, _, L in SC.LONG_CALLS}
    assert {1, LC.KT + 1, LC.RESIDENT_MAX_L + 1, 401, 1102} <= lengths and -(-1102 // LC.KT) == 18 and 401 % LC.KT and 401 % 128
    wide = SC.wide_calls()
    assert len(set(wide)) == len(wide)
    assert {C for _, N, C in wide if N == SC.N_WIDE} == set(WC.WIDTHS) and {(1, 512), (WC.KT + 1, 512)} <= {(N, C) for _, N, C in wide}
    for C in (64, 512):
        assert {WC.plan(B, N, C_)[2] for B, N, C_ in wide if C_ == C} == {1, 2, 4}
