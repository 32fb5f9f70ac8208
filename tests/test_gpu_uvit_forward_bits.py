"""The host sequence of a U-ViT forward (uspace_amd/csrc/uvit.hip) bit for bit, in both LayerNorm modes: the sha256 of every output
of the calls of tests/uvit_forward_cases.py, and the launch recorder's table of a plain forward, against
tests/golden/uvit_forward_digests.json (recorded by tests/golden/make_uvit_forward_digests.py at the commit named in the file).  The
folded run must really take the folded path at these sizes: its table holds GEMMs with USPACE_EPI_LN_IN, the separate mode's none."""
import json

import pytest

from tests import uvit_forward_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    rec = json.load(open(C.DIGESTS))
    assert rec["run_twice_equal"] and not rec["unstable"]
    return rec


@pytest.mark.parametrize("case", C.CASES)
def test_output_bytes_equal_the_recorded_digests(recorded, case):
    got = C.case_digests(case)
    want = recorded["digests"][case]
    for mode, calls in got.items():
        assert sorted(calls) == sorted(want[mode])
        for call, d in calls.items():
            print(case, mode, call, d)
    assert got == want


@pytest.mark.parametrize("case", C.CASES)
def test_launches_equal_the_recorded_table(recorded, case):
    fold, separate = C.launch_table(case, 1), C.launch_table(case, 0)
    print(case, "fold", fold)
    print(case, "separate", separate)
    assert C.folded_rows(fold) and not C.folded_rows(separate)
    assert {"fold": fold, "separate": separate} == recorded["launches"][case]
