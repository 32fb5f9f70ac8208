"""The row and elementwise kernels of uspace_amd/csrc/rowops.hip bit for bit: the sha256 of every output buffer of the calls of
tests/rowops_cases.py against tests/golden/rowops_digests.json (recorded by tests/golden/make_rowops_digests.py at the commit named
in the file).  The kernels use no atomics and are run-to-run bit-equal, so a change that keeps the order of every sum -- sharing the
row statistics among the LayerNorm, centring and head kernels, say -- must leave every digest as it is."""
import json

import pytest

from tests import rowops_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    rec = json.load(open(C.DIGESTS))
    assert rec["run_twice_equal"] and not rec["unstable"]
    return rec["digests"]


@pytest.mark.parametrize("case", list(C.CASES))
def test_output_bytes_equal_the_recorded_digests(recorded, case):
    got = C.case_digests(case)
    assert sorted(got) == sorted(recorded[case])
    for call, d in got.items():
        print(case, call, d)
    assert got == recorded[case]
