"""The two streaming attention kernels (attention_long.hip, attention_wide.hip) bit for bit: the sha256 of the raw output bytes of
the calls of tests/attention_stream_cases.py against tests/golden/attention_stream_digests.json (recorded by
tests/golden/make_attention_stream_digests.py at the commit named in the file).  Both kernels are run-to-run bit-equal, so a change
that keeps the key-tile sizes and the order of every accumulation -- a merge of the two into one kernel, say -- must leave every digest
as it is."""
import json

import pytest

from tests import attention_stream_cases as C

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
