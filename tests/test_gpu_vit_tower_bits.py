"""The three ViT towers bit for bit: the sha256 of the raw output bytes of the calls of tests/vit_tower_cases.py against
tests/golden/vit_tower_digests.json (recorded by tests/golden/make_vit_tower_digests.py at the commit named in the file).  The
towers are run-to-run bit-equal, so host-side changes to the encoder stack, the patch front or the wrappers must leave every
digest as it is."""
import json

import pytest

from tests import vit_tower_cases as C

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
