"""The epilogue of the two-stage 256 x 256 GEMM form leaves the bits it left before its store forms changed (uspace_amd/csrc/gemm.hip,
EPI_FORM_*; profiles/epilogue_forms.md): the launches of tests/gemm_epilogue_cases.py -- seven product flag sets, with and without
remainder strips, one and two rounds of tiles, 2 and 64 K tiles -- reproduce the sha256 of every output recorded in
tests/golden/gemm_epilogue_digests.json with tests/golden/make_gemm_epilogue_digests.py at the commit named in that file, the one
before the change.  Every output sits inside a NaN-canary allocation with guard rows: a line-pair exchange that writes a wrong row,
or runs past N, changes a canary or leaves one in the window.  The digests pin the arithmetic as this toolchain compiles it; re-record
them with a toolchain that contracts the epilogue's multiply-adds differently."""
import json
import os

import pytest

from tests import gemm_epilogue_cases as E

pytestmark = pytest.mark.gpu

GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_epilogue_digests.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN_FILE) as f:
        g = json.load(f)
    assert [tuple(s) for s in g["shapes"]] == list(E.SHAPES) and tuple(g["k"]) == E.KS
    yield g["digests"]
    E.make_data.cache_clear()        # the last shape's operands: not kept for the rest of the session


@pytest.mark.parametrize("p", E.PARAMS, ids=E.param_id)
def test_epilogue_outputs_are_the_recorded_bits(golden, p):
    want = golden[E.param_id(p)]
    res = E.run(p)
    assert sorted(res) == sorted(want)
    for layout, r in res.items():
        assert not r["fails"], (layout, r["fails"])
        for name, digest in r["digests"].items():
            print(E.param_id(p), layout, name, digest)
        assert r["digests"] == want[layout], (layout, [n for n in r["digests"] if r["digests"][n] != want[layout].get(n)])
