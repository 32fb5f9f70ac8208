#!/usr/bin/env python3
"""Records gemm_epilogue_digests.json: the sha256 of every output (fp32, bf16, the centred copy, the partial sums, c_out) of the
launches of tests/gemm_epilogue_cases.py -- seven product flag sets on the two-stage 256 x 256 form of the bf16 GEMM, with and without
remainder strips, one and two rounds of tiles, 2 and 64 K tiles.  Needs the GPU.  Run at the commit whose output bits are to be
pinned; the commit is written into the file.  Reads nothing outside the repository.

    make_gemm_epilogue_digests.py [output directory]"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import gemm_epilogue_cases as E  # noqa: E402
from tests.golden.make_blob_golden import commit, write  # noqa: E402


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else HERE
    digests = {}
    for p in E.PARAMS:
        res = E.run(p)
        for layout, r in res.items():
            assert not r["fails"], (E.param_id(p), layout, r["fails"])
            print(E.param_id(p), layout, r["digests"], flush=True)
        digests[E.param_id(p)] = {layout: r["digests"] for layout, r in res.items()}
    E.make_data.cache_clear()
    write("gemm_epilogue_digests.json", dict(recorded_at_commit=commit(), shapes=[list(s) for s in E.SHAPES], k=list(E.KS),
                                             digests=digests), out_dir)


if __name__ == "__main__":
    main()
