#!/usr/bin/env python3
"""Records uvit_forward_digests.json: the sha256 of every output of the calls of tests/uvit_forward_cases.py (the U-ViT forward of
uspace_amd/csrc/uvit.hip in both LayerNorm modes, through the tap, the mid hook, key scales, attention maps and the paired forward),
each case run twice, and the launch recorder's table [kind, flags, M, N, K, launches] of a plain forward of every case in both modes.
A call whose two runs differ is left out and listed under ``unstable``; the forward uses no atomics whose order reaches the output,
so that list is expected empty.  Needs the GPU.  Run at the commit whose output bits are to be pinned; the commit is written into
the file.  Reads nothing outside the repository.

    make_uvit_forward_digests.py [output directory]"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import uvit_forward_cases as C  # noqa: E402
from tests.golden.make_blob_golden import commit, write  # noqa: E402


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else HERE
    digests, launches, unstable = {}, {}, []
    for case in C.CASES:
        first, second = C.case_digests(case), C.case_digests(case)
        digests[case] = {}
        for mode, calls in first.items():
            digests[case][mode] = {call: d for call, d in calls.items() if second[mode][call] == d}
            unstable += [f"{case}::{mode}::{call}" for call, d in calls.items() if second[mode][call] != d]
            for call, d in calls.items():
                print(case, mode, call, d, "" if second[mode][call] == d else "UNSTABLE")
        launches[case] = {"fold": C.launch_table(case, 1), "separate": C.launch_table(case, 0)}
        assert C.folded_rows(launches[case]["fold"]), f"{case}: the folded mode issued no USPACE_EPI_LN_IN GEMM: pick other sizes"
        assert not C.folded_rows(launches[case]["separate"])
        for mode, table in launches[case].items():
            print(case, mode, "launches", table)
    write("uvit_forward_digests.json", dict(recorded_at_commit=commit(), run_twice_equal=not unstable, unstable=unstable, digests=digests,
                                            launches=launches), out_dir)


if __name__ == "__main__":
    main()
