#!/usr/bin/env python3
"""Records rowops_digests.json: the sha256 of every output buffer of the calls of tests/rowops_cases.py (the row and elementwise
kernels of uspace_amd/csrc/rowops.hip), each group run twice.  A call whose two runs differ is left out and listed under
``unstable``; none of these kernels uses atomics, so that list is expected empty.  Needs the GPU.  Run at the commit whose output bits
are to be pinned; the commit is written into the file.  Reads nothing outside the repository.

    make_rowops_digests.py [output directory]"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import rowops_cases as C  # noqa: E402
from tests.golden.make_blob_golden import commit, write  # noqa: E402


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else HERE
    digests, unstable = {}, []
    for case in C.CASES:
        first, second = C.case_digests(case), C.case_digests(case)
        digests[case] = {call: d for call, d in first.items() if second[call] == d}
        unstable += [f"{case}::{call}" for call, d in first.items() if second[call] != d]
        for call, d in first.items():
            print(case, call, d, "" if second[call] == d else "UNSTABLE")
    write("rowops_digests.json", dict(recorded_at_commit=commit(), run_twice_equal=not unstable, unstable=unstable, digests=digests),
          out_dir)


if __name__ == "__main__":
    main()
