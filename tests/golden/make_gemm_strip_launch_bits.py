#!/usr/bin/env python3
"""Record tests/golden/gemm_strip_launch_bits.npz: sha256 of every output window of every launch of tests/test_gpu_gemm_roles.py, as
the library in use computes them (needs the GPU).  The committed file was recorded from commit 4323b82, the commit before the role
bodies of the 256 x 256 form, built as a second library and named by USPACE_HIP_LIB:
    USPACE_HIP_LIB=<that build>/libuspace_hip.so python tests/golden/make_gemm_strip_launch_bits.py [out.npz]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import test_gpu_gemm_roles as T      # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN_FILE
    rec, bad = {}, 0
    for p in T.PARAMS:
        for layout, r in T.outcome(p).items():
            rec[T.golden_key(p, layout)] = r["digest"]
            if r["fails"] or r["unequal"]:
                bad += 1
                print(T.golden_key(p, layout), r["fails"], r["unequal"])
    np.savez(out, **rec)
    print(f"{len(rec)} launches recorded in {out}; {bad} of them fail the checks of the test on this library")


if __name__ == "__main__":
    main()
