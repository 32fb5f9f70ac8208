#!/usr/bin/env python3
"""Generate tests/golden/fid_frechet.npz by IMPORTING the reference's tools/fid_score.py (with stand-ins for the modules it
imports but calculate_frechet_distance does not use: torchvision and the reference's own tools/inception.py).  Runs only
where the reference is available; the tests read the ``.npz``.

    python tests/golden/make_fid_golden.py

  small      dims 64: two covariances of 200 random samples each, their means, the reference's distance
  singular   dims 32: singular PSD covariances whose product's square root is not finite, so the reference takes the
             eps retry; the distance it then returns
  imaginary  dims 8: an indefinite "covariance" whose product's square root has an imaginary diagonal: the reference
             raises ValueError (stored: the message's number)
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE_ROOT = os.environ.get("USPACE_REFERENCE_ROOT", "/root/reference")


def load_reference_fid():
    tv = types.ModuleType("torchvision")
    tv.transforms = types.ModuleType("torchvision.transforms")
    sys.modules.setdefault("torchvision", tv)
    sys.modules.setdefault("torchvision.transforms", tv.transforms)
    pkg = types.ModuleType("_ref_tools")
    pkg.__path__ = [os.path.join(REFERENCE_ROOT, "tools")]
    sys.modules["_ref_tools"] = pkg
    inc = types.ModuleType("_ref_tools.inception")
    inc.InceptionV3 = None
    sys.modules["_ref_tools.inception"] = inc
    spec = importlib.util.spec_from_file_location("_ref_tools.fid_score", os.path.join(REFERENCE_ROOT, "tools", "fid_score.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["_ref_tools.fid_score"] = mod
    spec.loader.exec_module(mod)
    return mod


def cases():
    rng = np.random.default_rng(2024)
    out = {}
    a = rng.standard_normal((200, 64)) @ rng.standard_normal((64, 64)) * 0.3 + 1.0
    b = rng.standard_normal((200, 64)) @ rng.standard_normal((64, 64)) * 0.25 + 1.2
    out["small"] = (a.mean(0), np.cov(a, rowvar=False), b.mean(0), np.cov(b, rowvar=False))
    u = rng.standard_normal((30, 40))
    v = rng.standard_normal((30, 40))
    s1 = np.zeros((32, 32))
    s2 = np.zeros((32, 32))
    # two rank-2 PSD blocks whose product is not diagonalisable at 0: it has no square root
    s1[:3, :3] = [[4.0, 0.0, -4.0], [0.0, 4.0, 4.0], [-4.0, 4.0, 8.0]]
    s2[:3, :3] = [[8.0, -4.0, 6.0], [-4.0, 4.0, -4.0], [6.0, -4.0, 5.0]]
    s1[3:, 3:] = np.cov(u[:29], rowvar=True)
    s2[3:, 3:] = np.cov(v[:29], rowvar=True)
    out["singular"] = (np.zeros(32), s1, np.full(32, 0.5), s2)
    q = rng.standard_normal((8, 8))
    s1 = q @ np.diag([4.0, -3.0, 2.0, -1.5, 1.0, -0.5, 0.7, -2.0]) @ q.T
    out["imaginary"] = (np.zeros(8), s1, np.ones(8), np.eye(8))
    return out


def main():
    ref = load_reference_fid()
    z = {}
    for name, (m1, s1, m2, s2) in cases().items():
        for k, v in zip(("mu1", "sigma1", "mu2", "sigma2"), (m1, s1, m2, s2)):
            z[f"{name}/{k}"] = v
        try:
            z[f"{name}/fid"] = np.float64(ref.calculate_frechet_distance(m1, s1, m2, s2))
            z[f"{name}/raises"] = np.bool_(False)
        except ValueError as e:
            z[f"{name}/fid"] = np.float64(float(str(e).split()[-1]))
            z[f"{name}/raises"] = np.bool_(True)
    np.savez_compressed(os.path.join(HERE, "fid_frechet.npz"), **z)
    print({k: z[k] for k in z if k.endswith(("/fid", "/raises"))})


if __name__ == "__main__":
    main()
