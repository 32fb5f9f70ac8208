#!/usr/bin/env python3
"""Generate tests/golden/vae_anysize_tiny.npz by IMPORTING the reference (through _refshim.py, as make_vae_encoder_golden.py does).
Runs only where the reference is available; tests/test_gpu_vae_anysize.py reads the ``*.npz``.

    python tests/golden/make_vae_anysize_golden.py

The reference's FrozenAutoencoderKL at a tiny configuration with NOMINAL resolution 64 (ch=64, ch_mult (1,2), 1 res block: 32x32
latents), fed OFF-nominal sizes with the same weights: latents z [2,4,33,33] -> decode -> images [2,3,66,66], and images x [2,3,66,66]
-> encode_moments -> [2,8,33,33].  33 x 33 = 1 089 latent positions: an odd side, beyond the 1 024 tokens of the nominal SD shape.
It pins that the reference itself takes its size from the tensor.  Inputs hold fp16-exact values; the two results are stored as fp16
(2^-11 relative, thirty times below the tolerances they are compared at) to keep the fixture under 200 KB.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _refshim  # noqa: E402
from make_vae_encoder_golden import SCALE, digest, meta_bytes, reference_model, save, smooth_images  # noqa: E402

TINY = dict(double_z=True, z_channels=4, resolution=64, in_channels=3, out_ch=3, ch=64, ch_mult=[1, 2],
            num_res_blocks=1, attn_resolutions=[], dropout=0.0)
SEED = 1234 + 17
H = 33


def main():
    _refshim.install()
    import importlib
    ae = importlib.import_module("libs.autoencoder")
    torch.set_grad_enabled(False)
    model = reference_model(ae, TINY, SEED)
    g = torch.Generator().manual_seed(9)
    z16 = (torch.randn(2, 4, H, H, generator=g) * SCALE * 4.0).to(torch.float16)
    x16 = smooth_images(2, 2 * H, 6)
    img = model.decode(z16.to(torch.float32))
    moments = model.encode_moments(x16.to(torch.float32))
    assert img.shape == (2, 3, 2 * H, 2 * H) and moments.shape == (2, 8, H, H)
    keys, n, sha = digest(model)
    meta = dict(ddconfig=TINY, weight_seed=SEED, sha256=sha, n_params=n, n_keys=len(keys), scale_factor=SCALE)
    save("vae_anysize_tiny.npz", z_fp16=z16.numpy(), img_fp16=img.to(torch.float16).numpy(), x_fp16=x16.numpy(),
         moments_fp16=moments.to(torch.float16).numpy(), meta_json=meta_bytes(meta))


if __name__ == "__main__":
    main()
