#!/usr/bin/env python3
"""Writes tests/golden/segformer_tiny.npz: ``transformers``' own SegformerForSemanticSegmentation, a tiny configuration
(tests/segformer_cases.TINY, 6 labels) with the weights of ``segformer_cases.seeded_state``, run in float64 on the CPU on two
100 x 132 images.  The file holds the key names and shapes of the model's state dict, every epsilon the modules hold, the sha256
of the images (``segformer_cases.images`` regenerates them), the logits in float64 and the four encoder hidden states rounded to
float32 -- in float64 they alone are 1.5 MB and new fixtures are kept under 1 MiB; the logits, which depend on every one of them,
carry the check at float64 rounding.  No weights: the tests regenerate them from the shared recipe.

    python tests/golden/make_segformer_golden.py        (needs transformers; nothing is downloaded)"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import segformer_cases as C  # noqa: E402


def main():
    from transformers import SegformerConfig, SegformerForSemanticSegmentation
    from uspace_amd.libs.resnet import IMAGENET_MEAN, IMAGENET_STD
    cfg = SegformerConfig(**{k: list(v) if isinstance(v, tuple) else v for k, v in C.TINY.items()}, num_labels=6)
    model = SegformerForSemanticSegmentation(cfg).eval()
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict(C.seeded_state(shapes))
    model = model.double()
    eps = {n: float(m.eps) for n, m in model.named_modules() if isinstance(m, (torch.nn.LayerNorm, torch.nn.BatchNorm2d))}
    x = C.images(2, *C.GOLDEN_SIZE)
    m, s = (torch.tensor(v, dtype=torch.float64).view(1, 3, 1, 1) for v in (IMAGENET_MEAN, IMAGENET_STD))
    with torch.no_grad():
        out = model(pixel_values=(x.double() - m) / s, output_hidden_states=True)
    keys = sorted(shapes)
    np.savez_compressed(
        C.GOLDEN, keys=np.array(keys), shapes=np.array([",".join(str(d) for d in shapes[k]) for k in keys]),
        eps_names=np.array(sorted(eps)), eps_values=np.array([eps[k] for k in sorted(eps)]), images_sha256=np.array(C.sha256(x.numpy())),
        logits=out.logits.numpy(), **{f"hidden_{i}": h.numpy().astype(np.float32) for i, h in enumerate(out.hidden_states)})
    print(f"wrote {C.GOLDEN}: {os.path.getsize(C.GOLDEN)} bytes, {len(keys)} keys, logits {tuple(out.logits.shape)}")


if __name__ == "__main__":
    main()
