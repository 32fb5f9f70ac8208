#!/usr/bin/env python3
"""Generate tests/golden/resnet_tiny.npz with Hugging Face ``transformers``: two tiny ``ResNetForImageClassification`` models built
OFFLINE from configs (never ``from_pretrained``), coded parameters, and what HF computes from them in float64 on the CPU.  Runs
only where ``transformers`` is installed; the tests read the ``.npz``.

    python tests/golden/make_resnet_golden.py

  bottleneck  embedding_size 16, hidden_sizes (64, 128, 192, 256), depths (2, 1, 1, 1)
  basic       embedding_size 16, hidden_sizes (16, 32, 48, 64), depths (1, 2, 1, 1)

both with ``downsample_in_first_stage=False``, ``downsample_in_bottleneck=False`` (the stride on the 3 x 3), ``hidden_act="relu"``,
``num_labels=40``.  Stored per model ``m``: ``{m}_config`` (JSON), the parameters and buffers under TORCHVISION key names
(``{m}_keys`` JSON in state-dict order; ``{m}_w{i}_code`` int8, ``{m}_w{i}_affine`` = (offset, step): value = offset + step * code
with a power-of-two step, exact in fp32; ``num_batches_tracked`` as ``{m}_w{i}_int``), ``{m}_hidden_states_{0..4}``, ``{m}_pooled``,
``{m}_logits`` (float64).  Shared: ``images`` (3 images of 40 x 56 in [0, 1], multiples of 1 / 255 in fp32: non-square, with odd
sides further down), ``mean``, ``std``; HF was fed ``(images - mean) / std`` in float64.  The batch-norm statistics and affine
terms are spread away from (0, 1), and every bias is non-zero, so that omitting one shows."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
OUT = os.path.join(HERE, "resnet_tiny.npz")

COMMON = dict(num_channels=3, embedding_size=16, hidden_act="relu", downsample_in_first_stage=False, downsample_in_bottleneck=False,
              num_labels=40)
MODELS = {"bottleneck": dict(layer_type="bottleneck", hidden_sizes=[64, 128, 192, 256], depths=[2, 1, 1, 1]),
          "basic": dict(layer_type="basic", hidden_sizes=[16, 32, 48, 64], depths=[1, 2, 1, 1])}
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def coded(key, t, g):
    """(offset, step, int8 codes) of one tensor, by its torchvision key."""
    code = torch.round(torch.randn(t.shape, generator=g) * 1.1).clamp(-3, 3).to(torch.int8)
    if key.endswith("running_var"):
        return 1.0, 2.0 ** -3, code                                    # 0.625 .. 1.375
    if key.endswith("running_mean"):
        return 2.0 ** -5, 2.0 ** -3, code
    if t.dim() == 1 and key.endswith("weight"):                        # a batch norm's
        return 1.0, 2.0 ** -3, code
    if key.endswith("bias"):
        return 2.0 ** -5, 2.0 ** -4, code                              # never exactly zero
    fan_in = t[0].numel()
    return 0.0, 2.0 ** round(np.log2((2.0 / fan_in) ** 0.5 / 1.1)), code


def main():
    from transformers import ResNetConfig, ResNetForImageClassification

    from uspace_amd.libs.resnet import hf_key
    g = torch.Generator().manual_seed(20261021)
    out = {"mean": np.asarray(MEAN, np.float64), "std": np.asarray(STD, np.float64)}
    images = torch.randint(0, 256, (3, 3, 40, 56), generator=g).float() / 255
    smooth = torch.nn.functional.interpolate(torch.rand(3, 3, 5, 7, generator=g), size=(40, 56), mode="bilinear")
    images = torch.round((0.7 * smooth + 0.3 * images) * 255).clamp(0, 255) / 255
    out["images"] = images.numpy().astype(np.float32)
    pixel = (images.double() - torch.tensor(MEAN, dtype=torch.float64).view(1, 3, 1, 1)) / torch.tensor(STD, dtype=torch.float64).view(1, 3, 1, 1)
    for name, kw in MODELS.items():
        cfg = ResNetConfig(**COMMON, **kw)
        model = ResNetForImageClassification(cfg).double().eval()
        sd = model.state_dict()
        keys = []
        for i, (k, v) in enumerate(sd.items()):
            tv = hf_key(k)
            keys.append(tv)
            if tv.endswith("num_batches_tracked"):
                out[f"{name}_w{i}_int"] = np.asarray(7, np.int64)
                v.fill_(7)
                continue
            off, step, code = coded(tv, v, g)
            out[f"{name}_w{i}_code"] = code.numpy()
            out[f"{name}_w{i}_affine"] = np.asarray([off, step], np.float64)
            v.copy_(off + step * code.double())
        model.load_state_dict(sd)
        with torch.no_grad():
            res = model(pixel_values=pixel, output_hidden_states=True)
            pooled = model.resnet(pixel_values=pixel).pooler_output
        assert len(res.hidden_states) == 5
        for s, h in enumerate(res.hidden_states):
            out[f"{name}_hidden_states_{s}"] = h.numpy()
        out[f"{name}_pooled"] = pooled.flatten(1).numpy()
        out[f"{name}_logits"] = res.logits.numpy()
        out[f"{name}_keys"] = np.asarray(json.dumps(keys))
        out[f"{name}_config"] = np.asarray(json.dumps(dict(COMMON, **kw)))
        print(name, len(keys), "tensors; logits", float(res.logits.abs().mean()), [tuple(h.shape) for h in res.hidden_states])
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")
    assert os.path.getsize(OUT) <= 1_000_000


if __name__ == "__main__":
    main()
