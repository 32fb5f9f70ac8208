#!/usr/bin/env python3
"""Generate tests/golden/dino_tiny.npz with Hugging Face ``transformers``: a tiny ``Dinov2Model`` and a tiny ``ViTModel`` (no
pooler) built OFFLINE from configs (never ``from_pretrained``), seeded parameters, and what HF computes from them in fp32 on the CPU.
Runs only where ``transformers`` is installed; the tests read the ``.npz``.

    python tests/golden/make_dino_golden.py

  dinov2  hidden 128, 2 heads, 3 layers, patch 14, position table 5 x 5 (image 70); run at 70 (26 tokens, 2 images) and at 42
          (10 tokens, 3 images, the table interpolated by HF)
  vit     hidden 128, 2 heads, 2 layers, patch 8, eps 1e-12, position table 5 x 5 (image 40); run at 24 (10 tokens, 3 images) with
          ``interpolate_pos_encoding=True``

Stored per run ``r`` in (dinov2_70, dinov2_42, vit_24): ``{r}_pixel_values``, ``{r}_embeddings``, ``{r}_hidden_states`` (every
hidden state, the embeddings first), ``{r}_pooler`` (``last_hidden_state[:, 0]``; the ``Dinov2Model``'s ``pooler_output``),
``{r}_keys`` (the last layer's keys through a forward hook on its key projection, ``...attention.attention.key``), ``{r}_pairs`` and ``{r}_structure``
(the fp64 structure distance of those image pairs from the fp32 keys).

The parameters are stored as int8 codes: value = offset + step * code with a power-of-two step per tensor (exact in fp32).  The
LayerScale factors span [0.0625, 1.5] and every bias is non-zero, so that omitting or swapping them shows."""
import json
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "dino_tiny.npz")

DINOV2 = dict(hidden_size=128, num_hidden_layers=3, num_attention_heads=2, mlp_ratio=4, patch_size=14, image_size=70,
              layer_norm_eps=1e-6, hidden_act="gelu", use_swiglu_ffn=False)
VIT = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=512, patch_size=8, image_size=40,
           layer_norm_eps=1e-12, hidden_act="gelu", qkv_bias=True)
PAIRS = {2: [[0, 1], [1, 1]], 3: [[0, 1], [1, 2], [2, 2]]}


def coded(name, shape, g):
    """(offset, step, int8 codes) of one parameter."""
    code = torch.round(torch.randn(shape, generator=g) * 1.1).clamp(-3, 3).to(torch.int8)
    if name.endswith("lambda1"):
        return 0.0625, 2.0 ** -6, torch.randint(0, 93, shape, generator=g).to(torch.int8)
    if "norm" in name and name.endswith("weight"):
        return 1.0, 2.0 ** -4, code
    if name.endswith("fc1.bias") or name.endswith("intermediate.dense.bias"):
        return -1.0, 2.0 ** -3, code                                   # the activation's negative tail carries weight
    if name.endswith("bias"):
        return 2.0 ** -5, 2.0 ** -4, code                              # never exactly zero
    if name.endswith("cls_token"):
        return 0.0, 2.0 ** -2, code
    if name.endswith("position_embeddings"):
        return 0.0, 2.0 ** -3, code
    fan_in = int(np.prod(shape[1:]))
    step = 2.0 ** round(np.log2(1.0 / (1.1 * fan_in ** 0.5)))          # weights of std about 1 / sqrt(fan_in)
    return 0.0, step, code


def structure(keys, pairs):
    k = keys.double()
    n = k.norm(dim=-1)
    s = (k @ k.transpose(1, 2)) / (n[:, :, None] * n[:, None, :]).clamp_min(1e-8)
    return np.array([float(((s[i] - s[j]) ** 2).mean()) for i, j in pairs])


def seeded(model, tag, g, arrays, skip=("mask_token",)):
    names, offs, steps, sd, i = [], [], [], {}, 0
    for name, p in model.state_dict().items():
        if name.endswith(skip):
            continue
        o, s, c = coded(name, tuple(p.shape), g)
        names.append(name), offs.append(o), steps.append(s)
        arrays[f"{tag}_param_{i}"] = c.numpy()
        sd[name] = (o + s * c.float()).to(torch.float32)
        i += 1
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.endswith(skip) for k in missing), (missing, unexpected)
    arrays[f"{tag}_param_names"] = np.array(names)
    arrays[f"{tag}_param_offset"] = np.array(offs, np.float64)
    arrays[f"{tag}_param_step"] = np.array(steps, np.float64)


def run(model, tag, side, B, g, arrays, key_module, n_layers, **kw):
    pv = torch.round(torch.randn(B, 3, side, side, generator=g) * 16) / 16          # coarse values: the file compresses
    kept = []
    hook = key_module.register_forward_hook(lambda _m, _i, o: kept.append(o.detach()))
    with torch.no_grad():
        out = model(pixel_values=pv, output_hidden_states=True, **kw)
    hook.remove()
    assert len(kept) == 1 and len(out.hidden_states) == n_layers + 1
    pooled = out.last_hidden_state[:, 0]
    if getattr(out, "pooler_output", None) is not None:
        assert torch.equal(out.pooler_output, pooled)
    pairs = PAIRS[B]
    d = structure(kept[0], pairs)
    arrays.update({f"{tag}_pixel_values": pv.numpy(), f"{tag}_embeddings": out.hidden_states[0].numpy(),
                   f"{tag}_hidden_states": torch.stack(out.hidden_states).numpy(), f"{tag}_pooler": pooled.numpy(),
                   f"{tag}_keys": kept[0].numpy(), f"{tag}_pairs": np.array(pairs), f"{tag}_structure": d})
    print(f"{tag}: tokens {kept[0].shape[1]}, structure {d}")


def main():
    from transformers import Dinov2Config, Dinov2Model, ViTConfig, ViTModel
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(20240915)
    arrays = dict(dinov2_config=json.dumps(DINOV2), vit_config=json.dumps(VIT))
    dm = Dinov2Model(Dinov2Config(**DINOV2)).eval()
    seeded(dm, "dinov2", g, arrays)
    key = dm.encoder.layer[-1].attention.attention.key
    run(dm, "dinov2_70", 70, 2, g, arrays, key, 3)
    run(dm, "dinov2_42", 42, 3, g, arrays, key, 3)
    vm = ViTModel(ViTConfig(**VIT), add_pooling_layer=False).eval()
    seeded(vm, "vit", g, arrays)
    # (the installed transformers names ViT's layers ``layers.{i}.attention.{q,k,v,o}_proj``; published files use the older
    # ``encoder.layer.{i}.attention.attention.{query,key,value}`` names: libs/dino.py maps both)
    run(vm, "vit_24", 24, 3, g, arrays, vm.layers[-1].attention.k_proj, 2, interpolate_pos_encoding=True)
    np.savez_compressed(OUT, **arrays)
    print(f"wrote {OUT}: {os.path.getsize(OUT) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
