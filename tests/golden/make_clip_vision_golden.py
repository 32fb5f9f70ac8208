#!/usr/bin/env python3
"""Generate tests/golden/clip_vision_tiny.npz with Hugging Face ``transformers``: a tiny ``CLIPModel`` built OFFLINE from a config
(never ``from_pretrained``), seeded parameters, and what HF computes from them in fp32 on the CPU.  Runs only where
``transformers`` is installed; the tests read the ``.npz``.

    python tests/golden/make_clip_vision_golden.py

  vision  hidden 128, 2 heads, 2 layers, ffn 512, image 56, patch 14 (17 tokens)
  text    vocab 1000, hidden 128, 2 heads, 2 layers, 77 positions; projection_dim 64; quick_gelu; eos_token_id 2 (the legacy
          config of the openai checkpoints: the pooled row is ``input_ids.argmax(-1)``)

Stored: both configs (json), the state dict, ``pixel_values`` [3, 3, 56, 56], the vision tower's embeddings (before
pre_layrnorm) and every hidden state, ``pooler_output``, ``image_embeds``, ``input_ids``, ``text_embeds`` and the 3 x 3 cosine matrix.

The parameters are stored as int8 codes: value = offset + step * code with a power-of-two step per tensor (exact in fp32), codes
from a clipped normal -- 1.0 M parameters in a few hundred KB instead of 4 MB."""
import json
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "clip_vision_tiny.npz")

VISION = dict(hidden_size=128, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, image_size=56, patch_size=14,
              hidden_act="quick_gelu", layer_norm_eps=1e-5)
TEXT = dict(vocab_size=1000, hidden_size=128, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2,
            max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5, eos_token_id=2, bos_token_id=0, pad_token_id=1)
PROJ = 64
BOS, EOS = 998, 999


def coded(name, shape, g):
    """(offset, step, int8 codes) of one parameter."""
    code = torch.round(torch.randn(shape, generator=g) * 1.1).clamp(-3, 3).to(torch.int8)
    if name == "logit_scale":
        return float(np.log(1 / 0.07)), 0.0, torch.zeros(shape, dtype=torch.int8)
    if "norm" in name and name.endswith("weight"):
        return 1.0, 2.0 ** -4, code
    if name.endswith("bias"):
        return 0.0, 2.0 ** -4, code
    if name.endswith(("token_embedding.weight", "class_embedding")):
        return 0.0, 2.0 ** -2, code
    if name.endswith("position_embedding.weight"):
        return 0.0, 2.0 ** -3, code
    fan_in = int(np.prod(shape[1:]))
    step = 2.0 ** round(np.log2(1.0 / (1.1 * fan_in ** 0.5)))          # weights of std about 1 / sqrt(fan_in)
    if name.endswith(("out_proj.weight", "fc2.weight")):
        step /= 2                                                     # the branches' last GEMMs: smaller updates
    return 0.0, step, code


def main():
    from transformers import CLIPConfig, CLIPModel
    torch.manual_seed(0)
    model = CLIPModel(CLIPConfig(text_config=dict(TEXT), vision_config=dict(VISION), projection_dim=PROJ)).eval()
    g = torch.Generator().manual_seed(20240601)
    names, offs, steps, codes, sd = [], [], [], [], {}
    for name, p in model.state_dict().items():
        if name.endswith("position_ids"):
            continue
        o, s, c = coded(name, tuple(p.shape), g)
        names.append(name), offs.append(o), steps.append(s), codes.append(c.numpy())
        sd[name] = (o + s * c.float()).to(torch.float32)
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.endswith("position_ids") for k in missing), (missing, unexpected)

    pv = torch.round(torch.randn(3, 3, 56, 56, generator=g) * 16) / 16          # coarse values: the file compresses
    ids = torch.full((3, 77), EOS, dtype=torch.long)
    ids[:, 0] = BOS
    for r, w in enumerate((4, 75, 19)):
        ids[r, 1:1 + w] = torch.randint(0, BOS, (w,), generator=g)
    with torch.no_grad():
        emb = model.vision_model.embeddings(pv)
        vo = model.vision_model(pixel_values=pv, output_hidden_states=True)
        image_embeds = model.visual_projection(vo.pooler_output)
        to = model.text_model(input_ids=ids)
        text_embeds = model.text_projection(to.pooler_output)
        # the pooled row is the first EOS (the largest id): HF's legacy argmax rule
        assert torch.equal(to.pooler_output, to.last_hidden_state[torch.arange(3), ids.argmax(-1)])
        a = image_embeds / image_embeds.norm(dim=-1, keepdim=True)
        b = text_embeds / text_embeds.norm(dim=-1, keepdim=True)
        cos = a @ b.T
    assert len(vo.hidden_states) == VISION["num_hidden_layers"] + 1
    arrays = dict(vision_config=json.dumps(VISION), text_config=json.dumps(TEXT), projection_dim=PROJ,
                  param_names=np.array(names), param_offset=np.array(offs, np.float64), param_step=np.array(steps, np.float64),
                  pixel_values=pv.numpy(), embeddings=emb.numpy(), hidden_states=torch.stack(vo.hidden_states).numpy(),
                  pooler_output=vo.pooler_output.numpy(), image_embeds=image_embeds.numpy(), input_ids=ids.numpy(),
                  text_embeds=text_embeds.numpy(), cosine=cos.numpy())
    for i, c in enumerate(codes):
        arrays[f"param_{i}"] = c
    np.savez_compressed(OUT, **arrays)
    print(f"wrote {OUT}: {os.path.getsize(OUT) / 1024:.0f} KiB, {len(names)} parameters")


if __name__ == "__main__":
    main()
