"""The calls whose raw output bytes pin the three ViT towers bit for bit (a helper, not a test): the CLIP text tower, the CLIP vision
tower and the DINO towers on fixtures the other tests already build.  Shared by tests/golden/make_vit_tower_digests.py (which records
the sha256 of every output) and tests/test_gpu_vit_tower_bits.py (which compares).  Every call is run-to-run bit-equal (the towers'
own tests assert it), so a change of the host code that moves no launch and no operand leaves every digest as it is."""
import hashlib
import json
import os

import numpy as np
import torch

from tests import clip_vision_cases as V
from tests import dino_cases as D

HERE = os.path.dirname(os.path.abspath(__file__))
DIGESTS = os.path.join(HERE, "golden", "vit_tower_digests.json")
VISION_CASES = ("tiny", "patch32")            # K 588 padded to 640, 17 tokens; K 3072 without pad, 50 tokens


def digest(t):
    """sha256 of the tensor's bytes as they lie in memory (bf16 as its 16-bit patterns)."""
    t = t.detach().cpu().contiguous()
    if t.dtype == torch.bfloat16:
        t = t.view(torch.int16)
    return hashlib.sha256(t.numpy().tobytes()).hexdigest()


def text_outputs():
    from uspace_amd.libs.clip import CLIPTextTransformer
    z = np.load(os.path.join(HERE, "golden", "clip_text_tiny.npz"))
    meta = json.loads(bytes(z["meta_json"]).decode())
    m = CLIPTextTransformer(**{k: meta[k] for k in ("vocab_size", "hidden_size", "intermediate_size", "num_hidden_layers",
                                                    "num_attention_heads", "max_position_embeddings", "layer_norm_eps", "hidden_act")})
    m.load_state_dict({"text_model." + k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd/")})
    m = m.cuda()
    ids = V.tiny_ids(3).cuda()
    assert int(ids.max()) < meta["vocab_size"] and ids.shape[1] <= meta["max_position_embeddings"]
    yield "last_hidden_state", m(ids)
    yield "hidden_state=1", m(ids, hidden_state=1)


def vision_outputs(name):
    from uspace_amd.libs.clip import CLIPVisionTransformer
    cfg = V.TOWER_CASES[name][0]
    m = CLIPVisionTransformer(**cfg)
    m.load_state_dict(V.case_params(name))
    m = m.cuda()
    pv = V.case_pixels(name).cuda()
    emb, pooled = m(pv, return_pooled=True)
    yield "image_embeds", emb
    yield "pooler_output", pooled
    for h in ("embeddings", 0, cfg["num_hidden_layers"]):
        yield f"hidden_state={h}", m(pv, hidden_state=h)


def dino_outputs(run):
    from uspace_amd.libs.dino import DinoVisionTransformer
    model, side = D.GOLDEN_RUNS[run]
    m = DinoVisionTransformer(seed=0, **D.golden_module_config(model, side))
    m.load_state_dict(D.raw_golden_state_dict(model))
    m = m.cuda()
    pv = torch.from_numpy(np.load(D.GOLDEN)[f"{run}_pixel_values"]).cuda()
    yield "pooler_output", m(pv)
    for h in ("embeddings", 1):
        yield f"hidden_state={h}", m(pv, hidden_state=h)
    for layer in (0, -1):
        yield f"keys(layer={layer})", m.keys(pv, layer=layer)


# tower case -> generator of (call, output tensor)
CASES = {"clip_text/tiny": text_outputs}
CASES.update({f"clip_vision/{n}": (lambda n=n: vision_outputs(n)) for n in VISION_CASES})
CASES.update({f"dino/{r}": (lambda r=r: dino_outputs(r)) for r in D.GOLDEN_RUNS})


def case_digests(case):
    """{call: sha256} of one tower case, computed on the GPU."""
    out = {call: digest(t) for call, t in CASES[case]()}
    torch.cuda.synchronize()
    return out
