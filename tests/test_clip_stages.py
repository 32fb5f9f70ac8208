"""The float64 CLIP restatement of tests/clip_stages.py (the reference of tests/test_gpu_clip_parity.py) pinned on the CPU: against
the HF module's own outputs (tests/golden/clip_text_tiny.npz), the numpy oracle, and -- where ``transformers`` imports -- HF
CLIPTextModel at full CLIP-L width on the generated stress parameters; and the generated parameter sets do what they claim."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import clip_oracle as K
from tests import clip_stages as S
from tests.util import rel_l2


@pytest.fixture(scope="module", autouse=True)
def _threads():
    n = S.cpu_threads()
    yield
    torch.set_num_threads(n)


def _tiny(golden_dir):
    z = np.load(os.path.join(golden_dir, "clip_text_tiny.npz"))
    meta = json.loads(bytes(z["meta_json"]).decode())
    return z, meta, {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd/")}


def test_loose_matches_hf_tiny_golden_and_oracle(golden_dir):
    z, meta, sd = _tiny(golden_dir)
    heads = meta["num_attention_heads"]
    out, hidden = S.forward(z["ids"], sd, "loose", heads=heads)
    assert len(hidden) == meta["num_hidden_layers"] + 1
    # the golden is HF's fp32 CPU run: fp32 noise only (measured 4.3e-7 for the output, 4.3e-7 / 4.2e-7 for taps 1 / 2, tap 0 exact)
    assert rel_l2(out.numpy(), z["out"]) < 1.3e-6
    for k, h in enumerate(hidden):
        assert rel_l2(h.numpy(), z[f"hidden/{k}"]) < (1e-12 if k == 0 else 1.3e-6), k
    ref = K.text_forward({k: v.numpy() for k, v in sd.items()}, z["ids"], heads)
    assert rel_l2(out.numpy(), ref) < 1.5e-6                     # measured 5.1e-7 (the oracle runs in fp32)
    # tight mode is the same computation with bf16 roundings: close, not equal
    tight, _ = S.forward(z["ids"], sd, "tight", heads=heads)
    assert 1e-5 < rel_l2(tight.numpy(), out.numpy()) < 2e-2


def test_generated_parameters_and_prompts():
    sd = S.clip_params("stress", seed=3, num_hidden_layers=2)
    assert list(sd)[:4] == ["embeddings.token_embedding.weight", "embeddings.position_embedding.weight",
                            "encoder.layers.0.self_attn.k_proj.weight", "encoder.layers.0.self_attn.k_proj.bias"]
    assert torch.equal(sd["encoder.layers.0.layer_norm1.weight"], S.clip_params("stress", seed=3, num_hidden_layers=2)[
        "encoder.layers.0.layer_norm1.weight"])                  # seeded
    ids = S.prompt_ids(6, seed=4)
    assert ids.shape == (6, 77) and (ids[:, 0] == S.BOS).all() and (ids[0, 1:] == S.EOS).all()
    assert int(ids.min()) == 0 and int(ids.max()) == S.EOS and (ids[1, 1:76] != S.EOS).all()
    # every branch moves the residual stream by 0.1-1x its size; the sink head's logits for key 0 lead by about 20-40
    x = S.embed(ids[1:3], sd)
    for i in range(2):
        y = S.layer(x, sd, i, "loose")
        assert 0.1 < float((y - x).norm() / x.norm()) < 1.0, i
        pre = f"encoder.layers.{i}."
        h = torch.nn.functional.layer_norm(x, (768,), S._v(sd, pre + "layer_norm1.weight"), S._v(sd, pre + "layer_norm1.bias"), 1e-5)
        lin = lambda a, n: a @ S._v(sd, pre + n + ".weight").T + S._v(sd, pre + n + ".bias")
        r = slice(64 * S.SINK_HEAD, 64 * S.SINK_HEAD + 64)
        s = lin(h, "self_attn.q_proj")[..., r] @ lin(h, "self_attn.k_proj")[..., r].transpose(-1, -2) / 8
        gap = s[:, 8:, 0] - torch.stack([s[:, q, 1:q + 1].amax(-1) for q in range(8, 77)], -1)
        assert 15 < float(gap.median()) < 45 and float(gap.min()) > 10, (i, float(gap.min()), float(gap.median()))
        x = y


def test_loose_matches_hf_clip_text_model_at_clip_l_width():
    """HF CLIPTextModel built offline from a config (never from_pretrained) at CLIP-L width with 2 layers, loaded with the stress
    parameters: its fp32 CPU last_hidden_state and hidden states against the float64 restatement."""
    transformers = pytest.importorskip("transformers")
    cfg = dict(S.CLIP_L, num_hidden_layers=2)
    sd = S.clip_params("stress", seed=11, **cfg)
    hf = transformers.CLIPTextModel(transformers.CLIPTextConfig(**cfg, hidden_act="quick_gelu", attention_dropout=0.0)).eval()
    pre = "text_model." if any(k.startswith("text_model.") for k in hf.state_dict()) else ""     # (the prefix depends on the version)
    missing, unexpected = hf.load_state_dict({pre + k: v for k, v in sd.items()}, strict=False)
    assert not unexpected and all("position_ids" in k for k in missing), (missing, unexpected)
    ids = S.prompt_ids(3, seed=12)
    with torch.no_grad():
        o = hf(input_ids=ids, output_hidden_states=True)
    out, hidden = S.forward(ids, sd, "loose")
    # fp32 noise (measured 5.9e-7; taps 1 / 2: 2.8e-7 / 4.7e-7, tap 0 exact)
    assert rel_l2(out.numpy(), o.last_hidden_state.numpy()) < 1.8e-6
    for k, h in enumerate(hidden):
        assert rel_l2(h.numpy(), o.hidden_states[k].numpy()) < (1e-12 if k == 0 else 1.5e-6), k
