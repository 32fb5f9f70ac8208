"""CLIP score, host side (no GPU): the float64 restatement of tests/clip_vision_cases.py against the Hugging Face golden and against
live HF at the CLIP-L width, its resize matrices against torch's antialiased bicubic in float64, the power of the bounds (every
one-fault reference lies at least twice its bound away), the state dict's keys and order, and the new C-ABI symbols."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import clip_vision_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# float64 model against HF's fp32 CPU forward: measured here 0 (embeddings: the golden's coarse parameters) ... 3.3e-7 (text_embeds), rel-L2 -- fp32 rounding
# of HF's own arithmetic; 3x the worst
HF_REL = 1.0e-6
HF_COS = 2.3e-7          # measured 7.4e-8, absolute, on the 3 x 3 cosine matrix
HF_REL_L = 1.6e-6        # measured 5.3e-7 at the CLIP-L width (K = 1024 / 4096 sums in fp32)
RESIZE_ABS = 1.2e-12     # measured 3.7e-13 on values in [0, 255] (1.4e-15 relative): float64 rounding of two summation orders

NEW_SYMBOLS = ("uspace_clipv_num_params", "uspace_clipv_param_numel", "uspace_clipv_weight_bytes", "uspace_clipv_workspace_bytes",
               "uspace_clipv_pack_weights", "uspace_clipv_forward", "uspace_clip_preprocess", "uspace_linear_f32",
               "uspace_gather_rows_f32", "uspace_cosine_f32", "uspace_normalized_diff_f32")


@pytest.fixture(scope="module")
def golden():
    z, sd = C.load_golden()
    pv = torch.from_numpy(z["pixel_values"])
    ids = torch.from_numpy(z["input_ids"])
    ref = C.vision_forward(pv, sd, 2, "loose")
    lh = C.text_forward(ids, sd, 2)
    te = C.text_embeds(lh, ids, sd["text_projection.weight"])
    return dict(z=z, sd=sd, pv=pv, ids=ids, ref=ref, last_hidden=lh, text_embeds=te)


def test_float64_model_equals_the_hf_golden(golden):
    z, ref = golden["z"], golden["ref"]
    errs = dict(embeddings=C.rel(ref["embeddings"], z["embeddings"]), pooler=C.rel(ref["pooler_output"], z["pooler_output"]),
                image_embeds=C.rel(ref["image_embeds"], z["image_embeds"]), text_embeds=C.rel(golden["text_embeds"], z["text_embeds"]))
    for k in range(3):
        errs[f"hidden{k}"] = C.rel(ref["hidden"][k], z["hidden_states"][k])
    cos = C.maxabs(C.cosine(ref["image_embeds"][:, None], golden["text_embeds"][None]), z["cosine"])
    print({k: "%.2e" % v for k, v in errs.items()}, "cosine %.2e" % cos)
    assert max(errs.values()) < HF_REL, errs
    assert cos < HF_COS
    # the tight model (bf16 where the kernels round) stays within the bf16 budget of the loose one
    tight = C.vision_forward(golden["pv"], golden["sd"], 2, "tight")
    assert 1e-4 < C.rel(tight["hidden"][2], ref["hidden"][2]) < 2e-2


def test_float64_model_equals_live_hf_at_clip_l_width():
    tr = pytest.importorskip("transformers")
    cfg = C.TOWER_CASES["clip_l"][0]
    n = C.S.cpu_threads()
    try:
        sd = C.vision_params("workflow", seed=5, **cfg)
        hf = tr.CLIPVisionModelWithProjection(tr.CLIPVisionConfig(hidden_act="quick_gelu", **cfg)).eval()
        assert list(hf.state_dict().keys()) == list(sd.keys())
        hf.load_state_dict(sd)
        pv = torch.randn(1, 3, 224, 224, generator=torch.Generator().manual_seed(6))
        with torch.no_grad():
            out = hf(pixel_values=pv, output_hidden_states=True)
        ref = C.vision_forward(pv, sd, cfg["num_attention_heads"], "loose")
        errs = [C.rel(ref["hidden"][k], out.hidden_states[k]) for k in range(3)] + [C.rel(ref["image_embeds"], out.image_embeds)]
        print(["%.2e" % e for e in errs])
        assert max(errs) < HF_REL_L, errs
    finally:
        torch.set_num_threads(n)


@pytest.mark.parametrize("H,S", C.PREPROCESS_SIZES)
def test_two_matrix_resize_equals_torch_float64(H, S):
    x = torch.rand(2, 3, H, H, dtype=torch.float64, generator=torch.Generator().manual_seed(H + S)) * 255.0
    W = C.resize_matrix(H, S)
    ref = F.interpolate(x, size=(S, S), mode="bicubic", antialias=True, align_corners=False)
    e = C.maxabs(W @ x @ W.T, ref)
    print(f"{H}->{S}: {e:.2e}")
    assert e < RESIZE_ABS
    assert torch.allclose(W.sum(1), torch.ones(S, dtype=torch.float64), atol=1e-14)       # renormalised windows, clipped ones too
    if H == S:
        assert torch.equal(W, torch.eye(S, dtype=torch.float64))


def _fault_distances(golden):
    """name -> distance of the one-fault reference from the true one, in the fault's metric, on the data meant to expose it."""
    sd, pv, ids, ref = golden["sd"], golden["pv"], golden["ids"], golden["ref"]
    d = {}
    for name in ("pos_shifted", "py_px_swapped", "k_order_ppc", "pad_nonzero"):
        d[name] = C.rel(C.embeddings(pv, sd, "loose", name), ref["embeddings"])
    d["no_pre_ln"] = C.rel(C.vision_forward(pv, sd, 2, "loose", fault="no_pre_ln")["hidden"][0], ref["hidden"][0])
    d["pool_mean"] = C.rel(C.pooled(ref["hidden"][2], sd, fault="pool_mean"), ref["pooler_output"])
    d["causal"] = float((C.layer(ref["hidden"][0], sd, 0, "loose", 2, fault="causal") - ref["hidden"][1]).norm()
                        / (ref["hidden"][1] - ref["hidden"][0]).norm())
    # quick-GELU and erf-GELU agree to a percent where the pre-activations are centred; the "gelu_tail" set (case one_tile) is theirs
    cfg, kind, B = C.TOWER_CASES["one_tile"]
    tail = C.vision_params(kind, seed=C.case_seed("one_tile"), **cfg)
    r = C.vision_forward(C.case_pixels("one_tile"), tail, cfg["num_attention_heads"], "loose")
    d["erf_gelu"] = float((C.layer(r["hidden"][0], tail, 0, "loose", 2, fault="erf_gelu") - r["hidden"][1]).norm()
                          / (r["hidden"][1] - r["hidden"][0]).norm())
    d["pool_last"] = C.rel(C.text_embeds(golden["last_hidden"], ids, sd["text_projection.weight"], fault="pool_last"), golden["text_embeds"])
    a, b = ref["image_embeds"], golden["text_embeds"]
    d["cos_unnormalised"] = C.maxabs(C.cosine(a, b, "cos_unnormalised"), C.cosine(a, b))
    img = C.make_images(2, 256, seed=3)
    true = C.preprocess(img, 224)
    d["no_antialias"] = C.maxabs(C.preprocess(img, 224, antialias=False), true)
    d["align_corners"] = C.maxabs(C.preprocess(img, 224, antialias=False, align_corners=True), true)
    d["mean_std_reversed"] = C.maxabs(C.preprocess(img, 224, mean=C.CLIP_MEAN[::-1], std=C.CLIP_STD[::-1]), true)
    d["no_quantize"] = C.maxabs(C.preprocess(img, 224, quantize=False), true)
    return d


def test_every_fault_lies_at_least_twice_its_bound_away(golden):
    d = _fault_distances(golden)
    assert set(d) == set(C.PERTURBED)
    print({k: "%.2e" % v for k, v in d.items()})
    weak = {k: (v, C.TOL[C.PERTURBED[k][0]]) for k, v in d.items() if not v >= 2.0 * C.TOL[C.PERTURBED[k][0]]}
    assert not weak, weak


def test_state_dict_keys_and_order_equal_hf(golden):
    from uspace_amd.libs.clip import CLIPTextProjection, CLIPVisionTransformer
    names = [str(n) for n in golden["z"]["param_names"]]
    want = [n for n in names if n.startswith(("vision_model.", "visual_projection"))]
    m = CLIPVisionTransformer(**C.TINY_VISION)
    assert list(m.state_dict().keys()) == want
    assert [tuple(v.shape) for v in m.state_dict().values()] == [tuple(golden["sd"][n].shape) for n in want]
    m.load_state_dict(golden["sd"])                                            # a CLIPModel checkpoint: text entries dropped
    assert torch.equal(m.state_dict()["visual_projection.weight"], golden["sd"]["visual_projection.weight"])
    m.load_state_dict({k[len(C.VP):] if k.startswith(C.VP) else k: v for k, v in golden["sd"].items() if k in want})   # no prefix
    p = CLIPTextProjection(128, 64)
    assert list(p.state_dict().keys()) == ["text_projection.weight"]
    p.load_state_dict(golden["sd"])
    assert torch.equal(p.text_projection.weight, golden["sd"]["text_projection.weight"])
    with pytest.raises(NotImplementedError):
        CLIPVisionTransformer(**dict(C.TINY_VISION, hidden_act="gelu"))
    with pytest.raises(NotImplementedError):
        CLIPVisionTransformer(**dict(C.TINY_VISION, num_attention_heads=4))     # head dim 32


def test_pooled_index_follows_hf():
    from uspace_amd.libs.clip import CLIPTextProjection
    ids = torch.tensor([[998, 5, 999, 999], [998, 7, 8, 999], [998, 999, 3, 4]])
    assert CLIPTextProjection.pooled_index(ids).tolist() == [2, 3, 1]
    assert CLIPTextProjection.pooled_index(ids, 2).tolist() == [2, 3, 1]
    assert CLIPTextProjection.pooled_index(torch.tensor([[1, 2000, 7, 7], [7, 1, 2, 7]]), 7).tolist() == [2, 0]


def test_new_symbols_are_declared_bound_and_exported():
    from uspace_amd import _hip
    hdr = open(os.path.join(ROOT, "include", "uspace_hip.h")).read()
    declared = set(re.findall(r"USPACE_API\s+[\w\s\*]+?\b(uspace_\w+)\s*\(", hdr))
    L = _hip.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _hip.SIGNATURES and hasattr(L, name), name
    assert _hip.ABI_VERSION == 11 and L.uspace_abi_version() == 11
    # the config struct, field by field against the header
    body = re.search(r"struct\s+uspace_clipv_config\s*\{(.*?)\}", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S), flags=re.S).group(1)
    fields = [tuple(d.split()) for d in body.split(";") if d.strip()]
    ctype = {"int": ctypes.c_int, "float": ctypes.c_float}
    assert [(n, ctype[t]) for t, n in fields] == list(_hip.ClipVisionConfig._fields_)


def test_invalid_vision_configs_report_no_parameters_and_no_bytes():
    from uspace_amd import _hip
    L = _hip.lib()
    good = _hip.ClipVisionConfig(224, 14, 1024, 16, 24, 4096, 768, 1e-5)
    n = L.uspace_clipv_num_params(ctypes.byref(good))
    assert n == 5 + 24 * 16 + 3
    total = sum(L.uspace_clipv_param_numel(ctypes.byref(good), i) for i in range(n))
    D, Fd = 1024, 4096
    per_layer = 4 * (D * D + D) + 2 * D + (Fd * D + Fd) + (D * Fd + D) + 2 * D
    assert total == D + D * 588 + 257 * D + 2 * D + 24 * per_layer + 2 * D + 768 * D
    assert L.uspace_clipv_param_numel(ctypes.byref(good), 1) == 1024 * 588
    assert L.uspace_clipv_weight_bytes(ctypes.byref(good)) > 2 * total
    assert L.uspace_clipv_workspace_bytes(ctypes.byref(good), 2) > 2 * 257 * 1024 * 4
    bad = [(224, 14, 1000, 16, 24, 4096, 768), (224, 14, 1024, 8, 24, 4096, 768), (224, 14, 1024, 16, 24, 4100, 768),
           (224, 14, 1024, 16, 24, 4096, 770), (224, 15, 1024, 16, 24, 4096, 768), (0, 14, 1024, 16, 24, 4096, 768),
           (224, 14, 1024, 16, -1, 4096, 768)]
    for b in bad:
        cfg = _hip.ClipVisionConfig(*b, 1e-5)
        assert L.uspace_clipv_num_params(ctypes.byref(cfg)) < 0, b
        assert L.uspace_clipv_param_numel(ctypes.byref(cfg), 0) < 0, b
        assert L.uspace_clipv_weight_bytes(ctypes.byref(cfg)) == 0, b
        assert L.uspace_clipv_workspace_bytes(ctypes.byref(cfg), 4) == 0, b
    assert L.uspace_clipv_workspace_bytes(ctypes.byref(good), 0) == 0


def test_host_tensors_are_refused_without_a_gpu(golden):
    from uspace_amd import _hip
    from uspace_amd.libs.clip import CLIPTextProjection, CLIPVisionTransformer
    from uspace_amd.tools import clip_score
    m = CLIPVisionTransformer(**C.TINY_VISION)
    with pytest.raises(_hip.UspaceHipError):
        m(golden["pv"])
    with pytest.raises(_hip.UspaceHipError):
        m.preprocess(torch.rand(1, 3, 64, 64))
    with pytest.raises(_hip.UspaceHipError):
        CLIPTextProjection(128, 64)(torch.zeros(1, 77, 128), golden["ids"][:1])
    with pytest.raises(_hip.UspaceHipError):
        clip_score.cosine(torch.zeros(2, 8), torch.zeros(2, 8))
