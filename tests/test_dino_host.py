"""CPU-only checks of the DINO towers and the structure distance: the float64 stage model of tests/dino_cases.py against the Hugging
Face golden, every planted fault against the bounds the GPU tests use, the library's parameter table against the golden's state
dicts, the weight-name mapping, the refused configurations, the Frechet distance on features, the ABI and ``PairMetrics`` left as
it was."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import dino_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("uspace_dino_num_params", "uspace_dino_param_numel", "uspace_dino_weight_bytes", "uspace_dino_workspace_bytes",
               "uspace_dino_pack_weights", "uspace_dino_forward", "uspace_self_similarity_mse_workspace_bytes",
               "uspace_self_similarity_mse_f64")


@pytest.fixture(scope="module")
def golden():
    return C.load_golden()


# ------------------------------------------------------------------------------------------------------------------ the stage model
@pytest.mark.parametrize("run", list(C.GOLDEN_RUNS))
def test_stage_model_meets_the_golden(golden, run):
    z, sds = golden
    model, _side = C.GOLDEN_RUNS[run]
    cfg = C.golden_module_config(model, _side)
    sd = sds[model]
    pv = torch.from_numpy(z[f"{run}_pixel_values"])
    out = C.tower_forward(pv, sd, cfg["num_attention_heads"], "loose", cfg["layer_norm_eps"])
    hs = z[f"{run}_hidden_states"]
    assert len(out["hidden"]) == hs.shape[0] == cfg["num_hidden_layers"] + 1
    errs = dict(embeddings=C.rel(out["embeddings"], z[f"{run}_embeddings"]),
                hidden=max(C.rel(h, hs[k]) for k, h in enumerate(out["hidden"])),
                pooler=C.rel(out["pooler"], z[f"{run}_pooler"]), keys=C.rel(out["last_keys"], z[f"{run}_keys"]))
    pairs = z[f"{run}_pairs"]
    k = out["last_keys"]
    d = C.structure(k[pairs[:, 0]], k[pairs[:, 1]]).numpy()
    want = z[f"{run}_structure"]
    print(run, {n: "%.2e" % e for n, e in errs.items()}, "structure", d, want)
    assert max(errs.values()) < 2e-6, errs                      # HF's own fp32 arithmetic
    same = pairs[:, 0] == pairs[:, 1]
    assert np.all(d[same] == 0.0) and np.all(want[same] == 0.0)
    assert np.max(np.abs(d[~same] - want[~same]) / want[~same]) < 1e-5


def test_interpolated_table_is_what_the_module_packs(golden):
    from uspace_amd.libs.dino import interpolate_position_table
    _z, sds = golden
    t = sds["dinov2"]["embeddings.position_embeddings"]
    assert torch.equal(interpolate_position_table(t, 5), t)
    got = interpolate_position_table(t, 3)
    assert got.shape == (1, 10, 128) and C.maxabs(got[0], C.position_table(sds["dinov2"], 3)) == 0.0
    assert C.rel(C.position_table(sds["dinov2"], 3, "pos_cropped"), got[0]) > 0.1


# ------------------------------------------------------------------------------------------------------------------ faults
def test_every_tower_fault_stands_clear_of_the_bounds():
    """Seeded parameters with a 5 x 5 table run at 3 x 3 (so that cropping differs from interpolating) and fc1 biases that put the
    MLP on the activation's negative tail (so that quick-GELU differs from erf-GELU)."""
    cfg = dict(hidden_size=128, num_attention_heads=2, num_hidden_layers=3, patch_size=14, image_size=42, table_size=70)
    sd = C.dino_params(seed=3, **cfg)
    pv = torch.randn(3, 3, 42, 42, generator=torch.Generator().manual_seed(5)) * 1.2
    ref = C.tower_forward(pv, sd, 2, "loose")
    seen = {}
    for name, (metric, _what) in C.TOWER_FAULTS.items():
        bad = C.tower_forward(pv, sd, 2, "loose", fault=name)
        if metric == "update":          # per layer from the TRUE previous state, as the GPU test measures it
            d = min(float((C.layer(ref["hidden"][k], sd, k, "loose", 2, fault=name)[0] - ref["hidden"][k + 1]).norm()
                          / (ref["hidden"][k + 1] - ref["hidden"][k]).norm()) for k in range(3))
        elif metric == "keys":
            d = C.rel(bad["last_keys"], ref["last_keys"])
        else:
            d = C.rel(bad[metric], ref[metric])
        seen[name] = d
        assert d > C.FAULT_MARGIN * C.TOL[metric], (name, metric, d, C.TOL[metric])
    print({n: "%.2e" % d for n, d in seen.items()})


def test_every_structure_fault_stands_clear_of_the_bounds():
    seen = {}
    for name, (metric, _what) in C.STRUCTURE_FAULTS.items():
        worst = np.inf
        for T, D in ((10, 64), (17, 384), (257, 64)):
            a, b = C.structure_keys(T, D, 3, "random")
            ref, bad = C.structure(a, b).numpy(), C.structure(a, b, fault=name).numpy()
            worst = min(worst, float(np.min(np.abs(bad - ref) / ref)))
        seen[name] = worst
        assert worst > C.FAULT_MARGIN * C.TOL[metric], (name, worst)
    print({n: "%.2e" % d for n, d in seen.items()})
    a, _ = C.structure_keys(17, 64, 2, "identical")
    assert torch.all(C.structure(a, a) == 0.0)
    a, b = C.structure_keys(17, 64, 2, "zero_row")
    assert torch.isfinite(C.structure(a, b)).all()


# ------------------------------------------------------------------------------------------------------------------ the library
def _lib_cfg(cfg):
    from uspace_amd import _hip
    D = cfg["hidden_size"]
    return _hip.DinoConfig(cfg["image_size"], cfg["patch_size"], D, cfg["num_attention_heads"], cfg["num_hidden_layers"],
                           D * cfg.get("mlp_ratio", 4), 1 if cfg["layerscale"] else 0, cfg["layer_norm_eps"])


@pytest.mark.parametrize("model,side", [("dinov2", 70), ("vit", 40)])
def test_parameter_table_agrees_with_the_golden_state_dict(golden, model, side):
    from uspace_amd import _hip
    from uspace_amd.libs.dino import DinoVisionTransformer
    _z, sds = golden
    L = _hip.lib()
    cfg = C.golden_module_config(model, side)
    c = _lib_cfg(cfg)
    m = DinoVisionTransformer(seed=0, **cfg)
    own = list(m.state_dict())
    sd = sds[model]
    assert set(own) == set(sd)
    if model == "dinov2":
        assert own == list(sd)                                   # HF Dinov2Model's order, mask_token dropped
    n = L.uspace_dino_num_params(ctypes.byref(c))
    assert n == len(own)
    numels = [L.uspace_dino_param_numel(ctypes.byref(c), i) for i in range(n)]
    assert numels == [sd[k].numel() for k in own]
    assert L.uspace_dino_param_numel(ctypes.byref(c), n) < 0
    D, K = cfg["hidden_size"], 3 * cfg["patch_size"] ** 2
    al = lambda v: (v + 255) // 256 * 256
    Kp = (K + 63) // 64 * 64
    want, i = 0, 0
    while i < len(own):
        k = own[i]
        if k.endswith("projection.weight"):
            want += al(D * Kp * 2)
        elif k.endswith("query.weight"):                         # q | k | v packed: weights, then biases
            want += al(3 * D * D * 2) + al(3 * D * 4)
            i += 5
        elif k.endswith("weight") and sd[k].dim() == 2:
            want += al(sd[k].numel() * 2)
        else:
            want += al(sd[k].numel() * 4)
        i += 1
    assert L.uspace_dino_weight_bytes(ctypes.byref(c)) == want + al(D * K * 2)      # + the pad step's staging copy
    assert L.uspace_dino_workspace_bytes(ctypes.byref(c), 2) > 2 * m.tokens * D * 4
    m.load_state_dict(C.raw_golden_state_dict(model))
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k]), k
    if side != 42:                   # the table the kernels would read at another side: interpolated, and counted by the library
        m42 = DinoVisionTransformer(seed=0, **dict(cfg, image_size=cfg["patch_size"] * 3))
        c42 = _lib_cfg(dict(cfg, image_size=cfg["patch_size"] * 3))
        shapes = [p.numel() for p in m42._canonical_params()]
        assert shapes[1] == 10 * D == L.uspace_dino_param_numel(ctypes.byref(c42), 1)


def test_name_mapping_round_trips():
    from uspace_amd.libs.dino import DinoVisionTransformer, map_state_dict_key
    cfg = dict(hidden_size=64, num_attention_heads=1, num_hidden_layers=2, patch_size=8, image_size=16, layerscale=False)
    m = DinoVisionTransformer(seed=1, **cfg)
    own = {k: v.clone() for k, v in m.state_dict().items()}
    classic = {}                   # the spelling of the published ViT files, with the prefix of a model with a head
    for k, v in own.items():
        c = k.replace("norm1.", "layernorm_before.").replace("norm2.", "layernorm_after.")
        c = c.replace("mlp.fc1.", "intermediate.dense.").replace("mlp.fc2.", "output.dense.")
        classic["vit." + c] = v + 1.0
    classic["vit.pooler.dense.weight"] = torch.zeros(64, 64)
    classic["classifier.weight"] = torch.zeros(3, 64)
    assert [map_state_dict_key(k) for k in classic if map_state_dict_key(k)] == list(own)
    m.load_state_dict(classic)
    assert all(torch.equal(v, own[k] + 1.0) for k, v in m.state_dict().items())
    m2 = DinoVisionTransformer(seed=2, **dict(cfg, layerscale=True))
    pref = {"dinov2." + k: v for k, v in m2.state_dict().items()}
    pref["dinov2.embeddings.mask_token"] = torch.zeros(1, 64)
    assert [map_state_dict_key(k) for k in pref][:-1] == list(m2.state_dict()) and map_state_dict_key("dinov2.embeddings.mask_token") is None
    m2.load_state_dict(pref)
    with pytest.raises(RuntimeError):
        m.load_state_dict(pref)                                   # LayerScale entries for a tower without


def test_unsupported_configurations_raise():
    from uspace_amd import _hip
    from uspace_amd.libs.dino import DINO_B8, DINOV2_B14, DINOV2_L14, DINOV2_S14, DinoVisionTransformer
    ok = dict(hidden_size=64, num_attention_heads=1, num_hidden_layers=1, patch_size=8, image_size=16, seed=0)
    DinoVisionTransformer(**ok)
    for bad, word in ((dict(use_swiglu_ffn=True), "SwiGLU"), (dict(num_register_tokens=4), "register"),
                      (dict(hidden_size=96), "head_dim"), (dict(image_size=20), "patch_size")):
        with pytest.raises(NotImplementedError, match=word):
            DinoVisionTransformer(**dict(ok, **bad))
    with pytest.raises(FileNotFoundError, match="never downloads"):
        DinoVisionTransformer(**dict(ok, seed=None))
    L = _hip.lib()
    good = _hip.DinoConfig(224, 14, 1024, 16, 24, 4096, 1, 1e-6)
    assert L.uspace_dino_num_params(ctypes.byref(good)) == 4 + 24 * 18 + 2
    for c in (_hip.DinoConfig(224, 14, 1024, 8, 24, 4096, 1, 1e-6), _hip.DinoConfig(225, 14, 1024, 16, 24, 4096, 1, 1e-6),
              _hip.DinoConfig(224, 14, 1024, 16, 24, 4096, 2, 1e-6), _hip.DinoConfig(224, 14, 1024, 16, 24, 4100, 1, 1e-6)):
        assert L.uspace_dino_num_params(ctypes.byref(c)) == -1 and L.uspace_dino_weight_bytes(ctypes.byref(c)) == 0
        assert L.uspace_dino_workspace_bytes(ctypes.byref(c), 1) == 0
    assert L.uspace_self_similarity_mse_workspace_bytes(0, 10) == 0 and L.uspace_self_similarity_mse_workspace_bytes(1, 1 << 20) == 0
    assert L.uspace_self_similarity_mse_workspace_bytes(2, 785) >= 2 * (2 * 785 + 50 * 50) * 4
    for preset, tokens in ((DINOV2_L14, 257), (DINOV2_B14, 257), (DINOV2_S14, 257), (DINO_B8, 785)):
        assert (preset["image_size"] // preset["patch_size"]) ** 2 + 1 == tokens
        assert preset["hidden_size"] == 64 * preset["num_attention_heads"]


# ------------------------------------------------------------------------------------------------------------------ metrics, ABI
def test_fd_on_features_is_the_float64_frechet_distance():
    from scipy import linalg
    from uspace_amd.tools.dino_metrics import fd
    g = np.random.default_rng(0)
    a = g.standard_normal((200, 24)).astype(np.float32) @ g.standard_normal((24, 24)).astype(np.float32)
    b = (g.standard_normal((150, 24)).astype(np.float32) + 0.3) @ g.standard_normal((24, 24)).astype(np.float32)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    ma, mb = a64.mean(0), b64.mean(0)
    ca, cb = np.cov(a64, rowvar=False), np.cov(b64, rowvar=False)
    want = float(((ma - mb) ** 2).sum() + np.trace(ca) + np.trace(cb) - 2 * np.trace(linalg.sqrtm(ca @ cb).real))
    assert abs(fd(a, b) - want) <= 1e-9 * abs(want)
    assert abs(fd(torch.from_numpy(a), torch.from_numpy(b)) - want) <= 1e-9 * abs(want)
    assert abs(fd(a, a)) < 1e-6 * np.trace(ca)


def test_abi_is_still_11_and_the_symbols_are_declared():
    from uspace_amd import _hip
    hdr = open(os.path.join(ROOT, "include", "uspace_hip.h")).read()
    declared = set(re.findall(r"USPACE_API\s+[\w\s\*]+?\b(uspace_\w+)\s*\(", hdr))
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    L = _hip.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _hip.SIGNATURES and hasattr(L, name), name
    for name in ("uspace_dino_forward", "uspace_dino_pack_weights", "uspace_self_similarity_mse_f64", "uspace_dino_config"):
        assert name in doc, name                                   # the symbol table rows of INTEGRATION.md
    assert declared == set(_hip.SIGNATURES)
    assert "#define USPACE_ABI_VERSION 11" in hdr and L.uspace_abi_version() == _hip.ABI_VERSION == 11
    assert len(_hip.SIGNATURES["uspace_dino_forward"][1]) == 12 and len(_hip.SIGNATURES["uspace_self_similarity_mse_f64"][1]) == 11
    fields = re.search(r"struct uspace_dino_config \{(.*?)\};", hdr, re.S).group(1)
    assert re.findall(r"(?:int|float)\s+(\w+);", fields) == [f for f, _ in _hip.DinoConfig._fields_]


def test_pair_metrics_without_structure_is_unchanged():
    from uspace_amd.tools.pair_metrics import PairMetrics
    sig = inspect.signature(PairMetrics.__init__)
    assert list(sig.parameters) == ["self", "device", "lpips", "net", "structure", "identity"]
    assert sig.parameters["structure"].default is None
    assert sig.parameters["identity"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["identity"].default is None
    pm = PairMetrics(device="cpu")
    assert list(pm._parts) == ["lpips", "ssim", "psnr"] and list(pm.values) == ["lpips", "ssim", "psnr"] and pm.n == 0
    with pytest.raises(ValueError):
        pm.compute()
    assert list(PairMetrics(device="cpu", structure=object()).values) == ["lpips", "ssim", "psnr", "structure"]
