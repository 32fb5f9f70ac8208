"""float64 restatement of the DINO towers and of the structure distance for the tests (a helper, not a test): HF Dinov2Model (and,
without LayerScale, HF ViTModel) stage by stage and the self-similarity distance, written from the math with torch CPU ops.

``mode="loose"``: plain float64 from the fp32 parameters.  ``mode="tight"``: rounded to bf16 exactly where dino.hip rounds -- the patch
rows and the patch weight, the GEMM weights of the layers (the out projection and fc2 with LayerScale folded in: bf16 of the fp32
product lambda[n] W[n, k], the bias lambda[n] b[n] in fp32), the LN1 / qkv / attention P / attention / LN2 outputs and the
erf-GELU output of fc1 (the activation is applied to the fp32 accumulator, one rounding); the residual stream, class token,
position table, norms and biases stay fp32 / float64.

Also here: the golden's loader, seeded parameter sets, the case lists of the GPU tests, one-fault references (``TOWER_FAULTS``,
``STRUCTURE_FAULTS``) and the bounds (``TOL``).  State dicts use the HF Dinov2Model names (the module's own)."""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

from tests.clip_vision_cases import _bf, attention, maxabs, patch_rows, rel  # noqa: F401  (the shared float64 pieces)

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "dino_tiny.npz")
FAULT_MARGIN = 10.0          # a planted fault must stand this many TOLs from the truth (tests/test_pair_metrics_host.py's margin)

# golden run -> (which model, image side the tower runs at)
GOLDEN_RUNS = dict(dinov2_70=("dinov2", 70), dinov2_42=("dinov2", 42), vit_24=("vit", 24))


def golden_module_config(model, image):
    """Keyword arguments of ``DinoVisionTransformer`` for a golden model run at ``image``."""
    c = json.loads(str(np.load(GOLDEN)[f"{model}_config"]))
    return dict(hidden_size=c["hidden_size"], num_attention_heads=c["num_attention_heads"], num_hidden_layers=c["num_hidden_layers"],
                patch_size=c["patch_size"], image_size=image, table_size=c["image_size"], mlp_ratio=4,
                layerscale=model == "dinov2", layer_norm_eps=c["layer_norm_eps"])


WIDE = dict(hidden_size=1024, num_attention_heads=16, num_hidden_layers=4, patch_size=14, image_size=224, table_size=224,
            layerscale=True, layer_norm_eps=1e-6)                                          # 257 tokens at the ViT-L width, B = 2
LONG = dict(hidden_size=128, num_attention_heads=2, num_hidden_layers=1, patch_size=8, image_size=224, table_size=224,
            layerscale=False, layer_norm_eps=1e-12)                                        # 785 tokens: the streaming attention, B = 1
SEEDED_CASES = dict(wide=(WIDE, 2), long=(LONG, 1))

STRUCTURE_T = (1, 10, 17, 257, 785)
STRUCTURE_D = (64, 384, 1024)
STRUCTURE_B = (1, 3)
STRUCTURE_DATA = ("random", "near", "zero_row", "identical")


# ------------------------------------------------------------------------------------------------------------------ golden, parameters
def load_golden():
    """-> (arrays, {"dinov2": sd, "vit": sd}) with both state dicts under the HF Dinov2Model names, in the npz's order.  value =
    offset + step * code, exact in fp32."""
    from uspace_amd.libs.dino import map_state_dict_key
    z = np.load(GOLDEN)
    sds = {}
    for tag in ("dinov2", "vit"):
        sd = {}
        for i, n in enumerate(z[f"{tag}_param_names"]):
            v = float(z[f"{tag}_param_offset"][i]) + float(z[f"{tag}_param_step"][i]) * torch.from_numpy(z[f"{tag}_param_{i}"].astype(np.float32))
            sd[map_state_dict_key(str(n))] = v.float()
        sds[tag] = sd
    return z, sds


def raw_golden_state_dict(tag):
    """The golden's state dict under the names HF gave it (what ``load_state_dict`` must accept)."""
    z = np.load(GOLDEN)
    return {str(n): (float(z[f"{tag}_param_offset"][i]) + float(z[f"{tag}_param_step"][i])
                     * torch.from_numpy(z[f"{tag}_param_{i}"].astype(np.float32))).float() for i, n in enumerate(z[f"{tag}_param_names"])}


def dino_params(seed=0, hidden_size=128, num_attention_heads=2, num_hidden_layers=2, patch_size=14, image_size=56, table_size=None,
                mlp_ratio=4, layerscale=True, **_ignored):
    """Seeded fp32 parameters in the HF Dinov2Model state_dict order: every branch moves the residual stream by a sizeable
    fraction of its size, norms and biases non-trivial, LayerScale in [0.05, 1.5], and every fc1 bias lowered by 2 with a large fc2, so that the
    MLP's output comes from the activation's negative tail, where quick-GELU and erf-GELU differ by tens of percent, and carries a
    good part of the layer's update."""
    g = torch.Generator().manual_seed(seed)
    D, Fd = hidden_size, hidden_size * mlp_ratio
    T = ((table_size or image_size) // patch_size) ** 2 + 1
    K = 3 * patch_size * patch_size
    rn = lambda *s: torch.randn(*s, generator=g)
    sd = {"embeddings.cls_token": rn(1, 1, D) * 0.5, "embeddings.position_embeddings": rn(1, T, D) * 0.3,
          "embeddings.patch_embeddings.projection.weight": rn(D, 3, patch_size, patch_size) * (0.7 / K ** 0.5),
          "embeddings.patch_embeddings.projection.bias": rn(D) * 0.2}
    for i in range(num_hidden_layers):
        pre = f"encoder.layer.{i}."
        sd[pre + "norm1.weight"] = 1.0 + 0.2 * rn(D)
        sd[pre + "norm1.bias"] = 0.1 * rn(D)
        for n, s in (("query", 1.4), ("key", 1.4), ("value", 1.0)):
            sd[pre + f"attention.attention.{n}.weight"] = rn(D, D) * (s / D ** 0.5)
            sd[pre + f"attention.attention.{n}.bias"] = rn(D) * 0.1
        sd[pre + "attention.output.dense.weight"] = rn(D, D) * (0.4 / D ** 0.5)
        sd[pre + "attention.output.dense.bias"] = rn(D) * 0.1
        if layerscale:
            sd[pre + "layer_scale1.lambda1"] = 0.05 + 1.45 * torch.rand(D, generator=g)
        sd[pre + "norm2.weight"] = 1.0 + 0.2 * rn(D)
        sd[pre + "norm2.bias"] = 0.1 * rn(D)
        sd[pre + "mlp.fc1.weight"] = rn(Fd, D) * (1.0 / D ** 0.5)
        sd[pre + "mlp.fc1.bias"] = rn(Fd) * 0.3 - 2.0
        sd[pre + "mlp.fc2.weight"] = rn(D, Fd) * (9.6 / Fd ** 0.5)
        sd[pre + "mlp.fc2.bias"] = rn(D) * 0.1
        if layerscale:
            sd[pre + "layer_scale2.lambda1"] = 0.05 + 1.45 * torch.rand(D, generator=g)
    sd["layernorm.weight"] = 1.0 + 0.2 * rn(D)
    sd["layernorm.bias"] = 0.1 * rn(D)
    return sd


def case_params(name):
    return dino_params(seed=500 + list(SEEDED_CASES).index(name), **SEEDED_CASES[name][0])


def case_pixels(name):
    cfg, B = SEEDED_CASES[name]
    g = torch.Generator().manual_seed(7500 + list(SEEDED_CASES).index(name))
    return torch.randn(B, 3, cfg["image_size"], cfg["image_size"], generator=g) * 1.2


# ------------------------------------------------------------------------------------------------------------------ the tower
def _w(sd, name, tight):
    w = sd[name]
    return (w.to(torch.bfloat16) if tight else w).to(torch.float64)


def _v(sd, name):
    return sd[name].to(torch.float64)


def n_layers(sd):
    n = 0
    while f"encoder.layer.{n}.norm1.weight" in sd:
        n += 1
    return n


def position_table(sd, grid, fault=None):
    """[grid^2 + 1, D] float64: the checkpoint's table interpolated as HF does it (bicubic, align_corners=False, fp32);
    ``fault="pos_cropped"``: the top-left grid x grid corner of the table instead."""
    t = sd["embeddings.position_embeddings"].to(torch.float32)
    n = int(round((t.shape[1] - 1) ** 0.5))
    if n == grid:
        return t[0].to(torch.float64)
    D = t.shape[-1]
    patch = t[:, 1:].reshape(1, n, n, D)
    if fault == "pos_cropped":
        patch = patch[:, :grid, :grid]
    else:
        patch = F.interpolate(patch.permute(0, 3, 1, 2), size=(grid, grid), mode="bicubic", align_corners=False).permute(0, 2, 3, 1)
    return torch.cat((t[0, :1], patch.reshape(-1, D)), 0).to(torch.float64)


def embeddings(pv, sd, mode, fault=None):
    """HF Dinov2Embeddings: cat(class, conv(pixel_values) + bias) + position table, [B, N + 1, D] float64."""
    t = mode == "tight"
    w = _w(sd, "embeddings.patch_embeddings.projection.weight", t)
    D, p = w.shape[0], w.shape[-1]
    pe = _bf(patch_rows(pv.to(torch.float64), p), t) @ w.reshape(D, -1).T
    if fault != "no_patch_bias":
        pe = pe + _v(sd, "embeddings.patch_embeddings.projection.bias")
    cls = _v(sd, "embeddings.cls_token").reshape(1, 1, D).expand(pv.shape[0], 1, D)
    return torch.cat([cls, pe], 1) + position_table(sd, pv.shape[-1] // p, fault)


def _ln(x, sd, name, eps):
    return F.layer_norm(x, (x.shape[-1],), _v(sd, name + ".weight"), _v(sd, name + ".bias"), eps)


def quick_gelu(x):
    return x * torch.sigmoid(1.702 * x)


def _scaled_linear(a, sd, pre, name, lam, tight):
    """lambda (.) (W a + b): tight folds lambda into the stored operands as dino.hip's pack step does."""
    W, b = sd[pre + name + ".weight"], sd[pre + name + ".bias"]
    if lam is None:
        return a @ _w(sd, pre + name + ".weight", tight).T + b.to(torch.float64)
    if tight:
        Wf = (lam.float()[:, None] * W.float()).to(torch.bfloat16).to(torch.float64)
        return a @ Wf.T + (lam.float() * b.float()).to(torch.float64)
    return lam.to(torch.float64) * (a @ W.to(torch.float64).T + b.to(torch.float64))


def layer(x, sd, i, mode, heads, eps=1e-6, fault=None):
    """-> (x after the layer, this layer's keys, this layer's queries), float64; keys / queries carry the bf16 rounding of the
    q|k|v GEMM's output in tight mode."""
    t = mode == "tight"
    pre = f"encoder.layer.{i}."
    x = x.to(torch.float64)
    lam = lambda k: sd.get(pre + f"layer_scale{k}.lambda1")
    l1, l2 = lam(1), lam(2)
    if fault == "no_layerscale":
        l1 = l2 = None
    elif fault == "layerscale_swapped":
        l1, l2 = l2, l1
    lin = lambda a, n: a @ _w(sd, pre + n + ".weight", t).T + _v(sd, pre + n + ".bias")
    h = _bf(_ln(x, sd, pre + "norm1", eps), t)
    q, k, v = (_bf(lin(h, f"attention.attention.{n}"), t) for n in ("query", "key", "value"))
    x = x + _scaled_linear(attention(q, k, v, heads, t), sd, pre, "attention.output.dense", l1, t)
    h = _bf(_ln(x, sd, pre + "norm2", eps), t)
    f1 = lin(h, "mlp.fc1")
    act = _bf(quick_gelu(f1) if fault == "quick_gelu" else F.gelu(f1), t)
    return x + _scaled_linear(act, sd, pre, "mlp.fc2", l2, t), k, q


def pooled(x, sd, eps=1e-6, fault=None):
    tok = x.to(torch.float64).mean(1) if fault == "pool_mean" else x.to(torch.float64)[:, 0]
    return tok if fault == "no_final_ln" else _ln(tok, sd, "layernorm", eps)


def tower_forward(pv, sd, heads, mode="loose", eps=1e-6, fault=None):
    """-> dict(embeddings, hidden=[embeddings, after layer 1, ...], pooler, keys=[per layer], last_keys), float64."""
    x = embeddings(pv, sd, mode, fault)
    hidden, keys, queries = [x], [], []
    for i in range(n_layers(sd)):
        x, k, q = layer(x, sd, i, mode, heads, eps, fault)
        hidden.append(x), keys.append(k), queries.append(q)
    last = keys[-1] if keys else None
    if fault == "keys_are_queries":
        last = queries[-1]
    elif fault == "keys_prev_layer":
        last = keys[-2]
    return dict(embeddings=hidden[0], hidden=hidden, pooler=pooled(x, sd, eps, fault), keys=keys, last_keys=last)


# ------------------------------------------------------------------------------------------------------------------ structure distance
def self_similarity(k, fault=None):
    k = k.to(torch.float64)
    if fault == "no_cls":
        k = k[..., 1:, :]
    g = k @ k.transpose(-1, -2)
    if fault == "unnormalised":
        return g
    n = k.norm(dim=-1)
    rows = torch.roll(n, 1, dims=-1) if fault == "neighbour_norm" else n
    return g / (rows[..., :, None] * n[..., None, :]).clamp_min(1e-8)


def structure(keys_a, keys_b, fault=None):
    """float64 [P]: mean over i, j of (S(Ka) - S(Kb))^2, the class token included."""
    if fault == "next_pair_b":
        keys_b = torch.roll(keys_b, -1, dims=0)
    d = (self_similarity(keys_a, fault) - self_similarity(keys_b, fault)) ** 2
    return d.sum((-1, -2)) if fault == "no_mean" else d.mean((-1, -2))


def structure_keys(T, D, B, data, seed=0):
    """(keys_a, keys_b) bf16 [B, T, D]: "random" independent sets with rows of very different lengths; "near": b = a plus a
    perturbation of about 2 %; "zero_row": random with one all-zero key row in each member (the 1e-8 floor); "identical": b = a."""
    g = torch.Generator().manual_seed(9000 + 131 * T + 7 * D + B + 1000 * seed)
    a = torch.randn(B, T, D, generator=g) * torch.exp(torch.randn(B, T, 1, generator=g))
    if data == "identical":
        b = a.clone()
    elif data == "near":
        b = a + 0.02 * torch.randn(B, T, D, generator=g) * a.abs().mean()
    else:
        b = torch.randn(B, T, D, generator=g) * torch.exp(torch.randn(B, T, 1, generator=g))
    if data == "zero_row":
        a[:, T // 2] = 0.0
        b[:, T - 1] = 0.0
    return a.to(torch.bfloat16), b.to(torch.bfloat16)


# ------------------------------------------------------------------------------------------------------------------ faults
# name -> (metric the fault must show in, what it does).  tests/test_dino_host.py builds every faulty reference and requires its
# distance from the true reference, in that metric, to be at least FAULT_MARGIN times the metric's TOL entry.
TOWER_FAULTS = dict(
    quick_gelu=("update", "quick-GELU instead of erf-GELU"),
    no_layerscale=("update", "LayerScale omitted"),
    layerscale_swapped=("update", "lambda1 of the two branches swapped"),
    no_patch_bias=("embeddings", "patch bias omitted"),
    pos_cropped=("embeddings", "position table cropped instead of interpolated"),
    no_final_ln=("pooler", "final LayerNorm omitted"),
    pool_mean=("pooler", "mean over tokens instead of the class token"),
    keys_are_queries=("keys", "queries returned as keys"),
    keys_prev_layer=("keys", "keys of the layer before"),
)
STRUCTURE_FAULTS = dict(
    unnormalised=("structure", "Gram matrix not normalised"),
    no_mean=("structure", "1 / T^2 forgotten"),
    no_cls=("structure", "class token excluded"),
    neighbour_norm=("structure", "a row normalised by its neighbour's norm"),
    next_pair_b=("structure", "member b of the next pair"),
)

# GPU bounds: 3x the worst value an MI355X measured against the float64 model or the golden (the convention of
# tests/clip_vision_cases.py); the measured value and the case that produced it stand beside each.  rel-L2 unless it says otherwise.
TOL = dict(
    embeddings=6.5e-3,         # measured 2.17e-3 (long; 2.15e-3 wide; 0 on the goldens, whose values are exact in bf16): vs the loose model /
                               # the golden, the bf16 rounding of the patch rows and the patch weight
    embeddings_tight=3.9e-7,   # measured 1.28e-7 (wide, K = 588 -> 640): vs the model with those two roundings, fp32 accumulation left
    hidden=2.4e-2,             # measured 7.99e-3 (wide, after layer 4; goldens 1.8e-3): every hidden state vs the loose model / the golden
    update=5.6e-3,             # measured 1.87e-3 (long, the streaming attention kernel; 1.30e-3 wide; 1.9e-5 on the goldens):
                               # ||T_k - layer(T_{k-1}, tight)|| / ||T_k - T_{k-1}|| from the GPU's own previous tap
    pooler=1.8e-7,             # measured 5.85e-8 (vit_24): the final LayerNorm of token 0 vs float64 of the GPU's last tap
    pooler_e2e=2.3e-2,         # measured 7.70e-3 (wide; goldens 3.5e-3; 3.1e-3 on the features of the end-to-end test): vs the loose model / golden
    keys=2.5e-4,               # measured 8.24e-5 (wide; 0 on the goldens): the bf16 keys vs the tight model's bf16 keys from the GPU's tap
    keys_golden=2.3e-2,        # measured 7.52e-3 (wide; goldens 2.8e-3, the bf16 rounding of the keys alone is 1.7e-3): vs the loose model / golden
    structure=1.5e-6,          # measured 4.93e-7 (T = 10, D = 1024, B = 3, zero_row; random 1.19e-7): the kernel vs float64 of the same stored
                               # keys, relative per pair
    structure_near=4.6e-6,     # measured 1.52e-6 (T = 10, D = 1024, B = 3): the same on near-identical members, where the differences cancel
    structure_e2e=2.2e-2,      # measured 7.29e-3 (images -> preprocess -> tiny tower -> keys -> distance vs the loose model; 1.1e-3 on the
                               # goldens' pixel_values): relative per pair
    fd=6.2e-4,                 # measured 2.04e-4 (160 + 160 images, tiny tower, FD 30.97): FDDino vs the Frechet distance of the loose model's features
)
