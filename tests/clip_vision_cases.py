"""float64 restatement of the CLIP score pipeline for the tests (a helper, not a test): image preprocessing in its two-matrix form,
HF CLIPVisionModelWithProjection stage by stage, the text pooling and projection, the cosine -- written from the math with torch
CPU ops.  The text tower itself is tests/clip_stages.py.

``mode="loose"``: plain float64 from the fp32 parameters.  ``mode="tight"``: rounded to bf16 exactly where clip_vision.hip rounds --
the patch rows and the patch weight, the GEMM weights of the layers, the LN1 / qkv / attention P / attention / LN2 / fc1 /
quick-GELU outputs (as tests/clip_stages.py does for the text layer); the residual stream, the class token, the position table,
the norms, biases and BOTH projections stay fp32 / float64.

Also here: seeded parameter sets in HF ``state_dict`` order ("workflow" and a "stress" set with a massive class token, a sink
head and a sharp head), the case lists of the GPU tests, one-fault references (``PERTURBED``) and the bounds (``TOL``)."""
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

from tests import clip_stages as S

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "clip_vision_tiny.npz")
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
VP = "vision_model."

TINY_VISION = dict(hidden_size=128, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, image_size=56, patch_size=14,
                   projection_dim=64, layer_norm_eps=1e-5)
TINY_TEXT = dict(vocab_size=1000, hidden_size=128, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2,
                 max_position_embeddings=77, layer_norm_eps=1e-5)
TINY_BOS, TINY_EOS = 998, 999

# (H, S) of the preprocessing cases: the production resize, two small downsamplings (one with a ratio that is no ratio of small
# integers), an upsampling and the identity
PREPROCESS_SIZES = ((256, 224), (64, 56), (40, 28), (32, 56), (224, 224))

# name -> (config, parameter kind, batch): the tower cases of the GPU test
TOWER_CASES = dict(
    tiny=(TINY_VISION, "golden", 3),                                                                           # 17 tokens; K 588 -> 640
    one_tile=(dict(TINY_VISION, image_size=28), "gelu_tail", 2),                                               # 5 tokens
    patch32=(dict(TINY_VISION, image_size=224, patch_size=32), "workflow", 2),                                 # 50 tokens; K 3072, no pad
    tokens257=(dict(TINY_VISION, image_size=224, num_hidden_layers=1), "workflow", 2),                         # 257 tokens
    tokens577=(dict(TINY_VISION, image_size=336, hidden_size=64, intermediate_size=256, num_attention_heads=1,
                    num_hidden_layers=1), "workflow", 2),                                                      # 577: streaming attention
    clip_l=(dict(hidden_size=1024, intermediate_size=4096, num_hidden_layers=2, num_attention_heads=16, image_size=224, patch_size=14,
                 projection_dim=768, layer_norm_eps=1e-5), "stress", 2),                                       # 257 tokens, CLIP-L width
)
SINK_HEAD, SHARP_HEAD = 1, 0
MASSIVE = (3, 40, 77, 120)          # stress set: channels of the class embedding at +-32


# ------------------------------------------------------------------------------------------------------------------ preprocessing
def keys_cubic(x, a=-0.5):
    x = x.abs()
    return torch.where(x < 1, ((a + 2) * x - (a + 3)) * x * x + 1, torch.where(x < 2, (((x - 5) * x + 8) * x - 4) * a, torch.zeros_like(x)))


def resize_matrix(H, S, antialias=True, align_corners=False, a=-0.5):
    """[S, H] float64: row o holds the weights of output pixel o.  Antialiased (the definition of uspace_clip_preprocess): Keys
    filter of support 2 max(H / S, 1) around (o + 0.5) H / S, the window clipped to the image and renormalised.  The two fault
    forms (``antialias=False``: support 2 at every ratio, border pixels replicated; ``align_corners=True``: centres o (H - 1) /
    (S - 1)) follow plain bicubic interpolation with the same filter."""
    W = torch.zeros(S, H, dtype=torch.float64)
    if antialias and not align_corners:
        scale = H / S
        support, inv = 2.0 * max(scale, 1.0), 1.0 / max(scale, 1.0)
        for o in range(S):
            c = scale * (o + 0.5)
            lo = max(int(c - support + 0.5), 0)
            hi = min(int(c + support + 0.5), H)
            j = torch.arange(lo, hi, dtype=torch.float64)
            w = keys_cubic((j - c + 0.5) * inv, a)
            W[o, lo:hi] = w / w.sum()
        return W
    for o in range(S):
        src = o * (H - 1) / (S - 1) if (align_corners and S > 1) else (o + 0.5) * H / S - 0.5
        f = math.floor(src)
        for t in range(-1, 3):
            w = float(keys_cubic(torch.tensor(src - (f + t), dtype=torch.float64), a))
            W[o, min(max(f + t, 0), H - 1)] += w
    return W


def preprocess(images, S_out, quantize=True, mean=CLIP_MEAN, std=CLIP_STD, antialias=True, align_corners=False):
    """images [B, 3, H, H] in [0, 1] -> pixel_values [B, 3, S, S] float64: Wy . (255 x, quantised) . Wx^T, clamp, / 255, mean / std.
    The quantisation is ``save_image``'s own fp32 arithmetic (x.mul(255).add_(0.5).clamp_(0, 255) -> uint8, what FIDStatistics
    applies): its result is an integer, and a tie decided in float64 instead would differ from the PNG by one grey level."""
    x = images.to(torch.float32) * 255.0
    if quantize:
        x = torch.floor(x + 0.5).clamp(0.0, 255.0)
    x = x.to(torch.float64)
    W = resize_matrix(images.shape[-1], S_out, antialias, align_corners)
    v = (W @ x @ W.T).clamp(0.0, 255.0) / 255.0
    m = torch.tensor(mean, dtype=torch.float32).to(torch.float64).view(1, 3, 1, 1)
    s = torch.tensor(std, dtype=torch.float32).to(torch.float64).view(1, 3, 1, 1)
    return (v - m) / s


def make_images(B, H, seed=0, kind="noise"):
    """[B, 3, H, H] fp32 in [0, 1]: sample 0 is noise (what separates antialiased from plain bicubic), the others smooth
    gradients plus mild texture; a few pixels sit outside [0, 1] and on the quantisation ties."""
    g = torch.Generator().manual_seed(1000 + seed * 7 + H)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, H), indexing="ij")
    out = torch.empty(B, 3, H, H)
    for b in range(B):
        for c in range(3):
            if b == 0 or kind == "noise":
                out[b, c] = torch.rand(H, H, generator=g)
            else:
                out[b, c] = 0.5 + 0.4 * torch.sin(3.0 * xx * (c + 1) + b) * torch.cos(2.0 * yy + c) + 0.05 * torch.randn(H, H, generator=g)
    out[:, :, 0, 0] = 1.07
    out[:, :, -1, -1] = -0.05
    out[:, 1, 1, 2] = 100.5 / 255.0
    return out.clamp(-0.1, 1.1)


# ------------------------------------------------------------------------------------------------------------------ the tower
def _bf(x, on):
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float64) if on else x


def _w(sd, name, tight):
    w = sd[name]
    return (w.to(torch.bfloat16) if tight else w).to(torch.float64)


def _v(sd, name):
    return sd[name].to(torch.float64)


def n_layers(sd, prefix=VP):
    n = 0
    while f"{prefix}encoder.layers.{n}.layer_norm1.weight" in sd:
        n += 1
    return n


def patch_rows(pv, p, order="cpp", swap_yx=False):
    """pixel_values [B, 3, S, S] -> rows [B, N, 3 p p] in (c, py, px) order (``order="ppc"``: (py, px, c); ``swap_yx``: (c, px, py))."""
    B, C, S_, _ = pv.shape
    G = S_ // p
    t = pv.reshape(B, C, G, p, G, p).permute(0, 2, 4, 1, 3, 5)          # b, gy, gx, c, py, px
    if swap_yx:
        t = t.transpose(-1, -2)
    if order == "ppc":
        t = t.permute(0, 1, 2, 4, 5, 3)
    return t.reshape(B, G * G, C * p * p)


def embeddings(pv, sd, mode, fault=None):
    """HF CLIPVisionEmbeddings: cat(class, conv(pixel_values)) + position table, [B, N + 1, D] float64."""
    t = mode == "tight"
    w = _w(sd, VP + "embeddings.patch_embedding.weight", t)
    D, p = w.shape[0], w.shape[-1]
    rows = _bf(patch_rows(pv.to(torch.float64), p, "ppc" if fault == "k_order_ppc" else "cpp", fault == "py_px_swapped"), t)
    pe = rows @ w.reshape(D, -1).T
    if fault == "pad_nonzero":           # the 52 pad columns of rows and weight read as 1 instead of 0 (ViT-L/14: K 588 -> 640)
        K = rows.shape[-1]
        pe = pe + float((K + 63) // 64 * 64 - K)
    cls = _v(sd, VP + "embeddings.class_embedding").expand(pv.shape[0], 1, D)
    pos = _v(sd, VP + "embeddings.position_embedding.weight")
    if fault == "pos_shifted":
        pos = torch.roll(pos, 1, dims=0)
    return torch.cat([cls, pe], 1) + pos


def _ln(x, sd, name, eps):
    return F.layer_norm(x, (x.shape[-1],), _v(sd, name + ".weight"), _v(sd, name + ".bias"), eps)


def attention(q, k, v, heads, tight, causal=False):
    """softmax(q k^T / 8) v per head; tight: P rounded to bf16, normalised by the sum of the rounded values, output rounded."""
    B, L, D = q.shape
    sh = lambda t: t.reshape(B, L, heads, D // heads).transpose(1, 2)
    s = sh(q) @ sh(k).transpose(-1, -2) / 8.0
    if causal:
        s = s.masked_fill(~torch.ones(L, L, dtype=torch.bool).tril(), float("-inf"))
    p = _bf(torch.exp(s - s.amax(-1, keepdim=True)), tight)
    o = (p @ sh(v)) / p.sum(-1, keepdim=True)
    return _bf(o.transpose(1, 2).reshape(B, L, D), tight)


def layer(x, sd, i, mode, heads, eps=1e-5, fault=None, prefix=VP):
    t = mode == "tight"
    pre = f"{prefix}encoder.layers.{i}."
    x = x.to(torch.float64)
    lin = lambda a, n: a @ _w(sd, pre + n + ".weight", t).T + _v(sd, pre + n + ".bias")
    h = _bf(_ln(x, sd, pre + "layer_norm1", eps), t)
    q, k, v = (_bf(lin(h, f"self_attn.{n}_proj"), t) for n in "qkv")
    x = x + lin(attention(q, k, v, heads, t, causal=fault == "causal"), "self_attn.out_proj")
    h = _bf(_ln(x, sd, pre + "layer_norm2", eps), t)
    f1 = _bf(lin(h, "mlp.fc1"), t)
    act = F.gelu(f1) if fault == "erf_gelu" else S.quick_gelu(f1)
    return x + lin(_bf(act, t), "mlp.fc2")


def pooled(x, sd, eps=1e-5, fault=None):
    tok = x.to(torch.float64).mean(1) if fault == "pool_mean" else x.to(torch.float64)[:, 0]
    return _ln(tok, sd, VP + "post_layernorm", eps)


def vision_forward(pv, sd, heads, mode="loose", eps=1e-5, fault=None):
    """-> dict(embeddings, hidden=[after pre_layrnorm, after layer 1, ...], pooler_output, image_embeds), float64."""
    e = embeddings(pv, sd, mode, fault)
    x = e if fault == "no_pre_ln" else _ln(e, sd, VP + "pre_layrnorm", eps)
    hidden = [x]
    for i in range(n_layers(sd)):
        x = layer(x, sd, i, mode, heads, eps, fault)
        hidden.append(x)
    po = pooled(x, sd, eps, fault)
    return dict(embeddings=e, hidden=hidden, pooler_output=po, image_embeds=po @ _v(sd, "visual_projection.weight").T)


# ------------------------------------------------------------------------------------------------------------------ text side, score
def text_sd(sd):
    """The text tower's entries of a CLIPModel state dict without their prefix (the names tests/clip_stages.py reads)."""
    return {k[len("text_model."):]: v for k, v in sd.items() if k.startswith("text_model.")}


def pooled_index(ids, eos_token_id=None, fault=None):
    ids = torch.as_tensor(ids, dtype=torch.long)
    if fault == "pool_last":
        return torch.full((ids.shape[0],), ids.shape[1] - 1, dtype=torch.long)
    if eos_token_id is None or eos_token_id == 2:
        return ids.argmax(-1)
    return (ids == eos_token_id).int().argmax(-1)


def text_embeds(last_hidden, ids, w_proj, eos_token_id=None, fault=None):
    idx = pooled_index(ids, eos_token_id, fault)
    return last_hidden.to(torch.float64)[torch.arange(ids.shape[0]), idx] @ w_proj.to(torch.float64).T


def text_forward(ids, sd, heads, mode="loose", eps=1e-5):
    """last_hidden_state float64 of the text tower in a CLIPModel state dict."""
    return S.forward(ids, text_sd(sd), mode, heads, eps, taps=False)[0]


def cosine(a, b, fault=None):
    a, b = a.to(torch.float64), b.to(torch.float64)
    if fault == "cos_unnormalised":
        return (a * b).sum(-1)
    return (a * b).sum(-1) / (a.norm(dim=-1) * b.norm(dim=-1))


def clip_score(a, b):
    return 100.0 * cosine(a, b).clamp_min(0.0)


def directional(e_src, e_edit, t_src, t_edit):
    n = lambda z: z.to(torch.float64) / z.to(torch.float64).norm(dim=-1, keepdim=True)
    return cosine(n(e_edit) - n(e_src), n(t_edit) - n(t_src))


def rel(got, ref):
    got, ref = torch.as_tensor(got).to(torch.float64), torch.as_tensor(ref).to(torch.float64)
    return float((got - ref).norm() / ref.norm())


def maxabs(got, ref):
    return float((torch.as_tensor(got).to(torch.float64) - torch.as_tensor(ref).to(torch.float64)).abs().max())


# ------------------------------------------------------------------------------------------------------------------ parameters
def vision_params(kind="workflow", seed=0, hidden_size=128, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2,
                  image_size=56, patch_size=14, projection_dim=64, **_ignored):
    """Seeded fp32 parameters in the HF CLIPVisionModelWithProjection state_dict order.  "workflow": every branch moves the
    residual stream by a sizeable fraction of its size; norms, biases non-trivial.  "stress": the same plus a massive class
    token (channels MASSIVE of the class embedding at +-32), head SINK_HEAD whose logits for the class token's key stand far above
    the others, and head SHARP_HEAD with 4x sharper logits.  "gelu_tail": the workflow set with every fc1 bias lowered by 2, so the MLP
    output comes from the activation's negative tail, where quick-GELU and erf-GELU differ by tens of percent."""
    g = torch.Generator().manual_seed(seed)
    D, Fd, T = hidden_size, intermediate_size, (image_size // patch_size) ** 2 + 1
    K = 3 * patch_size * patch_size
    rn = lambda *s: torch.randn(*s, generator=g)
    sd = {VP + "embeddings.class_embedding": rn(D) * 0.5,
          VP + "embeddings.patch_embedding.weight": rn(D, 3, patch_size, patch_size) * (0.7 / K ** 0.5),
          VP + "embeddings.position_embedding.weight": rn(T, D) * 0.3,
          VP + "pre_layrnorm.weight": 1.0 + 0.2 * rn(D), VP + "pre_layrnorm.bias": 0.1 * rn(D)}
    for i in range(num_hidden_layers):
        pre = f"{VP}encoder.layers.{i}."
        gain = 1.0 + 0.1 * i
        for n, s in (("k", 1.4), ("v", 1.0), ("q", 1.4), ("out", 0.45 * gain)):
            sd[pre + f"self_attn.{n}_proj.weight"] = rn(D, D) * (s / D ** 0.5)
            sd[pre + f"self_attn.{n}_proj.bias"] = rn(D) * 0.1
        sd[pre + "layer_norm1.weight"] = 1.0 + 0.2 * rn(D)
        sd[pre + "layer_norm1.bias"] = 0.1 * rn(D)
        sd[pre + "mlp.fc1.weight"] = rn(Fd, D) * (1.0 / D ** 0.5)
        sd[pre + "mlp.fc1.bias"] = rn(Fd) * 0.3
        sd[pre + "mlp.fc2.weight"] = rn(D, Fd) * (0.6 * gain / Fd ** 0.5)
        sd[pre + "mlp.fc2.bias"] = rn(D) * 0.1
        sd[pre + "layer_norm2.weight"] = 1.0 + 0.2 * rn(D)
        sd[pre + "layer_norm2.bias"] = 0.1 * rn(D)
    sd[VP + "post_layernorm.weight"] = 1.0 + 0.2 * rn(D)
    sd[VP + "post_layernorm.bias"] = 0.1 * rn(D)
    sd["visual_projection.weight"] = rn(projection_dim, D) * (1.0 / D ** 0.5)
    if kind == "gelu_tail":
        for i in range(num_hidden_layers):
            sd[f"{VP}encoder.layers.{i}.mlp.fc1.bias"] -= 2.0
    if kind == "stress":
        sign = torch.tensor([1.0, -1.0, 1.0, -1.0])
        sd[VP + "embeddings.class_embedding"][list(MASSIVE)] = 32.0 * sign
        e = rn(64)
        e = e / e.norm()
        for i in range(num_hidden_layers):
            pre = f"{VP}encoder.layers.{i}."
            rows = slice(SINK_HEAD * 64, (SINK_HEAD + 1) * 64)
            wk = sd[pre + "self_attn.k_proj.weight"]
            wk[rows] *= 0.25
            wk[rows][:, list(MASSIVE)] += 1.3 * e[:, None] * sign[None, :]
            sd[pre + "self_attn.q_proj.bias"][rows] = 4.0 * e
            sd[pre + "self_attn.q_proj.weight"][rows] *= 0.25
            rows = slice(SHARP_HEAD * 64, (SHARP_HEAD + 1) * 64)
            sd[pre + "self_attn.q_proj.weight"][rows] *= 4.0
            sd[pre + "self_attn.q_proj.bias"][rows] *= 4.0
    return sd


def tiny_ids(n=3, seed=0, L=77):
    """Prompt-shaped ids for the tiny text tower: BOS, words, EOS padding (EOS is the largest id: HF's argmax pooling finds the first)."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.full((n, L), TINY_EOS, dtype=torch.long)
    ids[:, 0] = TINY_BOS
    for r in range(n):
        w = (3 + 5 * r) % (L - 2) + 1
        ids[r, 1:1 + w] = torch.randint(0, TINY_BOS, (w,), generator=g)
    return ids


# ------------------------------------------------------------------------------------------------------------------ the golden
def load_golden():
    """tests/golden/clip_vision_tiny.npz -> (arrays, state dict).  The parameters are stored as small integer codes with a
    power-of-two step and an offset per tensor (what keeps the file small); value = offset + step * code, exact in fp32."""
    z = np.load(GOLDEN)
    names = [str(n) for n in z["param_names"]]
    sd = {}
    for i, n in enumerate(names):
        sd[n] = (float(z["param_offset"][i]) + float(z["param_step"][i]) * torch.from_numpy(z[f"param_{i}"].astype(np.float32))).float()
    return z, sd


def case_seed(name):
    return 300 + list(TOWER_CASES).index(name)


def case_params(name):
    """The state dict of a tower case (the golden's vision entries for "tiny")."""
    cfg, kind, _B = TOWER_CASES[name]
    if kind == "golden":
        return {k: v for k, v in load_golden()[1].items() if k.startswith((VP, "visual_projection"))}
    return vision_params(kind, seed=case_seed(name), **cfg)


def case_pixels(name):
    cfg, kind, B = TOWER_CASES[name]
    if kind == "golden":
        return torch.from_numpy(load_golden()[0]["pixel_values"])
    g = torch.Generator().manual_seed(7000 + case_seed(name))
    return torch.randn(B, 3, cfg["image_size"], cfg["image_size"], generator=g) * 1.2


class StubTokenizer:
    """Called like the HF CLIPTokenizer by CLIPScore: words -> ids of the tiny vocabulary (a fixed hash), BOS in front, EOS padding."""

    def __init__(self, bos=TINY_BOS, eos=TINY_EOS):
        self.bos, self.eos, self.calls = bos, eos, 0

    def word_id(self, w):
        return sum((i + 1) * 131 * ord(ch) for i, ch in enumerate(w)) % self.bos

    def __call__(self, text, truncation=True, max_length=77, padding="max_length", return_tensors="pt", **_kw):
        self.calls += 1
        rows = []
        for t in ([text] if isinstance(text, str) else text):
            ids = [self.bos] + [self.word_id(w) for w in t.split()][:max_length - 2]
            rows.append(ids + [self.eos] * (max_length - len(ids)))
        return {"input_ids": torch.tensor(rows, dtype=torch.long)}


# ------------------------------------------------------------------------------------------------------------------ faults
# name -> (metric the fault must show in, what it does).  The host test builds every faulty reference on the data set meant to
# expose it and requires its distance from the true reference, in that metric, to be at least twice the metric's TOL entry.
PERTURBED = dict(
    pos_shifted=("embeddings", "position table shifted by one row"),
    py_px_swapped=("embeddings", "(py, px) swapped inside a patch"),
    k_order_ppc=("embeddings", "patch K order (py, px, c) instead of (c, py, px)"),
    pad_nonzero=("embeddings", "pad columns of the patch rows nonzero"),
    no_pre_ln=("hidden", "pre_layrnorm skipped"),
    pool_mean=("pooler", "post_layernorm on the token mean instead of token 0"),
    causal=("update", "causal mask in the tower"),
    erf_gelu=("update", "erf-GELU instead of quick-GELU"),
    pool_last=("text_embeds", "text pooled at position L - 1"),
    cos_unnormalised=("cosine", "cosine without normalisation"),
    no_antialias=("preprocess", "resize without antialias"),
    align_corners=("preprocess", "align_corners=True"),
    mean_std_reversed=("preprocess", "mean and std channel order reversed"),
    no_quantize=("preprocess", "no input quantisation"),
)

# GPU bounds: 3x the worst value an MI355X measured against the float64 model (the convention of tests/attention_map_cases.py);
# the measured value and the case that produced it stand beside each.  rel-L2 unless it says otherwise.
TOL = dict(
    preprocess=2.3e-4,         # measured 7.66e-5 (256 -> 224, quantize on; 7.63e-5 off; 1.5e-5 at 64 -> 56, 4.2e-7 at 224 -> 224): max abs of
                               # pixel_values, whose unit is 1 / std = 3.7 -- 0.005 grey levels; the clipped border windows 6.5e-5
    embeddings=6.6e-3,         # measured 2.21e-3 (tokens257; 0 on the golden, whose values are exact in bf16): vs the loose model, the
                               # bf16 rounding of the patch rows and the patch weight
    embeddings_tight=9.5e-7,   # measured 3.15e-7 (patch32, K = 3072): vs the model with those two roundings, fp32 accumulation left
    hidden=1.14e-2,            # measured 3.80e-3 (clip_l, after layer 2; 2.2e-3 after pre_layrnorm everywhere): vs the loose model from the pixels
    update=4.4e-3,             # measured 1.46e-3 (tokens577, the streaming attention kernel; 9.9e-4 clip_l, 2.4e-4 tokens257):
                               # ||T_k - layer(T_{k-1}, tight)|| / ||T_k - T_{k-1}|| from the GPU's own previous tap
    pooler=2.3e-7,             # measured 7.52e-8 (tokens577): post_layernorm of token 0 vs float64 of the GPU's last tap
    image_embeds=9.2e-3,       # measured 3.07e-3 (clip_l): vs the loose model from the pixels
    text_embeds=7.6e-3,        # measured 2.54e-3 (golden ids; 2.9e-3 is the worse of both features in the score test, printed there)
    cosine=2.9e-3,             # measured 9.65e-4 (score test, tiny towers; 2.7e-4 on the golden's 3 x 3 matrix): absolute, end to end
    score=0.29,                # measured 9.65e-2 (the same pairs): absolute, of 100
    directional=7.3e-3,        # measured 2.42e-3: absolute; differences of unit vectors amplify the towers' error
    linear=3.4e-7,             # measured 1.12e-7 (clip_l's visual_projection, K = 1024; 9.96e-8 on random operands): uspace_linear_f32 vs float64
    cosine_op=5.5e-7,          # measured 1.83e-7 (B = 1, D = 768): uspace_cosine_f32 / uspace_normalized_diff_f32 vs float64 on fp32 inputs, absolute
)
