"""SegFormer restated in float64, stage by stage (``transformers``' SegformerForSemanticSegmentation in eval mode; the kernels are
csrc/segformer.hip and csrc/attention_kv.hip), with planted faults.  A helper of tests/test_segformer_host.py and
tests/test_gpu_segformer.py, not a test.

``arch``: dict(hidden, depths, heads, sr, mlp, D, L, eps=dict(embed, block, sr, stage, bn)).  ``sd``: the state dict (float64
tensors).  Maps are NHWC.  The tap stages are those of ``uspace_segformer_tap``: per encoder stage the patch embedding after its
LayerNorm, every block, the closing norm; then the concatenation, the fused map, the logits.  ``step`` computes one tap stage from
the stages in front of it, so a GPU stage can be judged from the GPU's own inputs.

``rnd=True`` is the working precision of the kernels: the operands of the five linears of a block rounded to bf16 (activations and
weights), q, k | v, the attention output, fc1's output and the dwconv / GELU output stored in bf16, P rounded to bf16; everything
else (the residual stream, the convolutions, the head) is left in float64, where the kernels have fp32.

FAULTS, each what a subtly wrong kernel would compute: the concatenation not reversed; ``align_corners=True``; the sr convolution
padded up instead of dropping trailing rows; the sr LayerNorm left out; 1 / sqrt(C) in place of 1 / 8; the dwconv bias left out;
GELU in front of the dwconv; batch norm eps 1e-3; argmax taking the highest index on ties; the patch embeddings' and the blocks'
LayerNorm epsilons swapped (the identity on a net whose LayerNorms all hold one epsilon, as the installed ``transformers`` modules
do: it is judged on the net ``segformer_cases`` builds with a different epsilon for every kind, and ``eps_for`` also gives any other
mis-wiring of the five epsilon fields).

Every function computes in the dtype of what it is given: float64 tensors give the reference, float32 tensors (``as_f32``) the
same statements in the kernels' own fp32."""
import math

import numpy as np
import torch
import torch.nn.functional as F

FAULTS = ("concat_not_reversed", "align_corners", "sr_padded", "sr_norm_omitted", "scale_1/sqrtC", "dwconv_bias_omitted",
          "gelu_before_dwconv", "bn_eps_1e-3", "argmax_highest", "eps_swapped")
EPS_KINDS = ("embed", "block", "sr", "stage", "bn")


def eps_for(arch, kind, fault=None):
    """The epsilon of a kind of norm.  'eps_swapped' exchanges embed and block; 'eps:a>b' puts kind a's epsilon where kind b's
    belongs (a mis-wired config field)."""
    if fault == "eps_swapped":
        kind = {"embed": "block", "block": "embed"}.get(kind, kind)
    elif fault and fault.startswith("eps:"):
        a, b = fault[4:].split(">")
        kind = a if kind == b else kind
    return arch["eps"][kind]


def as_f32(sd):
    return {k: v.to(torch.float32) for k, v in sd.items()}


def _bf(x, rnd):
    return x.to(torch.bfloat16).to(x.dtype) if rnd else x


def _ln(x, sd, name, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * sd[name + ".weight"] + sd[name + ".bias"]


def _lin(x, sd, name, rnd):
    return _bf(x, rnd) @ _bf(sd[name + ".weight"], rnd).t() + sd[name + ".bias"]


def _conv(x, sd, name, stride, padding, groups=1, bias=True):
    y = F.conv2d(x.permute(0, 3, 1, 2), sd[name + ".weight"], sd[name + ".bias"] if bias else None, stride, padding, groups=groups)
    return y.permute(0, 2, 3, 1)


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def normalise(images, mean, std):
    """images [B, 3, H, W] in [0, 1] -> float64 NHWC, (x - mean) / std."""
    x = images.to(torch.float64)
    m, s = (torch.tensor(v, dtype=torch.float64).view(1, 3, 1, 1) for v in (mean, std))
    return ((x - m) / s).permute(0, 2, 3, 1).contiguous()


def patch_embed(sd, arch, i, x, fault=None):
    p = f"segformer.stages.{i}.patch_embeddings"
    y = _conv(x, sd, p + ".proj", 4 if i == 0 else 2, 3 if i == 0 else 1)
    return _ln(y, sd, p + ".layer_norm", eps_for(arch, "embed", fault))


def block(sd, arch, i, j, x, rnd=False, fault=None):
    B, h, w, C = x.shape
    H, sr = arch["heads"][i], arch["sr"][i]
    p = f"segformer.stages.{i}.blocks.{j}"
    t = x.reshape(B, h * w, C)
    n1 = _ln(t, sd, p + ".layernorm_before", eps_for(arch, "block", fault))
    q = _bf(_lin(n1, sd, p + ".attention.q_proj", rnd), rnd)
    kin = n1
    if sr > 1:
        m = n1.reshape(B, h, w, C)
        if fault == "sr_padded":
            m = F.pad(m, (0, 0, 0, -w % sr, 0, -h % sr))
        kin = _conv(m, sd, p + ".attention.sequence_reduction.sequence_reduction", sr, 0).reshape(B, -1, C)
        if fault != "sr_norm_omitted":
            kin = _ln(kin, sd, p + ".attention.sequence_reduction.layer_norm", eps_for(arch, "sr", fault))
    k = _bf(_lin(kin, sd, p + ".attention.k_proj", rnd), rnd)
    v = _bf(_lin(kin, sd, p + ".attention.v_proj", rnd), rnd)
    qh, kh, vh = (u.reshape(B, -1, H, 64).permute(0, 2, 1, 3) for u in (q, k, v))
    s = qh @ kh.transpose(-1, -2) / (math.sqrt(C) if fault == "scale_1/sqrtC" else 8.0)
    pr = _bf(torch.exp(s - s.amax(-1, keepdim=True)), rnd)
    o = _bf(((pr @ vh) / pr.sum(-1, keepdim=True)).permute(0, 2, 1, 3).reshape(B, h * w, C), rnd)
    t = t + _lin(o, sd, p + ".attention.o_proj", rnd)
    n2 = _ln(t, sd, p + ".layernorm_after", eps_for(arch, "block", fault))
    f1 = _bf(_lin(n2, sd, p + ".mlp.fc1", rnd), rnd).reshape(B, h, w, -1)
    if fault == "gelu_before_dwconv":
        f1 = gelu(f1)
    d = _conv(f1, sd, p + ".mlp.dwconv.dwconv", 1, 1, groups=f1.shape[-1], bias=fault != "dwconv_bias_omitted")
    if fault != "gelu_before_dwconv":
        d = gelu(d)
    t = t + _lin(_bf(d, rnd).reshape(B, h * w, -1), sd, p + ".mlp.fc2", rnd)
    return t.reshape(B, h, w, C)


def stage_norm(sd, arch, i, x, fault=None):
    return _ln(x, sd, f"segformer.stages.{i}.layer_norm", eps_for(arch, "stage", fault))


def concat(sd, arch, stage_outs, fault=None):
    h0, w0 = stage_outs[0].shape[1:3]
    maps = []
    for i, so in enumerate(stage_outs):
        y = so @ sd[f"decode_head.linear_projections.{i}.proj.weight"].t() + sd[f"decode_head.linear_projections.{i}.proj.bias"]
        y = F.interpolate(y.permute(0, 3, 1, 2), size=(h0, w0), mode="bilinear", align_corners=fault == "align_corners")
        maps.append(y.permute(0, 2, 3, 1))
    return torch.cat(maps if fault == "concat_not_reversed" else maps[::-1], -1)


def fused(sd, arch, cat, fault=None):
    y = cat @ sd["decode_head.linear_fuse.weight"][:, :, 0, 0].t()
    eps = 1e-3 if fault == "bn_eps_1e-3" else eps_for(arch, "bn", fault)
    bn = "decode_head.batch_norm."
    y = (y - sd[bn + "running_mean"]) / torch.sqrt(sd[bn + "running_var"] + eps) * sd[bn + "weight"] + sd[bn + "bias"]
    return torch.relu(y)


def logits(sd, arch, fz):
    return fz @ sd["decode_head.classifier.weight"][:, :, 0, 0].t() + sd["decode_head.classifier.bias"]


def stage_index(arch):
    """[(kind, i, j)] of the tap stages in order: ('embed', i), ('block', i, j), ('norm', i), ('concat',), ('fused',), ('logits',)."""
    out = []
    for i in range(4):
        out.append(("embed", i, 0))
        out += [("block", i, j) for j in range(arch["depths"][i])]
        out.append(("norm", i, 0))
    return out + [("concat", 0, 0), ("fused", 0, 0), ("logits", 0, 0)]


def step(sd, arch, k, x_nhwc, taps, rnd=False, fault=None):
    """Tap stage k from ``taps`` (a list: the stages in front of it, float64 NHWC; ``x_nhwc`` the normalised image)."""
    idx = stage_index(arch)
    kind, i, j = idx[k]
    if kind == "embed":
        return patch_embed(sd, arch, i, x_nhwc if i == 0 else taps[k - 1], fault)
    if kind == "block":
        return block(sd, arch, i, j, taps[k - 1], rnd, fault)
    if kind == "norm":
        return stage_norm(sd, arch, i, taps[k - 1], fault)
    if kind == "concat":
        return concat(sd, arch, [taps[n] for n, e in enumerate(idx) if e[0] == "norm"], fault)
    if kind == "fused":
        return fused(sd, arch, taps[k - 1], fault)
    return logits(sd, arch, taps[k - 1])


def forward(sd, arch, x_nhwc, rnd=False, fault=None):
    """Every tap stage, each from the one in front of it: a list of float64 NHWC tensors, the logits last."""
    taps = []
    for k in range(len(stage_index(arch))):
        taps.append(step(sd, arch, k, x_nhwc, taps, rnd, fault))
    return taps


def labels(logits_nhwc, H, W, fault=None):
    """(labels uint8 [B, H, W], margin float64 [B, H, W]): bilinear resize (align_corners=False; with the 'align_corners' fault,
    True) and argmax with the lowest index on ties (the highest with 'argmax_highest'); the margin between the two largest."""
    z = F.interpolate(logits_nhwc.permute(0, 3, 1, 2), size=(H, W), mode="bilinear", align_corners=fault == "align_corners")
    z = z.permute(0, 2, 3, 1).numpy()
    if fault == "argmax_highest":
        lab = z.shape[-1] - 1 - np.argmax(z[..., ::-1], axis=-1)
    else:
        lab = np.argmax(z, axis=-1)
    top2 = np.partition(z, -2, axis=-1)[..., -2:]
    return lab.astype(np.uint8), top2[..., 1] - top2[..., 0]


def rel_l2(got, ref):
    got, ref = (np.asarray(t, dtype=np.float64) for t in (got, ref))
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-300))
