"""float64 restatement of the attribute-classifier tower of csrc/resnet.hip, written from the published architecture (the
torchvision-layout ResNet: He et al. 2015, the stride on the bottleneck's 3 x 3) with torch's CPU F.conv2d, one function per stage
as ``uspace_resnet_tap`` numbers them, the fc head, and the edit-effect columns of tools/attr_metrics.py in numpy.  It holds the
model, the planted faults and the measures; the cases and the tolerances are in tests/resnet_cases.py.  Not a test.

All maps are NCHW here (``nhwc`` / ``nchw`` convert).  ``stage(sd, arch, s, x)`` maps the output of stage s - 1 to stage s: 0 the
stem after the max pool (from the images in [0, 1]), 1 + u block u, 1 + U the pooled vector; ``logits(sd, pooled)`` is the head.
``dtype=torch.float32`` runs the same statements in fp32: the restatement that shows a bound is reachable by fp32 arithmetic.
``fault=`` plants one entry of ``FAULTS``; with None the model is bit-equal to itself."""
import json
import os
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resnet_tiny.npz")
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)

Arch = namedtuple("Arch", "block layers planes stem mean std", defaults=(IMAGENET_MEAN, IMAGENET_STD))

# name -> (the kind of stage whose bound must catch it, what is planted).  tests/test_resnet_host.py ties each to a stage and an
# input and requires the deviation there to be at least 10 x that stage's GPU bound.
FAULTS = {
    "norm_after_padding": ("stem", "mean / std folded into conv1: the zero padding is normalised too"),
    "maxpool_pad_0": ("tower", "max pool 3 x 3 stride 2 without its padding (the map shrinks: judged on the logits)"),
    "maxpool_ceil": ("tower", "max pool in ceil mode (an even map gains a row and a column: judged on the logits)"),
    "bn_eps_1e-3": ("block", "batch norm eps 1e-3 instead of 1e-5"),
    "stride_on_first_1x1": ("block", "the bottleneck's stride on its first 1 x 1 instead of the 3 x 3 (the v1 form)"),
    "relu_before_add": ("block", "ReLU on the branch before the residual add, none after"),
    "shortcut_without_bn": ("block", "downsample.0 without downsample.1"),
    "avgpool_padded_count": ("pooled", "the pixel sum divided by the count rounded up to a multiple of 64"),
    "fc_bias_omitted": ("logits", "fc without its bias"),
}


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


# ------------------------------------------------------------------------------------------------------------------ cases
def smooth_images(n, h, w, seed):
    """Images in [0, 1]: a 7 x 7 Gaussian field upsampled bilinearly plus 0.1 Gaussian noise, scaled into the range and clamped."""
    g = torch.Generator().manual_seed(seed)
    field = F.interpolate(torch.randn(n, 3, 7, 7, generator=g, dtype=torch.float64), size=(h, w), mode="bilinear", align_corners=False)
    x = field + 0.1 * torch.randn(n, 3, h, w, generator=g, dtype=torch.float64)
    return (0.5 + 0.25 * x).clamp(0, 1).float()


def perturbed(x, amplitude, seed):
    """A copy of x moved by ``amplitude`` times another smooth image's deviation from grey (clamped to [0, 1])."""
    other = smooth_images(x.shape[0], x.shape[2], x.shape[3], seed)
    return (x + amplitude * (other - 0.5)).clamp(0, 1)


def golden(name):
    """(arch, state dict under torchvision keys, npz) of the golden model ``name`` ("bottleneck" or "basic")."""
    z = np.load(GOLDEN)
    cfg = json.loads(str(z[f"{name}_config"]))
    exp = 4 if cfg["layer_type"] == "bottleneck" else 1
    arch = Arch(cfg["layer_type"], tuple(cfg["depths"]), tuple(h // exp for h in cfg["hidden_sizes"]), cfg["embedding_size"],
                tuple(float(v) for v in z["mean"]), tuple(float(v) for v in z["std"]))
    sd = {}
    for i, key in enumerate(json.loads(str(z[f"{name}_keys"]))):
        if f"{name}_w{i}_int" in z:
            sd[key] = torch.tensor(int(z[f"{name}_w{i}_int"]), dtype=torch.long)
        else:
            off, step = z[f"{name}_w{i}_affine"]
            sd[key] = (off + step * torch.from_numpy(z[f"{name}_w{i}_code"]).double()).float()
    return arch, sd, z


def block_specs(arch):
    """[(prefix, in, planes, out, stride, downsample)] of the blocks ``layer1.0`` .."""
    exp = 4 if arch.block == "bottleneck" else 1
    out, cin = [], arch.stem
    for l, (p, n) in enumerate(zip(arch.planes, arch.layers)):
        for j in range(n):
            s = 2 if (j == 0 and l > 0) else 1
            out.append((f"layer{l + 1}.{j}", cin, p, p * exp, s, s != 1 or cin != p * exp))
            cin = p * exp
    return out


# ----------------------------------------------------------------------------------------------------------------- tower
def _p(sd, key, dtype):
    return torch.as_tensor(sd[key]).to(dtype)


def bn(sd, prefix, x, fault=None):
    eps = 1e-3 if fault == "bn_eps_1e-3" else 1e-5
    d = x.dtype
    s = _p(sd, prefix + ".weight", d) / torch.sqrt(_p(sd, prefix + ".running_var", d) + eps)
    return (x - _p(sd, prefix + ".running_mean", d).reshape(1, -1, 1, 1)) * s.reshape(1, -1, 1, 1) + _p(sd, prefix + ".bias", d).reshape(1, -1, 1, 1)


def normalize(arch, x):
    d = x.dtype
    return (x - torch.tensor(arch.mean, dtype=d).reshape(1, 3, 1, 1)) / torch.tensor(arch.std, dtype=d).reshape(1, 3, 1, 1)


def stem(sd, arch, images, fault=None):
    """images [B, 3, H, W] in [0, 1] -> the stem after the max pool."""
    w = _p(sd, "conv1.weight", images.dtype)
    if fault == "norm_after_padding":      # what folding mean / std into conv1 computes: the padding is normalised too
        y = F.conv2d(normalize(arch, F.pad(images, (3, 3, 3, 3))), w, None, 2, 0)
    else:
        y = F.conv2d(normalize(arch, images), w, None, 2, 3)
    y = torch.relu(bn(sd, "bn1", y, fault))
    return F.max_pool2d(y, 3, 2, 0 if fault == "maxpool_pad_0" else 1, ceil_mode=fault == "maxpool_ceil")


def block(sd, arch, spec, x, fault=None):
    prefix, _cin, _p_, _cout, s, ds = spec
    d = x.dtype
    conv = lambda name, t, stride, pad: F.conv2d(t, _p(sd, f"{prefix}.{name}.weight", d), None, stride, pad)
    if arch.block == "bottleneck":
        s1, s2 = (s, 1) if fault == "stride_on_first_1x1" else (1, s)
        y = torch.relu(bn(sd, prefix + ".bn1", conv("conv1", x, s1, 0), fault))
        y = torch.relu(bn(sd, prefix + ".bn2", conv("conv2", y, s2, 1), fault))
        y = bn(sd, prefix + ".bn3", conv("conv3", y, 1, 0), fault)
    else:
        y = torch.relu(bn(sd, prefix + ".bn1", conv("conv1", x, s, 1), fault))
        y = bn(sd, prefix + ".bn2", conv("conv2", y, 1, 1), fault)
    if ds:
        sc = conv("downsample.0", x, s, 0)
        if fault != "shortcut_without_bn":
            sc = bn(sd, prefix + ".downsample.1", sc, fault)
    else:
        sc = x
    return torch.relu(y) + sc if fault == "relu_before_add" else torch.relu(y + sc)


def pooled(x, fault=None):
    """[B, C, h, w] -> [B, C]: the mean over the pixels."""
    hw = x.shape[2] * x.shape[3]
    count = -(-hw // 64) * 64 if fault == "avgpool_padded_count" else hw
    return x.flatten(2).sum(2) / count


def logits(sd, pool, fault=None):
    z = pool @ _p(sd, "fc.weight", pool.dtype).T
    return z if fault == "fc_bias_omitted" else z + _p(sd, "fc.bias", pool.dtype)


def n_stages(arch):
    """Stages 0 .. n_stages - 1 of the tap: the stem, the blocks, the pooled vector."""
    return sum(arch.layers) + 2


def stage_kind(arch, s):
    return "stem" if s == 0 else ("pooled" if s == n_stages(arch) - 1 else "block")


def stage(sd, arch, s, x, fault=None, dtype=torch.float64):
    """Output of tap stage s from the output of stage s - 1 (stage 0: from the images in [0, 1]), NCHW."""
    x = torch.as_tensor(x).to(dtype)
    specs = block_specs(arch)
    if s == 0:
        return stem(sd, arch, x, fault)
    if s <= len(specs):
        return block(sd, arch, specs[s - 1], x, fault)
    return pooled(x, fault)


def forward(sd, arch, images, fault=None, dtype=torch.float64):
    """images in [0, 1] -> (logits [B, A], [the output of stage s for s = 0 .. n_stages - 1])."""
    x, outs = images, []
    for s in range(n_stages(arch)):
        x = stage(sd, arch, s, x, fault, dtype)
        outs.append(x)
    return logits(sd, x, fault), outs


# --------------------------------------------------------------------------------------------------------------- the effect
def effect_columns(za, zb, target, sign, sigma=None):
    """fp64 numpy [B, 4]: target_shift, target_hit, off_target, selectivity from logits [B, A], as tools/attr_metrics.py defines
    them, the sums in attribute order."""
    za, zb = np.asarray(za, np.float64), np.asarray(zb, np.float64)
    B, A = za.shape
    sigma = np.ones(A) if sigma is None else np.asarray(sigma, np.float64)
    out = np.zeros((B, 4))
    for b in range(B):
        t, sg = int(target[b]), float(sign[b])
        off = 0.0
        for j in range(A):
            if j != t:
                off += abs(zb[b, j] - za[b, j]) / sigma[j]
        hit = abs(zb[b, t] - za[b, t]) / sigma[t]
        out[b] = (sg * (zb[b, t] - za[b, t]), 1.0 if sg * zb[b, t] > 0 else 0.0, off / (A - 1) if A > 1 else 0.0,
                  hit / (hit + off) if hit + off > 0 else 0.0)
    return out


# --------------------------------------------------------------------------------------------------------------- measures
def rel_l2(got, want):
    """|got - want| / |want| per sample (dim 0), float64."""
    got, want = torch.as_tensor(got).double().flatten(1), torch.as_tensor(want).double().flatten(1)
    return (got - want).norm(dim=1) / want.norm(dim=1)
