"""The segmentation operators of csrc/segformer.hip and the consistency metric of tools/seg_metrics.py: float64 restatements, the
cases and the bounds.  Shared by tests/test_segops_host.py (no GPU: the restatements against torch's own float64 operators and
hand-made label maps) and tests/test_gpu_segops.py / tests/test_gpu_seg_metrics.py.

Bounds.  None of them is measured: each is derived below from the number formats and the kernel's stated arithmetic, and the
GPU tests print the worst figure beside it.

* ``bilinear``: the kernel forms tap indices in integers (exact) and each weight l = rem / (2 out) with one fp32 rounding; 1 - l,
  the two products and the three fmas round once each.  Propagated through (1 - ly)((1 - lx) a + lx b) + ly(...) with weights
  summing to 1, that is at most 9 roundings of u = 2^-24 relative to M = max |neighbour|; the bound is 16 u M (``BILINEAR_ULPS``).
* ``dwconv``: fp32 accumulation of bias + 9 products (10 roundings, relative to S = |bias| + sum |w x|), through a GELU whose slope
  is at most 1.13 and whose polynomial is within 4.1e-7 + 1e-6 |v| of erf's (csrc/common.h), then one rounding to bf16: half an ulp,
  2^-8 |y| (1 + 2^-8) (bf16 keeps 8 significant bits), on top of the error E in front of it.  ``dwconv_bound`` returns that per element.
* ``labels``: equal to the float64 argmax wherever the float64 top-two margin exceeds 1e-5 times the largest |logit| (32 u M is
  4e-6 M: twice the bilinear bound), and at most 0.1 % of the pixels may lie under that margin.
* counts are integers and must be equal; the region sum is fp64 in another order than numpy's: 4e-16 relative per addition level is
  far below ``SSE_RTOL`` = 1e-12, and the pixel count must be equal.
"""
import math

import numpy as np
import torch

U32 = 2.0 ** -24
BILINEAR_ULPS = 16
LABEL_MARGIN = 1e-5
LABEL_UNDER_MARGIN_SHARE = 1e-3
SSE_RTOL = 1e-12

MAPS = [(1, 1), (3, 5), (25, 33), (24, 40)]
CHANNELS = [8, 64, 264]
# (in map, out map): the tower's upsampling to the stage-0 map, the identity, a downsampling, one row / column
RESIZES = [((1, 1), (3, 5)), ((4, 5), (25, 33)), ((3, 5), (24, 40)), ((24, 40), (24, 40)), ((25, 33), (7, 9)), ((1, 7), (5, 1))]
LABEL_COUNTS = [2, 6, 19, 150, 256]


def rng(*key):
    return np.random.default_rng([20240917] + [int(k) for k in key])


def bf16_round(x):
    """float32 values rounded to bfloat16 (nearest even), as float32."""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).float().numpy()


# ------------------------------------------------------------------------------------------------ bilinear, labels
def source_taps(n_in, n_out):
    """(i0, i1, l) of every output index, align_corners=False: the source coordinate (d + 1/2) n_in / n_out - 1/2 clamped at 0,
    its floor, the next index clamped at the edge, and its fractional part -- in exact rational arithmetic."""
    d = np.arange(n_out, dtype=np.int64)
    num = np.maximum((2 * d + 1) * n_in - n_out, 0)
    i0 = num // (2 * n_out)
    lam = (num - i0 * 2 * n_out) / float(2 * n_out)
    return i0, np.minimum(i0 + 1, n_in - 1), lam


def bilinear_f64(x, Ho, Wo):
    """x [B, h, w, C] -> float64 [B, Ho, Wo, C]."""
    x = np.asarray(x, dtype=np.float64)
    y0, y1, ly = source_taps(x.shape[1], Ho)
    x0, x1, lx = source_taps(x.shape[2], Wo)
    lx, ly = lx[None, None, :, None], ly[None, :, None, None]
    top = (1 - lx) * x[:, y0][:, :, x0] + lx * x[:, y0][:, :, x1]
    bot = (1 - lx) * x[:, y1][:, :, x0] + lx * x[:, y1][:, :, x1]
    return (1 - ly) * top + ly * bot


def bilinear_bound(x, Ho, Wo):
    """BILINEAR_ULPS u max |neighbour|, per output element."""
    a = np.abs(np.asarray(x, dtype=np.float64))
    y0, y1, _ = source_taps(x.shape[1], Ho)
    x0, x1, _ = source_taps(x.shape[2], Wo)
    m = np.maximum(np.maximum(a[:, y0][:, :, x0], a[:, y0][:, :, x1]), np.maximum(a[:, y1][:, :, x0], a[:, y1][:, :, x1]))
    return BILINEAR_ULPS * U32 * m


def labels_f64(logits, H, W, without=None):
    """(labels uint8 [B, H, W], margin float64 [B, H, W]) of logits [B, h, w, L]: argmax of the float64 interpolation, lowest
    index on ties, and the distance between its two largest values.  ``without``: channels left out of both."""
    z = bilinear_f64(logits, H, W)
    if without is not None:
        z[..., list(without)] = -np.inf
    lab = np.argmax(z, axis=-1)                      # numpy: the first occurrence
    if z.shape[-1] == 1:
        return lab.astype(np.uint8), np.full(lab.shape, np.inf)
    top2 = np.partition(z, -2, axis=-1)[..., -2:]
    return lab.astype(np.uint8), top2[..., 1] - top2[..., 0]


def logits_map(B, h, w, L, *key):
    """Smooth-plus-noise logits fp32 [B, h, w, L]: neighbouring pixels share their leader often, as a network's do."""
    g = rng(h, w, L, *key)
    yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    f = g.uniform(0.5, 3.0, (B, 1, 1, L, 2))
    ph = g.uniform(0, 2 * np.pi, (B, 1, 1, L))
    z = 3.0 * np.sin(2 * np.pi * (f[..., 0] * yy[None, :, :, None] + f[..., 1] * xx[None, :, :, None]) + ph)
    return (z + g.normal(0, 0.7, (B, h, w, L))).astype(np.float32)


# ------------------------------------------------------------------------------------------------ depthwise convolution + GELU
def dwconv_inputs(B, H, W, C, *key):
    """(x bf16-representable fp32 [B, H, W, C], w fp32 [9, C], bias fp32 [C])."""
    g = rng(H, W, C, *key)
    x = bf16_round(g.normal(0, 1.5, (B, H, W, C)))
    w = (g.normal(0, 1, (9, C)) / 3).astype(np.float32)
    return x, w, g.normal(0, 0.5, C).astype(np.float32)


def dwconv_preact_f64(x, w, bias):
    """(v, S): the float64 convolution + bias [B, H, W, C] and |bias| + sum |w x| over the taps inside the map."""
    x, w, bias = (np.asarray(t, dtype=np.float64) for t in (x, w, bias))
    B, H, W, C = x.shape
    xp = np.zeros((B, H + 2, W + 2, C))
    xp[:, 1:-1, 1:-1] = x
    v = np.broadcast_to(bias, x.shape).copy()
    s = np.broadcast_to(np.abs(bias), x.shape).copy()
    for ty in range(3):
        for tx in range(3):
            t = xp[:, ty:ty + H, tx:tx + W] * w[ty * 3 + tx]
            v += t
            s += np.abs(t)
    return v, s


def gelu_f64(v):
    return 0.5 * v * (1.0 + np.vectorize(math.erf)(v / math.sqrt(2.0)))


def dwconv_bound(v, s, ref):
    e = 1.13 * 10 * U32 * s + 4.1e-7 + 1e-6 * np.abs(v)
    return 2.0 ** -8 * (1 + 2.0 ** -8) * np.abs(ref) + e * (1 + 2.0 ** -8)


# ------------------------------------------------------------------------------------------------ the metric
def label_pair(B, H, W, L, *key):
    """Two batches of label maps uint8 [B, H, W]: blocky regions, the second a partly changed copy; pair 0 is unchanged."""
    g = rng(H, W, L, *key)
    bh, bw = max(1, H // 7), max(1, W // 9)
    coarse = g.integers(0, L, (B, -(-H // bh), -(-W // bw)))
    la = np.repeat(np.repeat(coarse, bh, axis=1), bw, axis=2)[:, :H, :W]
    flip = g.random((B, H, W)) < 0.2
    lb = np.where(flip, g.integers(0, L, (B, H, W)), la)
    lb[0] = la[0]
    return la.astype(np.uint8), lb.astype(np.uint8)


def pair_counts_np(la, lb, L):
    """int64 [B, 3, L]."""
    out = np.zeros((la.shape[0], 3, L), dtype=np.int64)
    for b in range(la.shape[0]):
        for l in range(L):
            ia, ib = la[b] == l, lb[b] == l
            out[b, :, l] = ia.sum(), ib.sum(), (ia & ib).sum()
    return out


def overlap_np(la, lb, L):
    """dict(agreement, miou, iou) straight from the definitions, pair by pair and label by label."""
    B = la.shape[0]
    iou = np.full((B, L), np.nan)
    agreement, miou = np.zeros(B), np.zeros(B)
    for b in range(B):
        agreement[b] = np.mean(la[b] == lb[b])
        vals = []
        for l in range(L):
            inter, union = np.sum((la[b] == l) & (lb[b] == l)), np.sum((la[b] == l) | (lb[b] == l))
            if union:
                iou[b, l] = inter / union
                vals.append(iou[b, l])
        miou[b] = sum(vals) / len(vals) if vals else np.nan
    return {"agreement": agreement, "miou": miou, "iou": iou}


def miou_atol(L):
    """The reference adds the L ratios (each at most 1) one after the other in float64: L roundings of at most 2^-53 L each before
    the division by their number; the product's sum is correctly rounded."""
    return L * 2.0 ** -53


def region_sums_np(a, b, la, lb, region):
    """float64 [B, 2]: (sum of squared differences, pixel count) outside the region in both maps; images [B, 3, H, W]."""
    keep = ~(np.isin(la, list(region)) | np.isin(lb, list(region)))
    d2 = ((np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) ** 2).sum(axis=1)
    return np.stack([(d2 * keep).sum(axis=(1, 2)), keep.sum(axis=(1, 2)).astype(np.float64)], 1)


def images(B, H, W, *key):
    """Smooth fp32 images [B, 3, H, W] in [0, 1]."""
    g = rng(H, W, 3, *key)
    yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    f = g.uniform(0.5, 4.0, (B, 3, 1, 1, 2))
    ph = g.uniform(0, 2 * np.pi, (B, 3, 1, 1))
    img = 0.5 + 0.4 * np.sin(2 * np.pi * (f[..., 0] * yy + f[..., 1] * xx) + ph) + g.normal(0, 0.03, (B, 3, H, W))
    return torch.from_numpy(np.clip(img, 0, 1).astype(np.float32))


def edit_pairs(B, H, W, *key):
    """(a, b): b is a with a smooth local change in pairs 1 .., pair 0 unmoved."""
    a = images(B, H, W, *key)
    yy, xx = np.meshgrid(np.linspace(-1, 1, H), np.linspace(-1, 1, W), indexing="ij")
    bump = torch.from_numpy(np.exp(-((yy - 0.2) ** 2 + (xx + 0.1) ** 2) / 0.15).astype(np.float32))
    b = a.clone()
    for i in range(1, B):
        b[i] = (a[i] + 0.35 * i / B * bump * torch.tensor([1.0, -0.6, 0.4]).view(3, 1, 1)).clamp(0, 1)
    return a, b


class StubParser:
    """A parser for the metric tests: a fixed, seeded mixing of nine colour features (the 4 x 4 mean-pooled colours, sin 7 c and
    cos 5 c of them) into L logits (torch on the device; test plumbing, not product code), made a tower by
    ``seg_metrics.LogitsParser``."""

    def __init__(self, L, seed=5):
        g = rng(L, seed)
        self.w = torch.from_numpy(g.normal(0, 2, (L, 9)).astype(np.float32))
        self.num_labels = L

    def logits(self, x):
        p = torch.nn.functional.avg_pool2d(x.float(), 4)
        f = torch.cat([p, torch.sin(7 * p), torch.cos(5 * p)], 1)
        return torch.einsum("lc,bchw->blhw", self.w.to(x.device), f)
