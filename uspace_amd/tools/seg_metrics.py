"""Where an edit acted: the overlap between the semantic parsing of the original and the parsing of the edit, and the image
difference outside the part the edit was meant to change -- the "segmentation consistency" the latent-editing papers report.
LPIPS, SSIM, PSNR, the DINO structure distance and the ArcFace cosine say how much an edit kept, ``attr_metrics`` how far the
target attribute moved; these columns say whether *smiling* left hair, background and skin alone.  With A, B the label maps of
the original and the edit (uint8 [H, W], labels 0 .. L - 1), per pair and in fp64:

* ``agreement``      the share of pixels with A == B
* ``iou``            per label l, |A = l and B = l| / |A = l or B = l|; NaN where l is in neither map
* ``miou``           the mean of ``iou`` over the labels present in either map
* ``outside_mse``    with ``region=`` (the label ids of the part the edit is meant to change): the mean over the pixels whose label
                     is in the region in NEITHER map, and over the 3 channels, of (a - b)^2; NaN where no pixel is outside
* ``outside_psnr``   10 log10(1 / outside_mse); +inf where the outside is untouched
* ``outside_share``  the share of pixels that are outside

The counts behind them come from ``uspace_seg_pair_counts`` and ``uspace_seg_region_sse_f64`` (csrc/segformer.hip; integers, and
one fp64 sum in a fixed order), the ratios are formed on the host from those (the mean over labels from the correctly rounded sum), so a pair's
values do not depend on the batch it sits in.  These definitions are this project's own.

The **tower** is whatever parses an image: an object with ``num_labels`` and ``labels(images) -> uint8 [B, H, W]`` for images
[B, 3, H, W] in [0, 1] on the device -- ``libs.segformer.SegFormer`` (built with ``weights=``, ``seed=`` or ``from_hf``; nothing is
ever downloaded), or ``LogitsParser(fn, num_labels)`` around any callable that returns logits [B, L, h, w] (the Hugging Face
layout, usually at H / 4 x W / 4).  Either way the label map is HF's ``post_process_semantic_segmentation`` -- bilinear resize to
the image size, ``align_corners=False``, then argmax with the lowest index on ties -- fused in ``uspace_seg_labels_u8``, which
never stores the full-size logits.  Images are parsed at their own size, without a resize.

``label_overlap`` takes two label maps; ``segmentation_consistency`` two image batches; ``SegmentationConsistency`` accumulates
over batches and is what the ``PairMetrics.parsing`` property takes; ``calculate_segmentation_consistency_given_paths`` pairs two
folders by file name."""
import math

import numpy as np
import torch

from uspace_amd import _hip
from uspace_amd.tools import _inputs

COLUMNS = ("agreement", "miou")
REGION_COLUMNS = ("outside_mse", "outside_psnr", "outside_share")
MAX_LABELS = 256


def _num_labels(num_labels):
    if isinstance(num_labels, bool) or not isinstance(num_labels, (int, np.integer)) or not 1 <= int(num_labels) <= MAX_LABELS:
        raise ValueError(f"num_labels must be an integer from 1 to {MAX_LABELS}, got {num_labels!r}")
    return int(num_labels)


class LogitsParser:
    """``labels(images)`` from a callable ``fn(images) -> logits [B, L, h, w]`` (any float dtype, on the device).  ``chunk``:
    images per call of ``fn`` (an image's labels must not depend on it)."""

    def __init__(self, fn, num_labels, chunk=32):
        self.fn, self.num_labels, self.chunk = fn, _num_labels(num_labels), max(1, int(chunk))

    @torch.no_grad()
    def labels(self, images):
        _hip.require_device(images, "images")
        if images.dim() != 4 or images.shape[0] < 1:
            raise ValueError(f"expected images [B, 3, H, W], got {tuple(images.shape)}")
        out = torch.empty(images.shape[0], images.shape[2], images.shape[3], dtype=torch.uint8, device=images.device)
        for lo in range(0, images.shape[0], self.chunk):
            z = self.fn(images[lo:lo + self.chunk])
            if z.dim() != 4 or z.shape[0] != out[lo:lo + self.chunk].shape[0] or z.shape[1] != self.num_labels:
                raise ValueError(f"the tower returned logits {tuple(z.shape)} for {self.num_labels} labels")
            out[lo:lo + self.chunk] = labels_from_logits(z, images.shape[2:])
        return out


def labels_from_logits(logits, size):
    """uint8 [B, H, W] from logits [B, L, h, w] on the device and ``size`` = (H, W): bilinear resize (``align_corners=False``) and
    argmax, lowest index on ties, in one kernel."""
    _hip.require_device(logits, "logits")
    if logits.dim() != 4:
        raise ValueError(f"expected logits [B, L, h, w], got {tuple(logits.shape)}")
    if logits.shape[1] > MAX_LABELS:
        raise NotImplementedError(f"{logits.shape[1]} labels: a label map is uint8, at most {MAX_LABELS} labels")
    return _hip.seg_labels(logits.detach().to(torch.float32).permute(0, 2, 3, 1).contiguous(), size)


def overlap_from_counts(counts, npx):
    """dict(agreement [B], miou [B], iou [B, L]) of fp64 numpy arrays from counts [B, 3, L] (``uspace_seg_pair_counts``) and the
    number of pixels of a map."""
    c = np.asarray(counts).astype(np.int64)
    in_a, in_b, both = c[:, 0], c[:, 1], c[:, 2]
    union = in_a + in_b - both
    iou = np.full(union.shape, np.nan)
    np.divide(both, union, out=iou, where=union > 0)
    # math.fsum: the correctly rounded sum, whatever the order
    miou = np.array([math.fsum(row[u > 0]) / np.count_nonzero(u > 0) if np.any(u > 0) else np.nan for row, u in zip(iou, union)],
                    dtype=np.float64)
    return {"agreement": both.sum(axis=1) / float(npx), "miou": miou, "iou": iou}


def label_overlap(la, lb, num_labels):
    """dict(agreement, miou, iou, counts) of two batches of label maps uint8 [B, H, W] on the device: fp64 numpy arrays [B], [B],
    [B, L] and the int64 counts [B, 3, L] behind them (pixels of each label in a, in b, in both)."""
    L = _num_labels(num_labels)
    counts = _hip.seg_pair_counts(la, lb, L).cpu().numpy().astype(np.int64)
    out = overlap_from_counts(counts, la[0].numel())
    out["counts"] = counts
    return out


def _member(region, num_labels):
    ids = sorted({int(r) for r in region})
    if not all(0 <= r < num_labels for r in ids):
        raise ValueError(f"region holds label ids outside 0 .. {num_labels - 1}: {ids}")
    m = np.zeros(num_labels, dtype=np.uint8)
    m[ids] = 1
    return torch.from_numpy(m)


def outside_from_sums(sums, npx):
    """dict(outside_mse, outside_psnr, outside_share) of fp64 numpy arrays [B] from ``uspace_seg_region_sse_f64``'s [B, 2]."""
    s = np.asarray(sums, dtype=np.float64)
    sse, n = s[:, 0], s[:, 1]
    mse = np.full(n.shape, np.nan)
    np.divide(sse, 3.0 * n, out=mse, where=n > 0)
    with np.errstate(divide="ignore"):
        psnr = 10.0 * np.log10(1.0 / mse)
    return {"outside_mse": mse, "outside_psnr": psnr, "outside_share": n / float(npx)}


def region_difference(a, b, la, lb, region, num_labels):
    """dict(outside_mse, outside_psnr, outside_share): images a, b fp32 [B, 3, H, W] in [0, 1] and their label maps uint8
    [B, H, W], all on the device; ``region``: the label ids of the part the edit is meant to change (may be empty)."""
    L = _num_labels(num_labels)
    member = _member(region, L).to(a.device)
    sums = _hip.seg_region_sse(a.detach().to(torch.float32).contiguous(), b.detach().to(torch.float32).contiguous(), la, lb, member)
    return outside_from_sums(sums.cpu().numpy(), la[0].numel())


@torch.no_grad()
def segmentation_consistency(tower, a, b, region=None, quantize=True):
    """dict(agreement, miou, iou[, outside_mse, outside_psnr, outside_share]) of fp64 numpy arrays, one row per pair, for the edit
    a -> b: image batches [B, 3, H, W] in [0, 1] on the device, parsed by ``tower`` (both sides in one batch; a label map does not
    depend on its place).  ``quantize`` as in ``PairMetrics.update``: save_image's rounding on both sides, before the tower and
    before the difference."""
    for t, name in ((a, "a"), (b, "b")):
        _hip.require_device(t, name)
    if a.dim() != 4 or a.shape != b.shape or a.shape[0] < 1 or a.shape[1] != 3:
        raise ValueError(f"expected two image batches [B, 3, H, W] of one shape, got {tuple(a.shape)} and {tuple(b.shape)}")
    L = _num_labels(tower.num_labels)
    x, y = (t.detach().to(torch.float32) for t in (a, b))
    if quantize:
        x, y = _inputs.quantize(x), _inputs.quantize(y)
    n = x.shape[0]
    lab = tower.labels(torch.cat([x, y]))
    if lab.dtype != torch.uint8 or tuple(lab.shape) != (2 * n,) + tuple(x.shape[2:]):
        raise ValueError(f"the tower returned labels {lab.dtype} {tuple(lab.shape)} for images {tuple(x.shape)}")
    la, lb = lab[:n].contiguous(), lab[n:].contiguous()
    out = label_overlap(la, lb, L)
    del out["counts"]
    if region is not None:
        out.update(region_difference(x, y, la, lb, region, L))
    return out


class SegmentationConsistency:
    """``segmentation_consistency`` with the tower and the region bound, accumulated over batches: ``update(a, b)``,
    ``values`` (the per-pair arrays seen so far), ``compute()`` (their means; NaN entries -- a label in neither map, a pair with
    no outside -- are left out of a mean, ``iou`` is the per-label mean).  ``columns(a, b)`` gives one batch's scalar columns
    (``column_names``), which is what the ``PairMetrics.parsing`` property reads."""

    def __init__(self, tower, region=None):
        self.tower = tower
        self.num_labels = _num_labels(tower.num_labels)
        self.region = None if region is None else sorted({int(r) for r in region})
        if self.region is not None:
            _member(self.region, self.num_labels)
        self.reset()

    @property
    def column_names(self):
        return COLUMNS + (REGION_COLUMNS if self.region is not None else ())

    def reset(self):
        self._parts = {k: [] for k in self.column_names + ("iou",)}

    def columns(self, original, edited, quantize=True):
        out = segmentation_consistency(self.tower, original, edited, self.region, quantize)
        return {k: out[k] for k in self.column_names}

    def __call__(self, original, edited, quantize=True):
        return segmentation_consistency(self.tower, original, edited, self.region, quantize)

    def update(self, original, edited, quantize=True):
        for k, v in self(original, edited, quantize).items():
            self._parts[k].append(v)

    @property
    def n(self):
        return sum(len(p) for p in self._parts["agreement"])

    @property
    def values(self):
        return {k: (np.concatenate(p) if p else np.empty((0, self.num_labels) if k == "iou" else 0)) for k, p in self._parts.items()}

    def compute(self):
        v = self.values
        if len(v["agreement"]) == 0:
            raise ValueError("SegmentationConsistency has seen no pairs")
        out = {}
        for k, arr in v.items():
            ok = np.isfinite(arr) | np.isposinf(arr)
            if k == "iou":
                cnt = ok.sum(axis=0)
                out[k] = np.where(cnt > 0, np.where(ok, arr, 0.0).sum(axis=0) / np.maximum(cnt, 1), np.nan)
            else:
                out[k] = float(np.mean(arr[ok])) if ok.any() else float("nan")
        out["n"] = len(v["agreement"])
        return out


def calculate_segmentation_consistency_given_paths(dir_a, dir_b, tower, region=None, device=None, batch_size=50):
    """``SegmentationConsistency.compute()``'s dict for the edits dir_a -> dir_b, the images of two folders paired by file name,
    and ``values``, the per-pair arrays behind the means.  A name present in one folder only, or an image whose size differs from
    its partner's or from the first pair's, raises ValueError, as ``calculate_pair_metrics_given_paths`` does."""
    device = _inputs.rocm_device(device, "the segmentation consistency")
    _names, files_a, files_b = _inputs.paired_image_files(dir_a, dir_b)
    acc = SegmentationConsistency(tower, region)
    for xa, xb in zip(_inputs.uint8_batches(files_a, batch_size), _inputs.uint8_batches(files_b, batch_size)):
        acc.update(xa.to(device).float() / 255, xb.to(device).float() / 255, quantize=False)
    res = acc.compute()
    res["values"] = acc.values
    return res


__all__ = ["LogitsParser", "SegmentationConsistency", "label_overlap", "labels_from_logits", "overlap_from_counts",
           "outside_from_sums", "region_difference", "segmentation_consistency", "calculate_segmentation_consistency_given_paths",
           "COLUMNS", "REGION_COLUMNS", "MAX_LABELS"]
