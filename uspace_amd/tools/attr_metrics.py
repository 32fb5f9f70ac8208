"""Whether an attribute edit did what it was asked to: the change of an attribute classifier's logits between the original and
the edit, on the gfx950 tower of csrc/resnet.hip (``libs.resnet.ResNet``, a torchvision-layout ResNet with one output per
attribute).  LPIPS, SSIM, PSNR, the DINO structure distance and the ArcFace identity cosine say what an edit kept; these columns
say what it changed -- the target attribute against the leakage into the others.  With z the original's logits, z' the edit's,
t the target, ``sign`` the intended direction (the sign of ``write_scale``) and sigma the per-attribute logit standard deviation
over a population (ones when not given):

* ``target_shift``  sign (z'_t - z_t)
* ``target_hit``    1 if sign z'_t > 0 else 0
* ``off_target``    the mean over j != t of |z'_j - z_j| / sigma_j
* ``selectivity``   |z'_t - z_t| / sigma_t over (that + the sum over j != t of |z'_j - z_j| / sigma_j); 0 when nothing moved

all fp64, one value per pair, computed on the device by ``uspace_attr_effect_f64``.  These definitions are this project's own
(INTEGRATION.md §A).  Images are taken as given: no face alignment, no crop, no resize.

``AttributeClassifier(tower)`` names the outputs (the 40 CelebA attributes by default); ``attribute_effect`` takes image batches in
[0, 1]; ``AttributeEffect`` is the callable the ``PairMetrics.attributes`` property takes; ``attribute_response`` reads a
``decode_write_scales`` sweep; ``calculate_attribute_effect_given_paths`` pairs two folders by file name.  The tower's weights
are never downloaded: build a ``ResNet`` with ``weights=`` or ``seed=`` and pass it in."""
import numpy as np
import torch

from uspace_amd import _hip
from uspace_amd.tools import _inputs
from uspace_amd.tools.utils_attr import CELEBA_ATTRS, get_attr_name_from_attr_id

COLUMNS = ("target_shift", "target_hit", "off_target", "selectivity")


class AttributeClassifier:
    """``logits(images)``: images [B, 3, H, W] in [0, 1] on the device -> fp32 [B, A].  ``names``: one per output of the tower,
    by default the 40 names ``utils_attr.get_attr_name_from_attr_id`` knows for CelebA; ``chunk`` images per launch sequence (an
    image's logits do not depend on it)."""

    def __init__(self, tower, names=None, chunk=32):
        if names is None:
            names = [get_attr_name_from_attr_id(i, "celeba") for i in range(len(CELEBA_ATTRS))]
        names = [str(n) for n in names]
        if len(names) != tower.num_classes or len(set(names)) != len(names):
            raise ValueError(f"{len(names)} attribute names ({len(set(names))} distinct) for a tower of {tower.num_classes} outputs")
        self.tower, self.names, self.chunk = tower, names, max(1, int(chunk))

    def index(self, target):
        """An attribute's index from its name or index."""
        if isinstance(target, str):
            if target not in self.names:
                raise ValueError(f"unknown attribute {target!r}")
            return self.names.index(target)
        if isinstance(target, (int, np.integer)) and not isinstance(target, bool) and 0 <= int(target) < len(self.names):
            return int(target)
        raise ValueError(f"attribute {target!r} is neither a name nor an index below {len(self.names)}")

    @torch.no_grad()
    def logits(self, images, quantize=True):
        """``quantize`` as in ``PairMetrics.update``: save_image's x * 255 + 0.5 -> clamp -> uint8, then / 255 -- the numbers of
        the written PNG."""
        _hip.require_device(images, "images")
        if images.dim() != 4 or images.shape[1] != 3 or images.shape[0] < 1:
            raise ValueError(f"expected images [B, 3, H, W], got {tuple(images.shape)}")
        x = images.detach().to(torch.float32)
        if quantize:
            x = _inputs.quantize(x)
        return self.tower(x, chunk=self.chunk)

    @torch.no_grad()
    def logit_std(self, images, quantize=True, device=None, batch_size=50):
        """fp64 numpy [A]: the standard deviation (population form, / N) of every logit over ``images`` -- a device batch
        [N, 3, H, W] in [0, 1], or a folder of equally sized image files.  The sigma of ``attribute_effect``."""
        if torch.is_tensor(images):
            z = self.logits(images, quantize).double()
        else:
            device = _inputs.rocm_device(device, "AttributeClassifier.logit_std")
            files = _inputs.image_files(images)
            if not files:
                raise ValueError(f"no images in {images}")
            z = torch.cat([self.logits(x.to(device).float() / 255, quantize=False).double()
                           for x in _inputs.uint8_batches(files, batch_size)])
        if z.shape[0] < 2:
            raise ValueError("a standard deviation needs at least two images")
        return z.cpu().numpy().std(axis=0)


def effect_columns(za, zb, target, sign, sigma=None):
    """fp64 [B, 4] on the device (``COLUMNS``) from logits za, zb fp32 [B, A], target int32 [B], sign fp32 [B] and sigma fp32
    [A] or None, all on the device (``uspace_attr_effect_f64``)."""
    for t, name in ((za, "za"), (zb, "zb"), (target, "target"), (sign, "sign")) + (((sigma, "sigma"),) if sigma is not None else ()):
        _hip.require_device(t, name)
    if za.dim() != 2 or za.shape != zb.shape or za.shape[0] < 1 or za.dtype != torch.float32 or zb.dtype != torch.float32:
        raise _hip.UspaceHipError(f"za and zb must be fp32 [B, A] of one shape, got {za.dtype} {tuple(za.shape)} and {zb.dtype} {tuple(zb.shape)}")
    B, A = za.shape
    if target.dtype != torch.int32 or tuple(target.shape) != (B,) or sign.dtype != torch.float32 or tuple(sign.shape) != (B,):
        raise _hip.UspaceHipError(f"target must be int32 [{B}] and sign fp32 [{B}]")
    if sigma is not None and (sigma.dtype != torch.float32 or tuple(sigma.shape) != (A,)):
        raise _hip.UspaceHipError(f"sigma must be fp32 [{A}], got {sigma.dtype} {tuple(sigma.shape)}")
    za, zb, target, sign = (t.contiguous() for t in (za, zb, target, sign))
    sigma = sigma.contiguous() if sigma is not None else None
    out = torch.empty(B, 4, dtype=torch.float64, device=za.device)
    _hip.check(_hip.lib().uspace_attr_effect_f64(_hip.ptr(za), _hip.ptr(zb), _hip.ptr(target), _hip.ptr(sign), _hip.ptr(sigma), B, A,
                                                 _hip.ptr(out), _hip.stream_ptr()), "uspace_attr_effect_f64")
    return out


def _per_pair(clf, target, sign, sigma, B):
    """(target int32 [B], sign fp32 [B], sigma fp32 [A] or None) as host tensors, checked."""
    if isinstance(target, (str, int, np.integer)):
        target = [target] * B
    target = [clf.index(t) for t in target]
    if len(target) != B:
        raise ValueError(f"{len(target)} targets for {B} pairs")
    sign = np.full(B, sign, dtype=np.float32) if np.ndim(sign) == 0 else np.array(sign, dtype=np.float32)
    if sign.shape != (B,) or not np.all(np.abs(sign) == 1):
        raise ValueError(f"sign must be +1 or -1, one value or one per pair, got {sign!r}")
    if sigma is not None:
        sigma = np.asarray(sigma, dtype=np.float64)
        if sigma.shape != (len(clf.names),) or not np.all(np.isfinite(sigma)) or not np.all(sigma > 0):
            raise ValueError(f"sigma must be {len(clf.names)} positive finite values")
        sigma = torch.from_numpy(sigma.astype(np.float32))
    return torch.tensor(target, dtype=torch.int32), torch.from_numpy(sign), sigma


@torch.no_grad()
def effect_on_device(clf, original, edited, target, sign=+1, sigma=None, quantize=True):
    """fp64 [B, 4] on the device (``COLUMNS``): ``attribute_effect`` before it is split into columns."""
    for t, name in ((original, "original"), (edited, "edited")):
        _hip.require_device(t, name)
    if original.dim() != 4 or original.shape != edited.shape:
        raise ValueError(f"expected two image batches [B, 3, H, W] of one shape, got {tuple(original.shape)} and {tuple(edited.shape)}")
    n = original.shape[0]
    tgt, sg, sig = _per_pair(clf, target, sign, sigma, n)
    z = clf.logits(torch.cat([original, edited]), quantize)       # one batch of 2B images; a row does not depend on its place
    dev = z.device
    return effect_columns(z[:n].contiguous(), z[n:].contiguous(), tgt.to(dev), sg.to(dev), sig.to(dev) if sig is not None else None)


def attribute_effect(clf, original, edited, target, sign=+1, sigma=None, quantize=True):
    """dict(target_shift, target_hit, off_target, selectivity) of fp64 numpy arrays [B]: the effect of the edit
    original -> edited (image batches [B, 3, H, W] in [0, 1] on the device) on attribute ``target`` -- a name, an index, or one of
    either per pair.  ``sign``: the intended direction (+1 or -1, one value or one per pair), the sign of ``write_scale``;
    ``sigma``: the per-attribute logit standard deviation (``AttributeClassifier.logit_std``), None for ones."""
    out = effect_on_device(clf, original, edited, target, sign, sigma, quantize).cpu().numpy()
    return {k: np.ascontiguousarray(out[:, i]) for i, k in enumerate(COLUMNS)}


class AttributeEffect:
    """``AttributeEffect(clf, target, sign, sigma)(original, edited)``: ``attribute_effect`` with the edit's description bound --
    what the ``PairMetrics.attributes`` property takes.  ``columns(original, edited)``: the same as fp64 [B, 4] on the device."""

    def __init__(self, clf, target, sign=+1, sigma=None):
        self.clf, self.target, self.sign, self.sigma = clf, target, sign, sigma
        if isinstance(target, (str, int, np.integer)):
            clf.index(target)

    def columns(self, original, edited, quantize=True):
        return effect_on_device(self.clf, original, edited, self.target, self.sign, self.sigma, quantize)

    def __call__(self, original, edited, quantize=True):
        return attribute_effect(self.clf, original, edited, self.target, self.sign, self.sigma, quantize)


@torch.no_grad()
def attribute_response(clf, sweep, scales, target, quantize=True):
    """How the logits follow the scale of a ``decode_write_scales`` sweep.  sweep: [S, B, 3, H, W] images in [0, 1] on the
    device, already decoded; scales: the S write scales; target: a name or an index.  Returns dict(logits fp64 [S, B, A],
    target_slope fp64 [B], slopes fp64 [B, A]): per sample the least-squares slope of every logit against the scale
    (sum (s - mean s)(z - mean z) / sum (s - mean s)^2, host numpy on the fp64 logits); ``target_slope`` is column ``target``."""
    _hip.require_device(sweep, "sweep")
    scales = np.asarray(scales, dtype=np.float64)
    if sweep.dim() != 5 or sweep.shape[2] != 3 or scales.shape != (sweep.shape[0],) or sweep.shape[0] < 2:
        raise ValueError(f"expected a sweep [S, B, 3, H, W] with S >= 2 and S scales, got {tuple(sweep.shape)} and {scales.shape}")
    ds = scales - scales.mean()
    if not np.any(ds):
        raise ValueError("the scales are all equal: no slope")
    t = clf.index(target)
    S, B = sweep.shape[:2]
    z = clf.logits(sweep.reshape((S * B,) + tuple(sweep.shape[2:])), quantize).double().cpu().numpy().reshape(S, B, -1)
    slopes = np.einsum("s,sba->ba", ds, z - z.mean(axis=0, keepdims=True)) / np.sum(ds * ds)
    return {"logits": z, "target_slope": np.ascontiguousarray(slopes[:, t]), "slopes": slopes}


def calculate_attribute_effect_given_paths(dir_a, dir_b, clf, target, sign=+1, device=None, batch_size=50, sigma=None):
    """dict(target_shift, target_hit, off_target, selectivity, n): the mean effect (numpy fp64 means) of the edits dir_a -> dir_b,
    the images of two folders paired by file name, and ``values``, the dict of fp64 arrays behind the means.  A name present in one
    folder only, or an image whose size differs from its partner's or from the first pair's, raises ValueError, as
    ``calculate_pair_metrics_given_paths`` does.  ``target`` and ``sign``: one for all pairs."""
    device = _inputs.rocm_device(device, "the attribute effect")
    _names, files_a, files_b = _inputs.paired_image_files(dir_a, dir_b)
    parts = []
    for xa, xb in zip(_inputs.uint8_batches(files_a, batch_size), _inputs.uint8_batches(files_b, batch_size)):
        parts.append(effect_on_device(clf, xa.to(device).float() / 255, xb.to(device).float() / 255, target, sign, sigma, quantize=False))
    out = torch.cat(parts).cpu().numpy()
    values = {k: np.ascontiguousarray(out[:, i]) for i, k in enumerate(COLUMNS)}
    res = {k: float(np.mean(v)) for k, v in values.items()}
    res["n"] = len(out)
    res["values"] = values
    return res


__all__ = ["AttributeClassifier", "AttributeEffect", "attribute_effect", "attribute_response", "effect_columns", "effect_on_device",
           "calculate_attribute_effect_given_paths", "COLUMNS"]
