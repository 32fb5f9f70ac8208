"""Whether an edited face is still the same person: the ID similarity of pSp, e4e, StyleCLIP and HyperStyle on the gfx950 tower of
csrc/idnet.hip -- the cosine between the ArcFace IR-SE50 embeddings (``libs.arcface.Backbone``) of the two images, one fp64 value
per pair.  With ``crop`` (default) an image in [-1, 1] is brought to 256 x 256 by adaptive average pooling unless it has that
size, cropped to [35:223, 32:220] and pooled to the tower's input size, as the ``IDLoss`` of those projects does; ``crop=False``
pools the whole image, for inputs that are aligned face crops already.

``IDSimilarity(tower)(a, b)`` and ``id_similarity`` take image batches in [0, 1]; ``calculate_id_similarity_given_paths`` pairs two
folders by file name; ``PairMetrics(identity=tower)`` (``tools/pair_metrics.py``) adds the number as an ``identity`` column.  The
tower's weights are never downloaded: build a ``Backbone`` with ``weights=`` or ``seed=`` and pass it in."""
import numpy as np
import torch

from uspace_amd import _hip
from uspace_amd.libs.arcface import similarity
from uspace_amd.tools import _inputs


class IDSimilarity:
    """``features(images)``: images [B, 3, H, W] in [0, 1] -> unit embeddings fp32 [B, 512]; ``__call__(a, b)``: fp64 [B], the dot
    product of every pair's embeddings.  ``chunk`` images per launch sequence (an image's embedding does not depend on it)."""

    def __init__(self, tower, crop=True, chunk=32):
        self.tower = tower
        self.crop = bool(crop)
        self.chunk = max(1, int(chunk))

    @torch.no_grad()
    def features(self, images, quantize=True):
        """``quantize`` as in ``PairMetrics.update``: save_image's x * 255 + 0.5 -> clamp -> uint8, then / 255 -- the numbers of
        the written PNG."""
        _hip.require_device(images, "images")
        if images.dim() != 4 or images.shape[1] != 3 or images.shape[0] < 1:
            raise ValueError(f"expected images [B, 3, H, W], got {tuple(images.shape)}")
        x = images.detach().to(torch.float32)
        if quantize:
            x = _inputs.quantize(x)
        return self.tower.embed_nhwc(self.tower.preprocess(x, normalize=True, crop=self.crop), self.chunk)

    @torch.no_grad()
    def __call__(self, a, b, quantize=True):
        for t, name in ((a, "a"), (b, "b")):
            _hip.require_device(t, name)
        if a.dim() != 4 or a.shape != b.shape:
            raise ValueError(f"expected two image batches [B, 3, H, W] of one shape, got {tuple(a.shape)} and {tuple(b.shape)}")
        n = a.shape[0]
        e = self.features(torch.cat([a, b]), quantize)      # one batch of 2B images; an embedding does not depend on its place
        return similarity(e[:n].contiguous(), e[n:].contiguous())


def id_similarity(tower, a, b, quantize=True, crop=True):
    """fp64 [B] on the device: the ID similarity of every pair of images a, b [B, 3, H, W] in [0, 1]."""
    return IDSimilarity(tower, crop)(a, b, quantize)


def calculate_id_similarity_given_paths(dir_a, dir_b, tower, device=None, batch_size=50, crop=True):
    """dict(identity, n): the mean ID similarity between the images of two folders paired by file name (a numpy fp64 mean), and
    ``values``, the fp64 array behind it.  A name present in one folder only, or an image whose size differs from its partner's or
    from the first pair's, raises ValueError, as ``calculate_pair_metrics_given_paths`` does."""
    device = _inputs.rocm_device(device, "the ID similarity")
    _names, files_a, files_b = _inputs.paired_image_files(dir_a, dir_b)
    metric = IDSimilarity(tower, crop, chunk=2 * batch_size)
    parts = []
    for xa, xb in zip(_inputs.uint8_batches(files_a, batch_size), _inputs.uint8_batches(files_b, batch_size)):
        parts.append(metric(xa.to(device).float() / 255, xb.to(device).float() / 255, quantize=False))
    values = torch.cat(parts).cpu().numpy()
    return {"identity": float(np.mean(values)), "n": len(values), "values": values}


__all__ = ["IDSimilarity", "id_similarity", "calculate_id_similarity_given_paths"]
