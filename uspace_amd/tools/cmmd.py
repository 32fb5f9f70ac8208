"""CMMD on the MI355X (Jayasumana et al., "Rethinking FID", CVPR 2024): the distribution metric of the text-to-image path that needs
neither Inception features nor a Gaussian fit -- the squared maximum mean discrepancy between the CLIP ViT-L/14-336 image
embeddings of a generated and a real set under a Gaussian RBF kernel.

With feature sets x [nx, F], y [ny, F] (fp32), gamma = 1 / (2 sigma^2) and K(a, b) = exp(-gamma D2(a, b)), D2 the fp64 squared
distance of uspace_amd/csrc/metrics.hip (between the rows scaled to unit length in fp64 when ``normalize``):

  Sxx = sum_{i != j} K(x_i, x_j),  Syy likewise,  Sxy = sum_{i, j} K(x_i, y_j)       (``uspace_metric_rbf_sums``: one launch, fp64,
                                                                                    fixed summation order, no atomics)
  V-statistic   mmd^2 = (Sxx + nx) / nx^2 + (Syy + ny) / ny^2 - 2 Sxy / (nx ny)     (K(a, a) = 1 added here; what CMMD uses)
  U-statistic   mmd^2 = Sxx / (nx (nx - 1)) + Syy / (ny (ny - 1)) - 2 Sxy / (nx ny)  (``unbiased=True``; needs nx, ny >= 2)
  CMMD = 1000 x the V-statistic with sigma = 10 on the L2-normalised ``image_embeds`` of CLIP ViT-L/14-336.

For unit vectors and sigma = 10 every kernel value lies in [0.98, 1] and the score is the difference of three means of them: it
lives in their fourth digit, which is why the sums are fp64 and deterministic.  The constants (sigma, the factor 1000, the
V-statistic with its diagonal, unit-norm embeddings) and the image handling are NOT verified against the published files
(INTEGRATION.md, section A); all of them are arguments.

The tower is ``CLIPVisionTransformer(**CLIP_L_336_VISION)`` (577 tokens: the streaming attention kernel); its unnormalised
``image_embeds`` are banked in a ``FeatureBank`` and normalised inside the kernel.  Where one tower serves this metric and the CLIP
score, ``CLIPScore.image_features(images)`` can be passed to ``CMMD.update_features``.  There is no CPU path."""
import math

import torch

from uspace_amd import _hip
from uspace_amd.tools.feature_metrics import FeatureBank, _device_features, _features
from uspace_amd.tools._inputs import chunked_features, image_files, require_paths, rocm_device, uint8_batches

SIGMA = 10.0
SCALE = 1000.0


def mmd2_from_sums(sums, nx, ny, unbiased=False):
    """MMD^2 (a Python float) from (Sxx, Syy, Sxy), the off-diagonal sums of the two sets and the full cross sum."""
    sxx, syy, sxy = (float(v) for v in sums)
    if unbiased:
        return sxx / (nx * (nx - 1)) + syy / (ny * (ny - 1)) - 2.0 * sxy / (nx * ny)
    return (sxx + nx) / (nx * nx) + (syy + ny) / (ny * ny) - 2.0 * sxy / (nx * ny)


@torch.no_grad()
def rbf_mmd2(x, y, sigma, normalize=True, unbiased=False):
    """MMD^2 of two feature sets (``FeatureBank``s or device tensors [n, F]) under K(a, b) = exp(-D2(a, b) / (2 sigma^2)); the
    V-statistic, or the U-statistic with ``unbiased``.  ``normalize``: D2 between the rows scaled to unit length."""
    tx, ty = _features(x, "x"), _features(y, "y")
    if tx.shape[1] != ty.shape[1]:
        raise ValueError(f"feature widths differ: {tx.shape[1]} and {ty.shape[1]}")
    nx, ny = tx.shape[0], ty.shape[0]
    if nx < 1 or ny < 1:
        raise ValueError(f"both sets need at least one row, got {nx} and {ny}")
    sigma = float(sigma)
    if not (sigma > 0.0 and math.isfinite(sigma)):
        raise ValueError(f"sigma must be positive and finite, got {sigma}")
    if unbiased and (nx < 2 or ny < 2):
        raise ValueError(f"the unbiased estimate needs at least two rows in each set, got {nx} and {ny}")
    tx, ty = _device_features(tx, "x"), _device_features(ty, "y")
    sums = _hip.metric_rbf_sums(tx, ty, 1.0 / (2.0 * sigma * sigma), normalize=bool(normalize))
    return mmd2_from_sums(sums.cpu().tolist(), nx, ny, unbiased)


def cmmd_score(fake, real, sigma=SIGMA, scale=SCALE):
    """``scale`` x the V-statistic MMD^2 of the L2-normalised features of a generated and a real set."""
    return float(scale) * rbf_mmd2(fake, real, sigma, normalize=True, unbiased=False)


class CMMD:
    """Running CMMD: ``update`` (generated images) / ``update_real`` / ``update_features`` / ``compute``; ``save`` / ``load`` keep
    the real set's embeddings as a ``FeatureBank`` .npz.  ``vision``: a ``CLIPVisionTransformer`` (``CLIP_L_336_VISION`` for the
    published metric); images [B, 3, H, H] in [0, 1] on the device go through ``vision.preprocess`` and the tower ``chunk`` at a
    time (a row's embedding does not depend on it), and the unnormalised ``image_embeds`` are kept."""

    def __init__(self, vision, device=None, chunk=64, sigma=SIGMA, scale=SCALE):
        self.device = rocm_device(device, "CMMD")
        self.vision = vision.to(self.device)
        self.chunk = max(1, int(chunk))
        self.dims = vision.cfg["proj_dim"]
        self.sigma, self.scale = float(sigma), float(scale)
        self.reset()

    @classmethod
    def from_pretrained(cls, version="openai/clip-vit-large-patch14-336", device=None):
        """The vision tower and its projection from the HF files of ``version`` on disk (``local_files_only=True``: nothing is
        downloaded; a missing file raises what HF raises)."""
        from transformers import CLIPModel

        from uspace_amd.libs.clip import CLIPVisionTransformer
        return cls(CLIPVisionTransformer.from_hf(CLIPModel.from_pretrained(version, local_files_only=True)), device)

    def reset(self, real=True):
        self.fake = FeatureBank.of_width(self.dims, self.device)
        if real:
            self.real = FeatureBank.of_width(self.dims, self.device)

    @torch.no_grad()
    def image_features(self, images, quantize=True):
        """images [B, 3, H, H] in [0, 1] on the device -> image_embeds fp32 [B, dims] (not normalised)."""
        return chunked_features(lambda x: self.vision(self.vision.preprocess(x, quantize=quantize)), images, self.chunk, self.dims)

    def update(self, images, quantize=True):
        """Add generated images."""
        self.fake.update_features(self.image_features(images.detach().to(self.device, torch.float32), quantize))

    def update_real(self, images, quantize=True):
        """Add real images."""
        self.real.update_features(self.image_features(images.detach().to(self.device, torch.float32), quantize))

    def update_features(self, feat, real=False):
        """Add embeddings [B, dims] computed elsewhere (e.g. ``CLIPScore.image_features`` of the same tower), unnormalised or not."""
        (self.real if real else self.fake).update_features(feat)

    def save(self, path):
        """The real set's embeddings as ``FeatureBank.save`` writes them."""
        self.real.save(path)

    def load(self, path):
        """Replace the real set by a saved bank."""
        bank = FeatureBank.load(path, device=self.device)
        if bank.dims != self.dims:
            raise ValueError(f"{path}: embeddings of width {bank.dims}, the tower's have {self.dims}")
        self.real = bank

    def compute(self):
        if len(self.fake) == 0 or len(self.real) == 0:
            raise ValueError(f"CMMD.compute() needs both sets: {len(self.fake)} generated and {len(self.real)} real embeddings so far")
        return cmmd_score(self.fake, self.real, self.sigma, self.scale)


def _bank_of_path(path, metric, batch_size, device):
    if str(path).endswith(".npz"):
        return FeatureBank.load(path, device=device)
    bank = FeatureBank.of_width(metric.dims, metric.device)
    for batch in uint8_batches(image_files(path), batch_size):
        # quantize=True on decoded bytes is the identity, exactly (see ``_inputs.quantize``): a folder written by save_image gives
        # the bits CMMD.update gives on the samples themselves (without it 255 fl(q / 255) misses q by an ulp)
        bank.update_features(metric.image_features(batch.to(metric.device).float() / 255, quantize=True))
    return bank


def calculate_cmmd_given_paths(paths, vision, device=None, batch_size=50, sigma=SIGMA, scale=SCALE):
    """CMMD between two folders of (square, equally sized) images, read in ``fid_score``'s file order, or saved banks (.npz) in
    either position: ``paths[0]`` real, ``paths[1]`` generated, as ``calculate_fid_given_paths``.  ``vision`` may be None when both
    are banks."""
    require_paths(paths)
    if vision is None and not all(str(p).endswith(".npz") for p in paths[:2]):
        raise ValueError("an image folder needs the vision tower")
    device = rocm_device(device, "CMMD")
    metric = CMMD(vision, device, chunk=batch_size) if vision is not None else None
    real, fake = (_bank_of_path(p, metric, batch_size, device) for p in paths[:2])
    return cmmd_score(fake, real, sigma, scale)


__all__ = ["CMMD", "rbf_mmd2", "cmmd_score", "mmd2_from_sums", "calculate_cmmd_given_paths", "SIGMA", "SCALE"]
