"""The two numbers a DINO backbone gives an editing stack, on the gfx950 tower of csrc/dino.hip:

* **FD-DINOv2** (Stein et al. 2023): the Frechet distance on the class-token features (``pooler_output``) of DINOv2 ViT-L/14 --
  ``FDDino`` accumulates them with ``FIDStatistics.update_features`` and finishes with ``calculate_frechet_distance``.
* **Structure distance** (Tumanyan et al. 2022; the "structure" column of PIE-Bench): the mean squared difference between the
  cosine self-similarity matrices of a ViT's last-layer keys for the original and the edited image, class token included --
  ``structure_distance`` (``uspace_self_similarity_mse_f64``).  The usual backbone is DINO ViT-B/8 (``libs.dino.DINO_B8``).

``FeatureBank.from_features(DinoFeatures(tower).features(images))`` (``tools/feature_metrics.py``) gives KID / PRDC on the same features.
The towers' weights are never downloaded: build a ``DinoVisionTransformer`` with ``weights=`` or ``seed=`` and pass it in."""
import numpy as np
import torch

from uspace_amd import _hip
from uspace_amd.tools._inputs import chunked_features, image_files, require_paths, rocm_device, uint8_batches
from uspace_amd.tools.fid_score import FIDStatistics, calculate_frechet_distance


class DinoFeatures:
    """``features(images)``: images [B, 3, H, H] in [0, 1] -> the tower's ``pooler_output`` fp32 [B, D], ``chunk`` images per
    launch sequence (a row's features do not depend on it)."""

    def __init__(self, tower, chunk=64):
        self.tower = tower
        self.chunk = max(1, int(chunk))
        self.dims = tower.cfg["dim"]

    @torch.no_grad()
    def features(self, images, quantize=True):
        return chunked_features(lambda x: self.tower(self.tower.preprocess(x, quantize=quantize)), images, self.chunk, self.dims)


class FDDino:
    """Frechet distance on DINO class-token features: ``update`` (generated) / ``update_real`` / ``compute``; ``save`` / ``load``
    keep the real set's statistics as ``FIDStatistics.save`` writes them (``mu``, ``sigma``)."""

    def __init__(self, tower, device=None, chunk=64):
        self.device = rocm_device(device, "FD-DINO")
        self.extractor = DinoFeatures(tower, chunk)
        self.dims = self.extractor.dims
        self.reset()

    def reset(self, real=True):
        self.fake = FIDStatistics.of_width(self.dims, self.device)
        if real:
            self.real = FIDStatistics.of_width(self.dims, self.device)
            self._real_loaded = None

    def update(self, images, quantize=True):
        self.fake.update_features(self.extractor.features(images.detach().to(self.device, torch.float32), quantize))

    def update_real(self, images, quantize=True):
        if self._real_loaded is not None:
            raise ValueError("the real set's statistics were loaded from a file: reset() before adding images")
        self.real.update_features(self.extractor.features(images.detach().to(self.device, torch.float32), quantize))

    def _real(self):
        return self._real_loaded if self._real_loaded is not None else (self.real.mu, self.real.sigma)

    def save(self, path):
        mu, sigma = self._real()
        np.savez(path, mu=mu, sigma=sigma)

    def load(self, path):
        with np.load(path) as f:
            mu, sigma = f["mu"][:], f["sigma"][:]
        if mu.shape != (self.dims,) or sigma.shape != (self.dims, self.dims):
            raise ValueError(f"{path}: statistics of width {mu.shape}, the tower's features have {self.dims}")
        self._real_loaded = (mu, sigma)

    def compute(self):
        mu_r, sigma_r = self._real()
        return float(calculate_frechet_distance(self.fake.mu, self.fake.sigma, mu_r, sigma_r))


def fd(features_a, features_b):
    """The Frechet distance of two feature sets [n, D] (numpy / torch, any float type) from their fp64 means and covariances."""
    a, b = (np.asarray(t.detach().cpu() if torch.is_tensor(t) else t, dtype=np.float64) for t in (features_a, features_b))
    return float(calculate_frechet_distance(a.mean(0), np.cov(a, rowvar=False), b.mean(0), np.cov(b, rowvar=False)))


def _folder_statistics(path, extractor, batch_size, device):
    if str(path).endswith(".npz"):
        with np.load(path) as f:
            return f["mu"][:], f["sigma"][:]
    st = FIDStatistics.of_width(extractor.dims, device)
    for batch in uint8_batches(image_files(path), batch_size):
        st.update_features(extractor.features(batch.to(device).float() / 255, quantize=False))
    return st.mu, st.sigma


def calculate_fd_dino_given_paths(paths, tower, device=None, batch_size=50):
    """FD-DINO between two folders of (square, equally sized) images or ``.npz`` statistics files."""
    device = rocm_device(device, "FD-DINO")
    require_paths(paths)
    ex = DinoFeatures(tower, batch_size)
    m1, s1 = _folder_statistics(paths[0], ex, batch_size, device)
    m2, s2 = _folder_statistics(paths[1], ex, batch_size, device)
    return float(calculate_frechet_distance(m1, s1, m2, s2))


@torch.no_grad()
def self_similarity_mse(keys_a, keys_b, ws=None):
    """fp64 [P] on the device: the mean squared difference of the cosine self-similarity matrices of bf16 key sets
    keys_a, keys_b [P, T, D] (views with strides are taken as they are where the library's alignment rules hold)."""
    for t, name in ((keys_a, "keys_a"), (keys_b, "keys_b")):
        _hip.require_device(t, name)
        if t.dtype != torch.bfloat16 or t.dim() != 3:
            raise _hip.UspaceHipError(f"{name} must be a bf16 [P, T, D] tensor, got {t.dtype} {tuple(t.shape)}")
    if keys_a.shape != keys_b.shape or keys_a.shape[0] < 1:
        raise _hip.UspaceHipError(f"key sets of different shapes: {tuple(keys_a.shape)} and {tuple(keys_b.shape)}")
    if keys_a.stride() != keys_b.stride() or keys_a.stride(2) != 1:
        keys_a, keys_b = keys_a.contiguous(), keys_b.contiguous()
    P, T, D = keys_a.shape
    L = _hip.lib()
    nbytes = L.uspace_self_similarity_mse_workspace_bytes(P, T)
    if nbytes == 0:
        raise _hip.UspaceHipError(f"uspace_self_similarity_mse_workspace_bytes({P}, {T}): invalid sizes")
    if ws is None:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=keys_a.device)
    out = torch.empty(P, dtype=torch.float64, device=keys_a.device)
    _hip.check(L.uspace_self_similarity_mse_f64(_hip.ptr(keys_a), _hip.ptr(keys_b), P, T, D, keys_a.stride(1), keys_a.stride(0),
                                                _hip.ptr(ws), ws.numel(), _hip.ptr(out), _hip.stream_ptr()),
               "uspace_self_similarity_mse_f64")
    return out


@torch.no_grad()
def structure_distance(tower, a, b, layer=-1, quantize=True, chunk=32):
    """fp64 [B] on the device: the structure distance of every pair of images a, b [B, 3, H, H] in [0, 1] -- ``tower.keys`` of
    ``layer`` for both members (one batch of 2 x ``chunk`` images per launch sequence), then ``self_similarity_mse``."""
    for t, name in ((a, "a"), (b, "b")):
        _hip.require_device(t, name)
    if a.dim() != 4 or a.shape != b.shape:
        raise ValueError(f"expected two image batches [B, 3, H, H] of one shape, got {tuple(a.shape)} and {tuple(b.shape)}")
    out = torch.empty(a.shape[0], dtype=torch.float64, device=a.device)
    for lo in range(0, a.shape[0], chunk):
        xa, xb = a[lo:lo + chunk], b[lo:lo + chunk]
        n = xa.shape[0]
        keys = tower.keys(tower.preprocess(torch.cat([xa, xb]), quantize=quantize), layer)
        out[lo:lo + n] = self_similarity_mse(keys[:n], keys[n:])
    return out


__all__ = ["DinoFeatures", "FDDino", "fd", "calculate_fd_dino_given_paths", "self_similarity_mse", "structure_distance"]
