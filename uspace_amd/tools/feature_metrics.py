"""Kernel Inception Distance and precision / recall / density / coverage on the MI355X, from the Inception pool features the
FID path computes (uspace_amd/tools/fid_score.py) or from any other fp32 features, e.g. the CLIP embeddings of
uspace_amd/tools/clip_score.py.

All five numbers are reductions over pairwise quantities of two feature sets [N, F] and [M, F].  The N x M matrix is never
stored: the fp64 Gram kernels of uspace_amd/csrc/metrics.hip fuse the reductions into the tiles, and the host only adds
integers, compares and divides.  With D2(i, j) = max(0, |x_i|^2 + |y_j|^2 - 2 x_i . y_j) in fp64 from the fp32 values:

  KID (Binkowski et al. 2018): the mean and standard deviation over random subsets of the unbiased MMD^2 estimate with the
  polynomial kernel K(a, b) = (gamma a . b + coef0)^degree.
  Improved precision / recall (Kynkaanniemi et al. 2019) and density / coverage (Naeem et al. 2020): with rR, rG the squared
  distances to the k-th nearest neighbour within the real and the generated set (self excluded by index),
    precision = mean_j [ #{i : D2(fake_j, real_i) <= rR_i} > 0 ]      density  = sum_j #{...} / (k n_fake)
    recall    = mean_i [ #{j : D2(real_i, fake_j) <= rG_j} > 0 ]      coverage = mean_i [ min_j D2(real_i, fake_j) <= rR_i ]

There is no CPU path: a CPU tensor or a missing library raises ``UspaceHipError``."""
import numpy as np
import torch

from uspace_amd import _hip
from uspace_amd.tools import fid_score
from uspace_amd.tools._inputs import image_files, require_paths, rocm_device
from uspace_amd.tools.inception import InceptionV3

MAX_NEAREST_K = 16
_CHUNK = 1024


class FeatureBank(fid_score.FeatureAccumulator):
    """The feature-keeping sibling of ``FIDStatistics`` (same constructor, ``of_width``, ``model`` and ``update``): fp32 features
    [n, dims] on the device, grown by chunks."""

    @classmethod
    def from_features(cls, feat, device=None):
        """A bank of arbitrary features [n, F] (any F >= 1: no dims check, no model), kept on ``device`` (default: where
        ``feat`` lives)."""
        feat = torch.as_tensor(feat)
        if feat.dim() != 2 or feat.shape[1] < 1:
            raise ValueError(f"expected features [n, F], got {tuple(feat.shape)}")
        bank = cls.of_width(feat.shape[1], device if device is not None else feat.device)
        bank.update_features(feat)
        return bank

    def reset(self):
        self.n = 0
        self._buf = None

    def __len__(self):
        return self.n

    @property
    def features(self):
        """fp32 [n, dims] on the device (a view of the bank's storage)."""
        if self._buf is None:
            return torch.empty(0, self.dims, dtype=torch.float32, device=self.device)
        return self._buf[:self.n]

    @torch.no_grad()
    def update_features(self, feat):
        """Append features [B, dims]; other dtypes are converted to fp32."""
        feat = torch.as_tensor(feat).detach().to(self.device, torch.float32)
        if feat.dim() != 2 or feat.shape[1] != self.dims:
            raise ValueError(f"expected features [B, {self.dims}], got {tuple(feat.shape)}")
        B = feat.shape[0]
        if B == 0:
            return
        need = self.n + B
        if self._buf is None or need > self._buf.shape[0]:
            cap = max(need, 2 * (0 if self._buf is None else self._buf.shape[0]))
            cap = (cap + _CHUNK - 1) // _CHUNK * _CHUNK
            buf = torch.empty(cap, self.dims, dtype=torch.float32, device=self.device)
            if self.n:
                buf[:self.n] = self._buf[:self.n]
            self._buf = buf
        self._buf[self.n:need] = feat
        self.n = need

    def save(self, path):
        """np.savez(path, features=...): fp32 [n, dims]."""
        np.savez(path, features=self.features.cpu().numpy())

    @classmethod
    def load(cls, path, device=None):
        """The bank ``save`` wrote, on ``device`` (default: the ROCm device)."""
        with np.load(path) as f:
            feat = np.asarray(f["features"], dtype=np.float32)
        return cls.from_features(torch.from_numpy(feat), device=rocm_device(device, "FeatureBank.load"))


def _features(a, name):
    t = a.features if isinstance(a, FeatureBank) else a
    if not torch.is_tensor(t) or t.dim() != 2 or t.shape[1] < 1:
        raise ValueError(f"{name} must be a FeatureBank or a tensor [n, F]")
    return t


def _device_features(t, name):
    _hip.require_device(t, name)
    return t.detach().to(torch.float32).contiguous()


def draw_subsets(n_fake, n_real, subsets, subset_size, seed):
    """(idx_fake, idx_real), int32 [subsets, subset_size]: per subset ``rng.choice(n_fake, subset_size, replace=False)`` first, then
    the same for n_real, from ``np.random.RandomState(seed)``."""
    rng = np.random.RandomState(seed)
    idx_f = np.empty((subsets, subset_size), np.int32)
    idx_r = np.empty((subsets, subset_size), np.int32)
    for s in range(subsets):
        idx_f[s] = rng.choice(n_fake, subset_size, replace=False)
        idx_r[s] = rng.choice(n_real, subset_size, replace=False)
    return idx_f, idx_r


def mmd2_unbiased(sums, m):
    """Per-subset unbiased MMD^2 (float64 [subsets]) from the kernel sums [subsets, 3] = (Sxx, Syy, Sxy) of subsets of size m."""
    sums = np.asarray(sums, np.float64)
    return sums[:, 0] / (m * (m - 1)) + sums[:, 1] / (m * (m - 1)) - 2 * sums[:, 2] / (m * m)


@torch.no_grad()
def kid_score(fake, real, subsets=100, subset_size=1000, degree=3, gamma=None, coef0=1.0, seed=2020):
    """(mean, std) of the unbiased polynomial-kernel MMD^2 over ``subsets`` random subsets of ``subset_size`` features of each
    set.  ``gamma=None`` means 1 / F.  Arguments: ``FeatureBank``s or device tensors [n, F]."""
    xf, xr = _features(fake, "fake"), _features(real, "real")
    if xf.shape[1] != xr.shape[1]:
        raise ValueError(f"feature widths differ: {xf.shape[1]} and {xr.shape[1]}")
    m = int(subset_size)
    if m < 2 or m > xf.shape[0] or m > xr.shape[0]:
        raise ValueError(f"subset_size must be in 2 .. min(n_fake, n_real) = {min(xf.shape[0], xr.shape[0])}, got {subset_size}")
    if int(subsets) < 1:
        raise ValueError("subsets must be at least 1")
    if int(degree) != degree or not 1 <= int(degree) <= 8:
        raise ValueError("degree must be an integer in 1 .. 8")
    xf, xr = _device_features(xf, "fake"), _device_features(xr, "real")
    g = 1.0 / xf.shape[1] if gamma is None else float(gamma)
    idx_f, idx_r = draw_subsets(xf.shape[0], xr.shape[0], int(subsets), m, seed)
    sums = _hip.metric_poly_sums(xf, xr, torch.from_numpy(idx_f).to(xf.device), torch.from_numpy(idx_r).to(xf.device),
                                 int(degree), g, float(coef0))
    mmd = mmd2_unbiased(sums.cpu().numpy(), m)
    return float(np.mean(mmd)), float(np.std(mmd))


@torch.no_grad()
def prdc(real, fake, nearest_k=5):
    """dict(precision, recall, density, coverage) as Python floats: two radius launches and two manifold launches."""
    xr, xf = _features(real, "real"), _features(fake, "fake")
    if xf.shape[1] != xr.shape[1]:
        raise ValueError(f"feature widths differ: {xr.shape[1]} and {xf.shape[1]}")
    n_real, n_fake = xr.shape[0], xf.shape[0]
    k = int(nearest_k)
    if k != nearest_k or not 1 <= k <= min(MAX_NEAREST_K, n_real - 1, n_fake - 1):
        raise ValueError(f"nearest_k must be in 1 .. min({MAX_NEAREST_K}, n_real - 1, n_fake - 1) = "
                         f"{min(MAX_NEAREST_K, n_real - 1, n_fake - 1)}, got {nearest_k}")
    xr, xf = _device_features(xr, "real"), _device_features(xf, "fake")
    r_real = _hip.metric_knn_radius2(xr, k)
    r_fake = _hip.metric_knn_radius2(xf, k)
    count_f, _ = _hip.metric_manifold(xf, xr, r_real, want_min=False)      # per generated sample: real balls it falls into
    count_r, min_r = _hip.metric_manifold(xr, xf, r_fake)                  # per real sample: generated balls; nearest generated
    count_f = count_f.cpu().numpy().astype(np.int64)
    count_r = count_r.cpu().numpy().astype(np.int64)
    covered = (min_r <= r_real).cpu().numpy()
    return dict(precision=int((count_f > 0).sum()) / n_fake, recall=int((count_r > 0).sum()) / n_real,
                density=int(count_f.sum()) / (k * n_fake), coverage=int(covered.sum()) / n_real)


def bank_of_path(path, model, batch_size, dims, device, num_workers=8):
    """A ``FeatureBank`` of an image folder (the files ``fid_score`` would read, in its order) or of a saved bank (.npz)."""
    if str(path).endswith(".npz"):
        return FeatureBank.load(path, device=device)
    act = fid_score.get_activations(image_files(path), model, batch_size, dims, device, num_workers)
    return FeatureBank.from_features(torch.from_numpy(act.astype(np.float32)), device=device)


def _banks_of_paths(paths, device, batch_size, dims, num_workers, model):
    device = rocm_device(device, "KID / PRDC")
    require_paths(paths)
    if model is None and not all(str(p).endswith(".npz") for p in paths):
        model = InceptionV3([InceptionV3.BLOCK_INDEX_BY_DIM[dims]]).to(device)
    return [bank_of_path(p, model, batch_size, dims, device, num_workers) for p in paths[:2]]


def calculate_kid_given_paths(paths, device=None, batch_size=50, dims=2048, num_workers=8, model=None, **kid_kwargs):
    """KID (mean, std) between two image folders or saved banks: ``paths[0]`` real, ``paths[1]`` generated, as
    ``calculate_fid_given_paths``; ``kid_kwargs`` go to ``kid_score``."""
    real, fake = _banks_of_paths(paths, device, batch_size, dims, num_workers, model)
    return kid_score(fake, real, **kid_kwargs)


def calculate_prdc_given_paths(paths, nearest_k=5, device=None, batch_size=50, dims=2048, num_workers=8, model=None):
    """Precision / recall / density / coverage between two image folders or saved banks: ``paths[0]`` real, ``paths[1]``
    generated."""
    real, fake = _banks_of_paths(paths, device, batch_size, dims, num_workers, model)
    return prdc(real, fake, nearest_k=nearest_k)


__all__ = ["FeatureBank", "kid_score", "prdc", "calculate_kid_given_paths", "calculate_prdc_given_paths", "draw_subsets",
           "mmd2_unbiased", "bank_of_path", "MAX_NEAREST_K"]
