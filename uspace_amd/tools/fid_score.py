"""Frechet Inception Distance on the MI355X (reference tools/fid_score.py, pytorch-fid): the same six functions with the
same signatures and defaults, with the features from the HIP Inception-v3 of uspace_amd/tools/inception.py and the
statistics accumulated in fp64 on the device.  No torchvision: files are read with PIL as uint8 and scaled by 1/255 on
the device (what ``transforms.ToTensor`` does).

``FIDStatistics`` is the in-memory path: images straight out of the sampler and the VAE decoder, quantised as
``save_image`` does, give the statistics the PNG round trip would give."""
import numpy as np
import torch
from scipy import linalg

from uspace_amd import _hip
from uspace_amd.tools import _inputs
from uspace_amd.tools._inputs import IMAGE_EXTENSIONS, MAX_WORKERS, ImagePathDataset, _batches  # noqa: F401  (the reference's names)
from uspace_amd.tools._inputs import image_files, require_paths, rocm_device, unit_batches
from uspace_amd.tools.inception import BLOCK_DIMS, InceptionV3

def _block_of(model, dims):
    block = InceptionV3.BLOCK_INDEX_BY_DIM[dims]
    if block > model.last_needed_block:
        raise ValueError(f"dims={dims} needs output block {block}; the model stops at block {model.last_needed_block}")
    return block


def get_activations(files, model, batch_size=50, dims=2048, device="cpu", num_workers=8):
    """Pool features [len(files), dims] (float64 array of fp32 values) of the images in ``files``, in order."""
    model.eval()
    block = _block_of(model, dims)
    pred_arr = np.empty((len(files), dims))
    start = 0
    for x in unit_batches(files, batch_size, num_workers, device):
        pred = model.features(x, block).cpu().numpy()
        pred_arr[start:start + pred.shape[0]] = pred
        start += pred.shape[0]
    return pred_arr


def calculate_frechet_distance(mu1, sigma1, mu2, sigma2, eps=1e-6):
    """d^2 = |mu1 - mu2|^2 + Tr(sigma1 + sigma2 - 2 sqrt(sigma1 sigma2)), the matrix square root by scipy in fp64.  A
    singular product is retried with eps added to both diagonals; an imaginary part above 1e-3 on the diagonal of the
    square root raises ValueError."""
    mu1, mu2 = np.atleast_1d(mu1), np.atleast_1d(mu2)
    sigma1, sigma2 = np.atleast_2d(sigma1), np.atleast_2d(sigma2)
    assert mu1.shape == mu2.shape, "Training and test mean vectors have different lengths"
    assert sigma1.shape == sigma2.shape, "Training and test covariances have different dimensions"
    diff = mu1 - mu2
    covmean, _ = linalg.sqrtm(sigma1.dot(sigma2), disp=False)
    if not np.isfinite(covmean).all():
        print(f"fid calculation produces singular product; adding {eps} to diagonal of cov estimates")
        offset = np.eye(sigma1.shape[0]) * eps
        covmean = linalg.sqrtm((sigma1 + offset).dot(sigma2 + offset))
    if np.iscomplexobj(covmean):
        if not np.allclose(np.diagonal(covmean).imag, 0, atol=1e-3):
            raise ValueError(f"Imaginary component {np.max(np.abs(covmean.imag))}")
        covmean = covmean.real
    return diff.dot(diff) + np.trace(sigma1) + np.trace(sigma2) - 2 * np.trace(covmean)


def calculate_activation_statistics(files, model, batch_size=50, dims=2048, device="cpu", num_workers=8):
    """(mu, sigma) of the features of ``files``: fp64 sums on the device, accumulated batch by batch as the features
    were computed (FIDStatistics), finalised as np.mean / np.cov(rowvar=False)."""
    act = get_activations(files, model, batch_size, dims, device, num_workers)
    bs = max(1, min(batch_size, len(files)))
    st = FIDStatistics(dims, device=device, model=model)
    for lo in range(0, len(act), bs):
        st.update_features(torch.from_numpy(act[lo:lo + bs].astype(np.float32)).to(device))
    return st.mu, st.sigma


def compute_statistics_of_path(path, model, batch_size, dims, device, num_workers=8):
    if path.endswith(".npz"):
        with np.load(path) as f:
            m, s = f["mu"][:], f["sigma"][:]
    else:
        m, s = calculate_activation_statistics(image_files(path), model, batch_size, dims, device, num_workers)
    return m, s


def save_statistics_of_path(path, out_path, device=None, batch_size=50, dims=2048, num_workers=8):
    device = rocm_device(device, "FID")
    model = InceptionV3([InceptionV3.BLOCK_INDEX_BY_DIM[dims]]).to(device)
    m1, s1 = compute_statistics_of_path(path, model, batch_size, dims, device, num_workers)
    np.savez(out_path, mu=m1, sigma=s1)


def calculate_fid_given_paths(paths, device=None, batch_size=50, dims=2048, num_workers=8, model=None):
    """FID between two folders of images or .npz statistics files.  ``model`` (an InceptionV3) overrides the pretrained
    network, e.g. with seeded weights."""
    device = rocm_device(device, "FID")
    require_paths(paths)
    if model is None:
        model = InceptionV3([InceptionV3.BLOCK_INDEX_BY_DIM[dims]]).to(device)
    m1, s1 = compute_statistics_of_path(paths[0], model, batch_size, dims, device, num_workers)
    m2, s2 = compute_statistics_of_path(paths[1], model, batch_size, dims, device, num_workers)
    return calculate_frechet_distance(m1, s1, m2, s2)


def finalize_statistics(n, shift, s1, s2):
    """mu, sigma (float64 numpy) from n samples' shifted sums: mu = c + S1 / n, sigma = (S2 - S1 S1^T / n) / (n - 1)."""
    shift, s1, s2 = (np.asarray(a, np.float64) for a in (shift, s1, s2))
    mu = shift + s1 / n
    sigma = (s2 - np.outer(s1, s1) / n) / (n - 1)
    return mu, sigma


_NO_MODEL = object()      # ``model`` of an accumulator over arbitrary features (``of_width``)


class FeatureAccumulator:
    """What ``FIDStatistics`` and ``FeatureBank`` share: the width check of the Inception pool blocks, the lazily built network
    and ``update`` on images.  ``of_width`` builds one over arbitrary features [n, dims], with no model behind it."""

    def __init__(self, dims=2048, device=None, model=None):
        if model is _NO_MODEL:
            self._setup(dims, device, None, None)
        elif dims not in InceptionV3.BLOCK_INDEX_BY_DIM:
            raise ValueError(f"dims must be one of {sorted(InceptionV3.BLOCK_INDEX_BY_DIM)}")
        else:
            self._setup(dims, device, model, InceptionV3.BLOCK_INDEX_BY_DIM[dims])

    @classmethod
    def of_width(cls, dims, device=None):
        """An accumulator of features of any width ``dims`` >= 1, fed by ``update_features`` only."""
        return cls(dims, device, _NO_MODEL)

    def _setup(self, dims, device, model, block):
        self.dims = int(dims)
        self.device = rocm_device(device, type(self).__name__)
        self.block = block
        self._model = model
        self.reset()

    @property
    def model(self):
        if self._model is None:
            if self.block is None:
                raise ValueError(f"a {type(self).__name__} made for features has no model: use update_features")
            self._model = InceptionV3([self.block]).to(self.device)
        return self._model

    @torch.no_grad()
    def update(self, images, quantize=True):
        """Add images [B, 3, H, W] in [0, 1].  quantize=True applies save_image's x * 255 + 0.5 -> clamp -> uint8, then
        / 255 (``_inputs.quantize``), so the result equals that of the written PNGs read back."""
        x = images.detach().to(self.device, torch.float32)
        self.update_features(self.model.features(_inputs.quantize(x) if quantize else x, self.block))


class FIDStatistics(FeatureAccumulator):
    """Running mean and covariance of FID features on the device.  S1 = sum(x - c) and S2 = sum((x - c)(x - c)^T) are
    accumulated in fp64 by uspace_fid_stats_accumulate, with c the first batch's mean (fp64), so a large common offset
    of the features costs no precision; ``mu`` / ``sigma`` equal np.mean / np.cov(rowvar=False) of all features seen."""

    def reset(self):
        self.n = 0
        self.shift = self.s1 = self.s2 = None

    @torch.no_grad()
    def update_features(self, feat):
        """Add features [B, dims] (fp32 on the device)."""
        _hip.require_device(feat, "features")
        feat = feat.detach().to(torch.float32).contiguous()
        if feat.dim() != 2 or feat.shape[1] != self.dims:
            raise ValueError(f"expected features [B, {self.dims}], got {tuple(feat.shape)}")
        B = feat.shape[0]
        if B == 0:
            return
        if self.n == 0:
            self.shift = feat.double().mean(0)
            self.s1 = torch.zeros(self.dims, dtype=torch.float64, device=feat.device)
            self.s2 = torch.zeros(self.dims, self.dims, dtype=torch.float64, device=feat.device)
        _hip.check(_hip.lib().uspace_fid_stats_accumulate(_hip.ptr(feat), B, self.dims, _hip.ptr(self.shift),
                                                          _hip.ptr(self.s1), _hip.ptr(self.s2), _hip.stream_ptr()),
                   "uspace_fid_stats_accumulate")
        self.n += B

    def _final(self):
        if self.n < 2:
            raise ValueError("FID statistics need at least two samples")
        return finalize_statistics(self.n, self.shift.cpu().numpy(), self.s1.cpu().numpy(), self.s2.cpu().numpy())

    @property
    def mu(self):
        return self._final()[0]

    @property
    def sigma(self):
        return self._final()[1]

    def save(self, path):
        """The reference's statistics file: np.savez(path, mu=..., sigma=...)."""
        mu, sigma = self._final()
        np.savez(path, mu=mu, sigma=sigma)


__all__ = ["IMAGE_EXTENSIONS", "ImagePathDataset", "get_activations", "calculate_frechet_distance",
           "calculate_activation_statistics", "compute_statistics_of_path", "save_statistics_of_path",
           "calculate_fid_given_paths", "FIDStatistics", "finalize_statistics", "BLOCK_DIMS"]
