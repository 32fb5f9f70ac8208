"""sFID on the MI355X (Nash et al. 2021, as ADM's evaluator computes it): the Frechet distance of ``fid_score`` on the mean and
covariance of SPATIAL features instead of the pool features.

Spatial features.  For image b: ``tap(stage=14)[b, :, :, :7]`` of uspace_amd/tools/inception.py, flattened in (h, w, c) order to
[2023].  Stage 14 is Mixed_6d; its concatenated output starts with branch1x1, so these are the first 7 channels of
Mixed_6d.branch1x1 after BN and ReLU over the 17 x 17 map.  This is a reading of ADM's ``mixed_6/conv:0[..., :7]`` with TF's
mixed_6 taken to be torchvision's Mixed_6d; it has NOT been checked against the TF graph, so ``spatial_stage`` and
``spatial_channels`` stay parameters with these defaults.  The weights are the pytorch-fid port's: these are that port's numbers.

sFID = ``calculate_frechet_distance`` (unchanged) on mean and covariance of the spatial features, accumulated in fp64 on the
device by uspace_fid_stats_accumulate and finished by ``finalize_statistics``, exactly as FID's.  The features come from
``InceptionV3.suite``: the same walk of the network that yields the pool features.

Statistics files: ``mu_s`` / ``sigma_s`` (the keys of ADM's reference batches) hold the spatial statistics, ``mu`` / ``sigma`` the
pool statistics; a file may hold either pair or both."""
import numpy as np
import torch

from uspace_amd.tools import _inputs
from uspace_amd.tools.fid_score import FIDStatistics, calculate_frechet_distance
from uspace_amd.tools.inception import SPATIAL_CHANNELS, SPATIAL_STAGE, STAGE_SHAPES, InceptionV3

STAT_KEYS = {"fid": ("mu", "sigma"), "sfid": ("mu_s", "sigma_s")}


def spatial_dims(spatial_stage=SPATIAL_STAGE, spatial_channels=SPATIAL_CHANNELS):
    """Length of one image's spatial feature vector: h * w * spatial_channels of the stage (17 * 17 * 7 = 2023)."""
    stage, nch = int(spatial_stage), int(spatial_channels)
    if not 1 <= stage <= 18:
        raise ValueError(f"spatial_stage must be in 1 .. 18, got {spatial_stage}")
    h, w, c = STAGE_SHAPES[stage]
    if not 1 <= nch <= c:
        raise ValueError(f"spatial_channels must be in 1 .. {c} for stage {stage}, got {spatial_channels}")
    return h * w * nch


class SpatialFIDStatistics(FIDStatistics):
    """``FIDStatistics`` over the spatial features: the same fp64 running sums, ``mu`` / ``sigma`` / ``n`` / ``reset`` /
    ``update`` / ``update_features``, with ``dims = 17 * 17 * spatial_channels`` and the features from ``InceptionV3.suite``."""

    def __init__(self, device=None, model=None, spatial_stage=SPATIAL_STAGE, spatial_channels=SPATIAL_CHANNELS):
        # (FIDStatistics.__init__ admits only the four pool widths; everything else is the base's _setup)
        self.spatial_stage = int(spatial_stage)
        self.spatial_channels = int(spatial_channels)
        self._setup(spatial_dims(spatial_stage, spatial_channels), device, model, 3)

    @torch.no_grad()
    def update(self, images, quantize=True):
        """Add images [B, 3, H, W] in [0, 1]; ``quantize`` as in ``FIDStatistics.update``."""
        x = images.detach().to(self.device, torch.float32)
        _pool, spatial = self.model.suite(_inputs.quantize(x) if quantize else x, spatial_stage=self.spatial_stage, spatial_channels=self.spatial_channels)
        self.update_features(spatial)

    def save(self, path):
        """np.savez(path, mu_s=..., sigma_s=...): the keys of ADM's reference batches."""
        mu, sigma = self._final()
        np.savez(path, mu_s=mu, sigma_s=sigma)


def load_statistics(path, kind):
    """(mu, sigma) of ``kind`` ("fid": keys mu / sigma, "sfid": keys mu_s / sigma_s) from an .npz; KeyError names what is missing."""
    k_mu, k_sigma = STAT_KEYS[kind]
    with np.load(path) as f:
        if k_mu not in f or k_sigma not in f:
            raise KeyError(f"{path} holds {sorted(f.keys())}: the {kind} statistics need {k_mu!r} and {k_sigma!r}")
        return f[k_mu][:], f[k_sigma][:]


def suite_statistics_of_folder(path, model, batch_size, device, num_workers=8, spatial_stage=SPATIAL_STAGE,
                               spatial_channels=SPATIAL_CHANNELS):
    """(FIDStatistics, SpatialFIDStatistics) of a folder's images, read as ``fid_score`` reads them: one network pass per batch."""
    pool_st = FIDStatistics(2048, device=device, model=model)
    sp_st = SpatialFIDStatistics(device=device, model=model, spatial_stage=spatial_stage, spatial_channels=spatial_channels)
    for x in _inputs.unit_batches(_inputs.image_files(path), batch_size, num_workers, device):
        pool, spatial = model.suite(x, spatial_stage=spatial_stage, spatial_channels=spatial_channels)
        pool_st.update_features(pool)
        sp_st.update_features(spatial)
    return pool_st, sp_st


def compute_spatial_statistics_of_path(path, model, batch_size, device, num_workers=8, spatial_stage=SPATIAL_STAGE,
                                       spatial_channels=SPATIAL_CHANNELS):
    """(mu_s, sigma_s) of an image folder, or of an .npz holding ``mu_s`` / ``sigma_s``."""
    if str(path).endswith(".npz"):
        return load_statistics(path, "sfid")
    _pool_st, sp_st = suite_statistics_of_folder(path, model, batch_size, device, num_workers, spatial_stage, spatial_channels)
    return sp_st.mu, sp_st.sigma


def save_statistics_of_path(path, out_path, device=None, batch_size=50, num_workers=8, model=None, spatial_stage=SPATIAL_STAGE,
                            spatial_channels=SPATIAL_CHANNELS):
    """The twin of ``fid_score.save_statistics_of_path`` that writes all four arrays: mu, sigma (pool) and mu_s, sigma_s."""
    device = _inputs.rocm_device(device, "sFID")
    if model is None:
        model = InceptionV3([3]).to(device)
    pool_st, sp_st = suite_statistics_of_folder(path, model, batch_size, device, num_workers, spatial_stage, spatial_channels)
    np.savez(out_path, mu=pool_st.mu, sigma=pool_st.sigma, mu_s=sp_st.mu, sigma_s=sp_st.sigma)


def calculate_sfid_given_paths(paths, device=None, batch_size=50, num_workers=8, model=None, spatial_stage=SPATIAL_STAGE,
                               spatial_channels=SPATIAL_CHANNELS):
    """sFID between two image folders or .npz statistics files (keys ``mu_s`` / ``sigma_s``)."""
    device = _inputs.rocm_device(device, "sFID")
    _inputs.require_paths(paths)
    if model is None and not all(str(p).endswith(".npz") for p in paths):
        model = InceptionV3([3]).to(device)
    stats = [compute_spatial_statistics_of_path(p, model, batch_size, device, num_workers, spatial_stage, spatial_channels)
             for p in paths[:2]]
    return calculate_frechet_distance(stats[0][0], stats[0][1], stats[1][0], stats[1][1])


__all__ = ["SpatialFIDStatistics", "spatial_dims", "load_statistics", "compute_spatial_statistics_of_path",
           "suite_statistics_of_folder", "save_statistics_of_path", "calculate_sfid_given_paths", "STAT_KEYS"]
