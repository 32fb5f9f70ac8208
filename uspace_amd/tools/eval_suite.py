"""The usual generative-model table from ONE Inception pass per batch, straight from decoded samples: FID, sFID and the
Inception Score, and with ``bank=True`` also KID and precision / recall / density / coverage.

``EvalSuite.update`` runs ``InceptionV3.suite`` once per batch and feeds the pool features to a ``FIDStatistics(2048)``, the
head's logits to an ``InceptionScore``, the spatial features to a ``SpatialFIDStatistics`` and, with ``bank=True``, the pool
features to a ``FeatureBank``.  Every number equals what the single-metric tools give on the same images, bit for bit: they
see the same features.  The definitions are theirs (fid_score.py, sfid_score.py, inception_score.py, feature_metrics.py); the
weights are the pytorch-fid port's, so these are that port's numbers, not the TF graph's."""
import numpy as np
import torch

from uspace_amd.tools import _inputs, feature_metrics, sfid_score
from uspace_amd.tools.fid_score import FIDStatistics, calculate_frechet_distance
from uspace_amd.tools.inception import SPATIAL_CHANNELS, SPATIAL_STAGE, InceptionHead, InceptionV3
from uspace_amd.tools.inception_score import InceptionScore


class EvalSuite:
    def __init__(self, device=None, model=None, head=None, bank=False, bias=True, spatial_stage=SPATIAL_STAGE,
                 spatial_channels=SPATIAL_CHANNELS):
        self.device = _inputs.rocm_device(device, "EvalSuite")
        self._model = model
        self._head = head
        self.fid = FIDStatistics(2048, device=self.device, model=model)
        self.sfid = sfid_score.SpatialFIDStatistics(device=self.device, model=model, spatial_stage=spatial_stage,
                                                    spatial_channels=spatial_channels)
        self.inception_score = InceptionScore(device=self.device, model=model, head=head, bias=bias)
        self.bank = feature_metrics.FeatureBank(2048, device=self.device, model=model) if bank else None

    @property
    def model(self):
        if self._model is None:
            self._model = InceptionV3([3]).to(self.device)
        return self._model

    @property
    def head(self):
        if self._head is None:
            self._head = InceptionHead().to(self.device)
            self.inception_score._head = self._head
        return self._head

    @property
    def n(self):
        return self.fid.n

    def reset(self):
        for part in (self.fid, self.sfid, self.inception_score, self.bank):
            if part is not None:
                part.reset()

    @torch.no_grad()
    def update(self, images, quantize=True):
        """Add images [B, 3, H, W] in [0, 1] with one network pass; ``quantize`` as in ``FIDStatistics.update`` (save_image's
        x * 255 + 0.5 -> clamp -> uint8, then / 255)."""
        x = images.detach().to(self.device, torch.float32)
        if quantize:
            x = _inputs.quantize(x)
        pool, spatial = self.model.suite(x, spatial_stage=self.sfid.spatial_stage, spatial_channels=self.sfid.spatial_channels)
        head = self.head
        self.fid.update_features(pool)
        self.sfid.update_features(spatial)
        self.inception_score.update_logits(head.logits(pool, bias=self.inception_score.bias))
        if self.bank is not None:
            self.bank.update_features(pool)

    # ------------------------------------------------------------------------------------------------ statistics and their files
    def statistics(self):
        """dict(mu, sigma, mu_s, sigma_s), each accumulator finalised once (a finalisation copies its fp64 sums to the host)."""
        (mu, sigma), (mu_s, sigma_s) = self.fid._final(), self.sfid._final()
        return dict(mu=mu, sigma=sigma, mu_s=mu_s, sigma_s=sigma_s)

    def save(self, path):
        """np.savez(path, mu, sigma, mu_s, sigma_s): readable by ``fid_score`` (mu / sigma) and ``sfid_score`` (mu_s / sigma_s)."""
        np.savez(path, **self.statistics())

    @staticmethod
    def load(path):
        """dict(mu, sigma, mu_s, sigma_s) of a file ``save`` (or ``sfid_score.save_statistics_of_path``) wrote; a file holding
        only one pair gives only that pair."""
        out = {}
        with np.load(path) as f:
            for k in ("mu", "sigma", "mu_s", "sigma_s"):
                if k in f:
                    out[k] = f[k][:]
        return out

    def _reference(self, real):
        if isinstance(real, EvalSuite):
            return real.statistics(), real.bank
        if isinstance(real, dict):
            return real, None
        return self.load(real), None

    def compute(self, real, splits=10, kid=None, nearest_k=5):
        """dict(fid, sfid, is_mean, is_std) against ``real``: another ``EvalSuite`` or a saved statistics file (a file without one
        of the pairs leaves that distance out).  With feature banks on both sides also kid_mean / kid_std (``kid``: a dict of
        ``kid_score`` keyword arguments) and precision / recall / density / coverage (``nearest_k``)."""
        ref, ref_bank = self._reference(real)
        own = self.statistics()
        out = {}
        if "mu" in ref and "sigma" in ref:
            out["fid"] = float(calculate_frechet_distance(own["mu"], own["sigma"], ref["mu"], ref["sigma"]))
        if "mu_s" in ref and "sigma_s" in ref:
            out["sfid"] = float(calculate_frechet_distance(own["mu_s"], own["sigma_s"], ref["mu_s"], ref["sigma_s"]))
        out["is_mean"], out["is_std"] = self.inception_score.compute(splits)
        if self.bank is not None and ref_bank is not None:
            out["kid_mean"], out["kid_std"] = feature_metrics.kid_score(self.bank, ref_bank, **(kid or {}))
            out.update(feature_metrics.prdc(ref_bank, self.bank, nearest_k=nearest_k))
        return out


__all__ = ["EvalSuite"]
