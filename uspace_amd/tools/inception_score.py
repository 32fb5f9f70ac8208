"""Inception Score on the MI355X (Salimans et al. 2016), from the logits of the HIP Inception-v3: the pool features of
uspace_amd/tools/inception.py through ``InceptionHead`` (torchvision's ``fc``), the statistics in fp64 on the device
(uspace_inception_score_f64 of csrc/inception_score.hip).

Definition.  From logits [N, C] and ``splits`` (default 10), split k covers the rows [k * N // splits, (k + 1) * N // splits).
Within a split
    p_i = softmax(logits_i),   pbar = mean_i p_i,   score_k = exp(mean_i sum_c p_ic (log p_ic - log pbar_c)),
terms with p_ic == 0 contributing 0, and the result is (mean_k score_k, std_k score_k) with ddof = 0.  ``N < splits`` or
``splits < 1`` raises ValueError.

The weights are those of the pytorch-fid port of the network, so these are that port's numbers, not the TF graph's.
``bias=False`` drops ``fc.bias`` from the logits (believed to be torch-fidelity's "unbiased logits"; unverified: an option, not
a parity claim).  There is no CPU path."""
import numpy as np
import torch

from uspace_amd import _hip
from uspace_amd.tools import _inputs
from uspace_amd.tools.inception import BLOCK_DIMS, InceptionHead, InceptionV3


def split_bounds(n, splits):
    """[(lo, hi)] of the ``splits`` row ranges of n rows: [k * n // splits, (k + 1) * n // splits).  ValueError unless
    1 <= splits <= n."""
    if int(splits) != splits or splits < 1:
        raise ValueError(f"splits must be an integer >= 1, got {splits}")
    splits = int(splits)
    if n < splits:
        raise ValueError(f"the Inception Score over {splits} splits needs at least {splits} samples, got {n}")
    return [(k * n // splits, (k + 1) * n // splits) for k in range(splits)]


@torch.no_grad()
def split_scores(logits, splits=10):
    """float64 numpy [splits]: score_k of every split, from device fp32 logits [N, C]."""
    if not torch.is_tensor(logits) or logits.dim() != 2 or logits.shape[1] < 1:
        raise ValueError("logits must be a tensor [N, C]")
    split_bounds(logits.shape[0], splits)
    _hip.require_device(logits, "logits")
    logits = logits.detach().to(torch.float32).contiguous()
    return _hip.inception_score_splits(logits, int(splits)).cpu().numpy()


def inception_score(logits, splits=10):
    """(mean, std) over the splits of exp(mean_i KL(p_i || pbar)) -- see the module docstring -- from device fp32 logits [N, C];
    std with ddof = 0."""
    s = split_scores(logits, splits)
    return float(np.mean(s)), float(np.std(s))


class InceptionScore:
    """Running Inception Score: keeps the fp32 logits [n, C] of everything seen on the device (the score of a split needs the
    split's marginal first, so it cannot be accumulated as sums) and computes on demand.  ``model`` (an ``InceptionV3`` reaching
    block 3) and ``head`` (an ``InceptionHead``) default to the pretrained ones from the local cache."""

    def __init__(self, device=None, model=None, head=None, bias=True):
        self.device = _inputs.rocm_device(device, "the Inception Score")
        self._model = model
        self._head = head
        self.bias = bool(bias)
        self.reset()

    def reset(self):
        self.n = 0
        self._parts = []

    def __len__(self):
        return self.n

    @property
    def model(self):
        if self._model is None:
            self._model = InceptionV3([3]).to(self.device)
        return self._model

    @property
    def head(self):
        if self._head is None:
            self._head = InceptionHead().to(self.device)
        return self._head

    @property
    def logits(self):
        """fp32 [n, C] on the device, in the order the samples were added."""
        if not self._parts:
            return torch.empty(0, self.head.num_classes, dtype=torch.float32, device=self.device)
        if len(self._parts) > 1:
            self._parts = [torch.cat(self._parts)]
        return self._parts[0]

    @torch.no_grad()
    def update(self, images, quantize=True):
        """Add images [B, 3, H, W] in [0, 1], quantised as ``FIDStatistics.update`` does (save_image's x * 255 + 0.5 -> clamp ->
        uint8, then / 255)."""
        x = images.detach().to(self.device, torch.float32)
        self.update_features(self.model.features(_inputs.quantize(x) if quantize else x, 3))

    @torch.no_grad()
    def update_features(self, pool):
        """Add pool features [B, 2048] (fp32 on the device)."""
        if pool.dim() != 2 or pool.shape[1] != BLOCK_DIMS[3]:
            raise ValueError(f"expected features [B, {BLOCK_DIMS[3]}], got {tuple(pool.shape)}")
        _hip.require_device(pool, "features")
        if pool.shape[0] == 0:
            return
        self.update_logits(self.head.logits(pool, bias=self.bias))

    @torch.no_grad()
    def update_logits(self, logits):
        """Add logits [B, C] (fp32 on the device)."""
        _hip.require_device(logits, "logits")
        if logits.dim() != 2 or (self._parts and logits.shape[1] != self._parts[0].shape[1]):
            raise ValueError(f"expected logits [B, C] of one width, got {tuple(logits.shape)}")
        if logits.shape[0] == 0:
            return
        self._parts.append(logits.detach().to(torch.float32).clone())
        self.n += logits.shape[0]

    def compute(self, splits=10):
        """(mean, std) of the split scores of everything added so far."""
        split_bounds(self.n, splits)
        return inception_score(self.logits, splits)


def calculate_is_given_path(path, device=None, batch_size=50, num_workers=8, model=None, head=None, splits=10, bias=True):
    """Inception Score (mean, std) of a folder of images: the files ``fid_score`` would read, in its order and batches."""
    device = _inputs.rocm_device(device, "the Inception Score")
    _inputs.require_paths([path])
    acc = InceptionScore(device=device, model=model, head=head, bias=bias)
    for x in _inputs.unit_batches(_inputs.image_files(path), batch_size, num_workers, device):
        acc.update(x, quantize=False)
    return acc.compute(splits)


__all__ = ["inception_score", "split_scores", "split_bounds", "InceptionScore", "calculate_is_given_path"]
