"""How much of the original an edit or an inversion kept: LPIPS, SSIM and PSNR of image pairs on the gfx950 kernels of
csrc/lpips.hip, one fp64 value per pair.  The pairs are what the workflows produce: a u-space ``write`` sweep against the
unedited sample, a p2p / ``local_prompt`` edit against the source prompt's image, the encode -> decode round trip of a real
image (the reference's ``vis_reversible``, which it judges by eye).

``psnr`` and ``ssim`` take any pair of equal-shaped image batches; ``PairMetrics`` accumulates all three over batches of images
in [0, 1]; ``calculate_pair_metrics_given_paths`` pairs two folders by file name; ``reconstruction_fidelity`` is the round trip."""
import numpy as np
import torch

from uspace_amd import _hip
from uspace_amd.tools import _inputs
from uspace_amd.tools.lpips import LPIPS


def _pair(a, b, what):
    for t, name in ((a, "a"), (b, "b")):
        _hip.require_device(t, f"{what}: {name}")
    if a.dim() != 4 or a.shape != b.shape or a.shape[0] < 1:
        raise ValueError(f"{what}: expected two image batches [B, C, H, W] of one shape, got {tuple(a.shape)} and {tuple(b.shape)}")
    return tuple(t.detach().to(torch.float32).contiguous() for t in (a, b))


def _workspace(nbytes, what, device):
    if nbytes == 0:
        raise _hip.UspaceHipError(f"{what}: invalid sizes")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


@torch.no_grad()
def psnr(a, b, data_range=1.0, ws=None):
    """fp64 [B] on the device: 10 log10(data_range^2 / mse) of every pair of a, b [B, C, H, W]; identical images give +inf.
    ``ws``: a uint8 device tensor of ``uspace_psnr_workspace_bytes`` bytes at least (default: allocated here)."""
    x, y = _pair(a, b, "psnr")
    B, n = x.shape[0], x[0].numel()
    L = _hip.lib()
    if ws is None:
        ws = _workspace(L.uspace_psnr_workspace_bytes(B, n), f"uspace_psnr_workspace_bytes({B}, {n})", x.device)
    out = torch.empty(B, dtype=torch.float64, device=x.device)
    _hip.check(L.uspace_psnr_f64(_hip.ptr(x), _hip.ptr(y), B, n, float(data_range), _hip.ptr(ws), ws.numel(), _hip.ptr(out),
                                 _hip.stream_ptr()), "uspace_psnr_f64")
    return out


@torch.no_grad()
def ssim(a, b, data_range=1.0, ws=None):
    """fp64 [B] on the device: the mean structural similarity (Wang et al. 2004) of every pair of a, b [B, C, H, W]: Gaussian
    window of 11 taps, sigma 1.5, over the valid region, K1 = 0.01, K2 = 0.03, averaged over positions and channels.  H or W
    below 11 raises.  ``ws``: a uint8 device tensor of ``uspace_ssim_workspace_bytes`` bytes at least (default: allocated here)."""
    x, y = _pair(a, b, "ssim")
    B, C, H, W = x.shape
    L = _hip.lib()
    if ws is None:
        ws = _workspace(L.uspace_ssim_workspace_bytes(B, C, H, W), f"uspace_ssim_workspace_bytes({B}, {C}, {H}, {W})", x.device)
    out = torch.empty(B, dtype=torch.float64, device=x.device)
    _hip.check(L.uspace_ssim_f64(_hip.ptr(x), _hip.ptr(y), B, C, H, W, float(data_range), _hip.ptr(ws), ws.numel(), _hip.ptr(out),
                                 _hip.stream_ptr()), "uspace_ssim_f64")
    return out


class PairMetrics:
    """Per-pair LPIPS / SSIM / PSNR accumulated over batches.  ``lpips``: an ``LPIPS`` module (e.g. with seeded weights) or a
    weight file's path; with neither, ``LPIPS(net)`` needs its weights at first use and says so.  ``structure``: a
    ``DinoVisionTransformer`` (usually ``DINO_B8``) adds a ``structure`` column, ``dino_metrics.structure_distance`` of every
    pair on that tower's last-layer keys; ``identity``: an ArcFace ``Backbone`` (usually ``IR_SE50``) adds an ``identity`` column,
    ``id_metrics.id_similarity`` of every pair (keyword only).  The defaults None leave the three columns as they are.
    ``attributes``: a property, None by default; set to an ``attr_metrics.AttributeEffect`` before the first ``update`` it adds that
    edit's ``target_shift``, ``target_hit``, ``off_target`` and ``selectivity`` columns (``attr_metrics.attribute_effect`` of every
    pair).  It is not a parameter of ``__init__``, whose parameter list is pinned as it is.  ``parsing``: a property set and read
    the same way; a ``seg_metrics.SegmentationConsistency`` adds its ``column_names`` (``agreement``, ``miou`` and, with a region,
    ``outside_mse``, ``outside_psnr``, ``outside_share``)."""

    def __init__(self, device=None, lpips=None, net="alex", structure=None, *, identity=None):
        self.device = _inputs.rocm_device(device, "PairMetrics")
        self.net = net
        self._lpips = lpips
        self._structure = structure
        self._identity = identity
        self._attributes = None
        self._parsing = None
        self.reset()

    @property
    def parsing(self):
        return self._parsing

    @parsing.setter
    def parsing(self, consistency):
        if self.n:
            raise ValueError("PairMetrics.parsing must be set before the first update (or after reset)")
        self._parsing = consistency
        self.reset()

    @property
    def attributes(self):
        return self._attributes

    @attributes.setter
    def attributes(self, effect):
        if self.n:
            raise ValueError("PairMetrics.attributes must be set before the first update (or after reset)")
        self._attributes = effect
        self.reset()

    @property
    def lpips(self):
        if not isinstance(self._lpips, LPIPS):
            self._lpips = LPIPS(self.net, weights=self._lpips).to(self.device)
        return self._lpips

    def reset(self):
        self._parts = {"lpips": [], "ssim": [], "psnr": []}
        if self._structure is not None:
            self._parts["structure"] = []
        if self._identity is not None:
            self._parts["identity"] = []
        if self._attributes is not None:
            from uspace_amd.tools.attr_metrics import COLUMNS
            self._parts.update({k: [] for k in COLUMNS})
        if self._parsing is not None:
            self._parts.update({k: [] for k in self._parsing.column_names})

    @property
    def n(self):
        return sum(len(p) for p in self._parts["psnr"])

    @property
    def values(self):
        """dict(lpips, ssim, psnr): fp64 numpy arrays, one value per pair seen, in order."""
        return {k: (torch.cat(p).cpu().numpy() if p else np.empty(0)) for k, p in self._parts.items()}

    @torch.no_grad()
    def update(self, original, edited, quantize=True):
        """Add pairs of images [B, 3, H, W] in [0, 1]; ``quantize`` as in ``EvalSuite.update`` (save_image's x * 255 + 0.5 ->
        clamp -> uint8, then / 255), applied to both sides: the numbers of the written PNGs."""
        x, y = (t.detach().to(self.device, torch.float32) for t in (original, edited))
        if quantize:
            x, y = _inputs.quantize(x), _inputs.quantize(y)
        self._parts["lpips"].append(self.lpips(x, y, normalize=True))
        self._parts["ssim"].append(ssim(x, y, 1.0))
        self._parts["psnr"].append(psnr(x, y, 1.0))
        if self._structure is not None:
            from uspace_amd.tools.dino_metrics import structure_distance
            # from the inputs as given: the tower's preprocess applies the same quantisation on integers, before its resize
            xa, xb = (t.detach().to(self.device, torch.float32) for t in (original, edited))
            self._parts["structure"].append(structure_distance(self._structure, xa, xb, quantize=quantize))
        if self._identity is not None:
            from uspace_amd.tools.id_metrics import id_similarity
            self._parts["identity"].append(id_similarity(self._identity, x, y, quantize=False))     # x, y are quantised above
        if self._attributes is not None:
            from uspace_amd.tools.attr_metrics import COLUMNS
            cols = self._attributes.columns(x, y, quantize=False)                                   # fp64 [B, 4]; likewise
            for i, k in enumerate(COLUMNS):
                self._parts[k].append(cols[:, i].contiguous())
        if self._parsing is not None:
            for k, v in self._parsing.columns(x, y, quantize=False).items():                       # fp64 numpy [B]; likewise
                self._parts[k].append(torch.from_numpy(np.ascontiguousarray(v)))

    def compute(self):
        """dict(lpips, ssim, psnr, n) -- with ``structure=`` also ``structure``, with ``identity=`` also ``identity``, with
        ``attributes`` set also its four columns, with ``parsing`` set also its columns --: the means over the pairs seen (numpy fp64 means of ``values``)."""
        v = self.values
        n = len(v["psnr"])
        if n == 0:
            raise ValueError("PairMetrics has seen no pairs")
        out = {k: float(np.mean(a)) for k, a in v.items()}
        out["n"] = n
        return out


def calculate_pair_metrics_given_paths(dir_a, dir_b, device=None, batch_size=50, lpips=None, net="alex"):
    """Mean LPIPS / SSIM / PSNR between the images of two folders paired by file name (``PairMetrics.compute``'s dict).  A name
    present in one folder only, or an image whose size differs from its partner's or from the first pair's, raises ValueError."""
    _names, files_a, files_b = _inputs.paired_image_files(dir_a, dir_b)
    pm = PairMetrics(device=device, lpips=lpips, net=net)
    for xa, xb in zip(_inputs.uint8_batches(files_a, batch_size), _inputs.uint8_batches(files_b, batch_size)):
        pm.update(xa.to(pm.device).float() / 255, xb.to(pm.device).float() / 255, quantize=False)
    return pm.compute()


@torch.no_grad()
def reconstruction_fidelity(cnf, vae, images, cond=None, metrics=None, **kw):
    """The number behind the reference's ``vis_reversible`` picture: images [B, 3, R, R] in [0, 1] -> ``vae.encode`` ->
    ``cnf.encode`` -> ``cnf.decode`` -> ``vae.decode`` -> ``PairMetrics`` of (images, reconstruction).  ``kw`` goes to both solves
    (``solver_kwargs=...``); ``metrics``: the ``PairMetrics`` to add to (default: a new one).  Returns its ``compute()``."""
    pm = metrics if metrics is not None else PairMetrics(device=images.device)
    z = vae.encode(images * 2 - 1)
    noise = cnf.encode(z, cond, **kw)
    z_rec = cnf.decode(noise, cond, **kw)
    rec = (vae.decode(z_rec) * 0.5 + 0.5).clamp(0, 1)
    pm.update(images, rec)
    return pm.compute()


__all__ = ["psnr", "ssim", "PairMetrics", "calculate_pair_metrics_given_paths", "reconstruction_fidelity"]
