"""LPIPS (Zhang et al. 2018, "The Unreasonable Effectiveness of Deep Features as a Perceptual Metric") on the gfx950 kernels
of csrc/lpips.hip: the AlexNet and VGG-16 feature stacks with the linear heads of the ``lpips`` package.  There is no CPU path
and nothing is ever downloaded: pretrained weights are read from ``weights=``, seeded weights come from ``seed=``.

The module's state_dict uses its own keys: ``features.{i}.weight`` / ``features.{i}.bias`` with torchvision's indices into
``alexnet().features`` / ``vgg16().features``, and ``lin{k}.weight`` [C_k], k = 0 .. 4.  ``load_state_dict`` also accepts the
keys of the published files merged into one dict: torchvision's ``features.N.*`` (its ``classifier.*`` entries are ignored)
together with the lpips package's ``lin{k}.model.1.weight`` [1, C_k, 1, 1].  That mapping is
written from the published layouts and has not been checked against the files, which were not available when this was written."""
import os

import torch
import torch.nn as nn

from uspace_amd import _hip
from uspace_amd._blob import PackedWeights, WorkspaceCache

NETS = {"alex": 0, "vgg": 1}
# (index in torchvision's features, cin, cout, kernel, stride, padding)
_ALEX = [(0, 3, 64, 11, 4, 2), (3, 64, 192, 5, 1, 2), (6, 192, 384, 3, 1, 1), (8, 384, 256, 3, 1, 1), (10, 256, 256, 3, 1, 1)]
_VGG = [(i, ci, co, 3, 1, 1) for i, ci, co in (
    (0, 3, 64), (2, 64, 64), (5, 64, 128), (7, 128, 128), (10, 128, 256), (12, 256, 256), (14, 256, 256), (17, 256, 512),
    (19, 512, 512), (21, 512, 512), (24, 512, 512), (26, 512, 512), (28, 512, 512))]
CONVS = {"alex": _ALEX, "vgg": _VGG}
TAP_CHANNELS = {"alex": (64, 192, 384, 256, 256), "vgg": (64, 128, 256, 512, 512)}
WORKSPACE_TARGET = 1 << 30      # bytes: the default chunk keeps one launch sequence's workspace below this


def stage_shapes(net, H, W):
    """[(h, w, c)] of tap stages 0 .. 5 for an H x W input (stage 0 is the scaled input), as ``uspace_lpips_tap`` numbers them."""
    out = [(H, W, 3)]
    h, w = H, W
    if net == "alex":
        for k, (_i, _ci, co, ks, s, p) in enumerate(_ALEX):
            if k in (1, 2):
                h, w = (h - 3) // 2 + 1, (w - 3) // 2 + 1
            h, w = (h + 2 * p - ks) // s + 1, (w + 2 * p - ks) // s + 1
            out.append((h, w, co))
    elif net == "vgg":
        for k, c in enumerate(TAP_CHANNELS["vgg"]):
            if k:
                h, w = h // 2, w // 2
            out.append((h, w, c))
    else:
        raise ValueError(f"net must be one of {sorted(NETS)}, got {net!r}")
    return out


def state_dict_layout(net):
    """[(key, shape)] of the module's state_dict: weight then bias per convolution, then lin0 .. lin4."""
    if net not in NETS:
        raise ValueError(f"net must be one of {sorted(NETS)}, got {net!r}")
    out = []
    for i, ci, co, k, _s, _p in CONVS[net]:
        out.append((f"features.{i}.weight", (co, ci, k, k)))
        out.append((f"features.{i}.bias", (co,)))
    for k, c in enumerate(TAP_CHANNELS[net]):
        out.append((f"lin{k}.weight", (c,)))
    return out


def map_state_dict(state_dict, net):
    """The module's own keys from a dict in either naming (see the module docstring).  Keys that belong to neither raise KeyError."""
    own = dict(state_dict_layout(net))
    out = {}
    unexpected = []
    for key, v in state_dict.items():
        k = key
        if k.startswith("classifier."):
            continue
        v = torch.as_tensor(v)
        for j in range(5):
            if k == f"lin{j}.model.1.weight":
                k, v = f"lin{j}.weight", v.reshape(-1)
        if k in own:
            out[k] = v
        else:
            unexpected.append(key)
    missing = [k for k in own if k not in out]
    if missing or unexpected:
        raise KeyError(f"LPIPS({net}) state_dict: missing keys {missing}, unexpected keys {unexpected}")
    for k, v in out.items():
        if tuple(v.shape) != tuple(own[k]):
            raise ValueError(f"LPIPS({net}) state_dict: {k} has shape {tuple(v.shape)}, expected {tuple(own[k])}")
    return out


class _Conv(nn.Module):
    def __init__(self, ci, co, k):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(co, ci, k, k))
        self.bias = nn.Parameter(torch.zeros(co))


class _Lin(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(c))


class LPIPS(nn.Module):
    """``LPIPS(net)(img0, img1)``: fp64 [B] on the device, the learned perceptual distance of every pair."""

    def __init__(self, net="alex", weights=None, seed=None):
        super().__init__()
        if net not in NETS:
            raise ValueError(f"net must be one of {sorted(NETS)}, got {net!r}")
        self.net = net
        self.features = nn.Module()
        for i, ci, co, k, _s, _p in CONVS[net]:
            self.features.add_module(str(i), _Conv(ci, co, k))
        for k, c in enumerate(TAP_CHANNELS[net]):
            self.add_module(f"lin{k}", _Lin(c))
        if seed is not None:
            self._seed(seed)
        else:
            if weights is None or not os.path.exists(weights):
                raise FileNotFoundError(
                    f"LPIPS({net}) weights not found at {weights}: pass weights= (a state dict of torchvision's {net} features and "
                    "the lpips package's linear layers) or seed=; uspace_amd never downloads")
            self.load_state_dict(torch.load(weights, map_location="cpu"))
        for p in self.parameters():
            p.requires_grad = False
        self._packed = PackedWeights("uspace_lpips_", f"LPIPS({net})", self._canonical_params, cfg=NETS[net])
        self._ws = WorkspaceCache(1)

    @torch.no_grad()
    def _seed(self, seed):
        """Seeded random weights for tests: He-scaled convolutions with small biases, non-negative linear weights (the trained
        ones are non-negative)."""
        g = torch.Generator().manual_seed(int(seed))
        for i, ci, co, k, _s, _p in CONVS[self.net]:
            m = getattr(self.features, str(i))
            m.weight.copy_(torch.randn(co, ci, k, k, generator=g) * (2.0 / (ci * k * k)) ** 0.5)
            m.bias.copy_(0.2 * torch.rand(co, generator=g) - 0.1)
        for k, c in enumerate(TAP_CHANNELS[self.net]):
            getattr(self, f"lin{k}").weight.copy_(torch.rand(c, generator=g) * (2.0 / c))

    def load_state_dict(self, state_dict, strict=True, assign=False):
        """Loads the module's own keys or the published ones (``map_state_dict``); a missing or unexpected key raises KeyError, a
        wrong shape ValueError, and names it."""
        return super().load_state_dict(map_state_dict(state_dict, self.net), strict=True, assign=assign)

    def invalidate_packed(self):
        """Forget the packed weight blob; needed only after in-place edits through ``p.data`` (``PackedWeights.invalidate``)."""
        self._packed.invalidate()

    # ------------------------------------------------------------------------------------------------ kernels
    def _canonical_params(self):
        return list(self.state_dict().values())

    def _packed_blob(self, device):
        return self._packed.blob(device)

    def _workspace(self, B, H, W, device):
        nbytes = _hip.lib().uspace_lpips_workspace_bytes(NETS[self.net], B, H, W)
        if nbytes == 0:
            raise _hip.UspaceHipError(f"LPIPS({self.net}) cannot take {B} pairs of {H} x {W} images (too small for the network, or "
                                      "too many elements for one launch sequence: pass a smaller chunk=)")
        return self._ws.take(B, device, nbytes)

    def _inputs(self, img0, img1):
        for t, name in ((img0, "img0"), (img1, "img1")):
            _hip.require_device(t, name)
        if img0.dim() != 4 or img0.shape[1] != 3 or img0.shape != img1.shape or img0.shape[0] < 1:
            raise ValueError(f"expected two image batches [B, 3, H, W] of one shape, got {tuple(img0.shape)} and {tuple(img1.shape)}")
        return tuple(t.detach().to(torch.float32).contiguous() for t in (img0, img1))

    def default_chunk(self, B, H, W):
        """The most pairs per launch sequence whose workspace stays below WORKSPACE_TARGET (at least 1, at most B)."""
        per_pair = max(1, _hip.lib().uspace_lpips_workspace_bytes(NETS[self.net], 1, H, W))
        return max(1, min(B, WORKSPACE_TARGET // per_pair))

    def _chunks(self, B, H, W, chunk):
        chunk = max(1, min(int(chunk), B)) if chunk else self.default_chunk(B, H, W)
        return chunk, [(lo, min(chunk, B - lo)) for lo in range(0, B, chunk)]

    @torch.no_grad()
    def forward(self, img0, img1, normalize=False, per_layer=False, chunk=None):
        """fp64 [B] on the device: the distance of every pair (``normalize=False``: images in [-1, 1]; ``True``: in [0, 1]).  With
        ``per_layer`` also the five layers' terms, fp64 [5, B]: (total, layers), total = layers summed in layer order.  ``chunk``:
        pairs per launch sequence (default: what keeps the workspace below 1 GiB); a pair's value does not depend on it."""
        x0, x1 = self._inputs(img0, img1)
        B, _, H, W = x0.shape
        dev = x0.device
        blob = self._packed.blob(dev)
        out = torch.empty(B, dtype=torch.float64, device=dev)
        layers = torch.empty(5, B, dtype=torch.float64, device=dev) if per_layer else None
        chunk, parts = self._chunks(B, H, W, chunk)
        ws = self._workspace(chunk, H, W, dev)
        L = _hip.lib()
        for lo, n in parts:
            part = torch.empty(5, n, dtype=torch.float64, device=dev) if per_layer else None
            _hip.check(L.uspace_lpips_forward(NETS[self.net], _hip.ptr(blob), _hip.ptr(ws), ws.numel(), _hip.ptr(x0[lo:lo + n]),
                                              _hip.ptr(x1[lo:lo + n]), n, H, W, 1 if normalize else 0, _hip.ptr(out[lo:lo + n]),
                                              _hip.ptr(part), _hip.stream_ptr()), "uspace_lpips_forward")
            if per_layer:
                layers[:, lo:lo + n] = part
        return (out, layers) if per_layer else out

    @torch.no_grad()
    def tap(self, img0, img1, stage, normalize=False):
        """Test aid: the activations of tap stage ``stage`` (0 the scaled input, 1 .. 5 the taps) as NHWC [2B, h, w, c], img0's
        images first."""
        x0, x1 = self._inputs(img0, img1)
        B, _, H, W = x0.shape
        dev = x0.device
        blob = self._packed.blob(dev)
        h, w, c = stage_shapes(self.net, H, W)[stage]
        out = torch.empty(2 * B, h, w, c, dtype=torch.float32, device=dev)
        ws = self._workspace(B, H, W, dev)
        _hip.check(_hip.lib().uspace_lpips_tap(NETS[self.net], _hip.ptr(blob), _hip.ptr(ws), ws.numel(), _hip.ptr(x0), _hip.ptr(x1), B,
                                               H, W, 1 if normalize else 0, int(stage), _hip.ptr(out), _hip.stream_ptr()),
                   "uspace_lpips_tap")
        return out


def lpips_distance(f0, f1, w, ws=None):
    """The distance head alone (``uspace_lpips_distance_f64``): f0, f1 fp32 [B, HW, C] on the device, w fp32 [C] -> fp64 [B]."""
    for t, name in ((f0, "f0"), (f1, "f1"), (w, "w")):
        _hip.require_device(t, name)
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise _hip.UspaceHipError(f"{name} must be a contiguous fp32 tensor, got {t.dtype} {tuple(t.shape)}")
    if f0.dim() != 3 or f0.shape != f1.shape or tuple(w.shape) != (f0.shape[2],):
        raise _hip.UspaceHipError(f"expected f0, f1 [B, HW, C] and w [C], got {tuple(f0.shape)}, {tuple(f1.shape)}, {tuple(w.shape)}")
    B, HW, C = f0.shape
    L = _hip.lib()
    if ws is None:
        nbytes = L.uspace_lpips_distance_workspace_bytes(B, HW, C)
        if nbytes == 0:
            raise _hip.UspaceHipError(f"uspace_lpips_distance_workspace_bytes({B}, {HW}, {C}): invalid sizes")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=f0.device)
    out = torch.empty(B, dtype=torch.float64, device=f0.device)
    _hip.check(L.uspace_lpips_distance_f64(_hip.ptr(f0), _hip.ptr(f1), _hip.ptr(w), B, HW, C, _hip.ptr(ws), ws.numel(), _hip.ptr(out),
                                           _hip.stream_ptr()), "uspace_lpips_distance_f64")
    return out


__all__ = ["LPIPS", "NETS", "CONVS", "TAP_CHANNELS", "stage_shapes", "state_dict_layout", "map_state_dict", "lpips_distance"]
