"""ArcFace identity tower on the gfx950 kernels of csrc/idnet.hip: ``Backbone(input_size, num_layers, mode)`` of TreB1eN's
InsightFace_Pytorch ``model_irse.py`` in eval mode.  ``Backbone(112, 50, "ir_se")`` (the preset ``IR_SE50``) is the class behind
the ``model_ir_se50.pth`` file that the ``IDLoss`` of pSp and e4e loads; ``tools/id_metrics.py`` builds the ID similarity on it.

The module is assembled from torch's own layer classes in the published nesting, so its ``state_dict`` has the published keys
(``input_layer.0.weight``, ``body.3.res_layer.5.fc1.weight``, ``output_layer.3.bias``, ..., the ``num_batches_tracked`` buffers
included) and ``load_state_dict`` is strict.  The layers only hold the tensors: ``forward`` runs the kernels, there is no CPU
path, Dropout is the identity and the batch norms use their running statistics.  Nothing is ever downloaded: weights come from
``weights=`` (a state dict saved with ``torch.save``) or ``seed=``; a module built with neither says what is missing at first
use, or takes ``load_state_dict``.

Seeded weights (``seed=``) are for tests and benchmarks and are chosen to be well conditioned.  PyTorch's default init gives
near-parallel embeddings for unrelated images (cosine about 0.98) and plain He init through 49 convolutions is chaotic (an input
change of 2 % decorrelates the embedding).  The recipe: He-normal convolution, SE and Linear weights; batch norm weights
U(0.7, 1.3), running means N(0, 0.2^2), running variances U(0.5, 1.5), biases N(0, 0.2^2) (the Linear's too); the residual
branch's last batch norm (``res_layer.4``) with weight and bias scaled by 0.3, so a unit moves its input instead of replacing it;
PReLU slopes U(0.05, 0.45).  On a float64 restatement IR-SE50 with seed 0 gives cosines of 1.0000, 0.998, 0.98 and about 0.85
between smooth random images and copies perturbed at amplitude 0.001, 0.1, 0.3 and 1.0, and 0.60 - 0.73 between unrelated images."""
import ctypes
import os

import torch
import torch.nn as nn

from uspace_amd import _hip
from uspace_amd._blob import PackedWeights, WorkspaceCache

BLOCKS = {50: (3, 4, 14, 3), 100: (3, 13, 30, 3), 152: (3, 8, 36, 3)}
WIDTHS = (64, 128, 256, 512)
EMBED_DIM = 512
IR_SE50 = dict(input_size=112, num_layers=50, mode="ir_se")


def unit_specs(blocks):
    """[(in, depth, stride)] of the units ``body.0`` ..: per level one unit (in, depth, 2), then n - 1 units (depth, depth, 1)."""
    out, cin = [], 64
    for depth, n in zip(WIDTHS, blocks):
        out.append((cin, depth, 2))
        out += [(depth, depth, 1)] * (n - 1)
        cin = depth
    return out


def stage_shapes(input_size, blocks):
    """[(h, w, c)] of tap stages 0 .. number of units (``uspace_idnet_tap``; the last stage, the 512-vector, is not a map)."""
    h = input_size
    out = [(h, h, 64)]
    for _cin, depth, stride in unit_specs(blocks):
        h = (h - 1) // stride + 1
        out.append((h, h, depth))
    return out


class SEModule(nn.Module):
    def __init__(self, channels, reduction):
        super().__init__()
        self.avg_pool = nn.AdaptiveAvgPool2d(1)
        self.fc1 = nn.Conv2d(channels, channels // reduction, 1, bias=False)
        self.relu = nn.ReLU(inplace=True)
        self.fc2 = nn.Conv2d(channels // reduction, channels, 1, bias=False)
        self.sigmoid = nn.Sigmoid()


class bottleneck_IR(nn.Module):
    """res_layer(x) + shortcut_layer(x); ``se`` appends the SE module (the published ``bottleneck_IR_SE``)."""

    def __init__(self, in_channel, depth, stride, se):
        super().__init__()
        if in_channel == depth:
            self.shortcut_layer = nn.MaxPool2d(1, stride)
        else:
            self.shortcut_layer = nn.Sequential(nn.Conv2d(in_channel, depth, 1, stride, bias=False), nn.BatchNorm2d(depth))
        layers = [nn.BatchNorm2d(in_channel), nn.Conv2d(in_channel, depth, 3, 1, 1, bias=False), nn.PReLU(depth),
                  nn.Conv2d(depth, depth, 3, stride, 1, bias=False), nn.BatchNorm2d(depth)]
        if se:
            layers.append(SEModule(depth, 16))
        self.res_layer = nn.Sequential(*layers)


class Backbone(nn.Module):
    """``Backbone(...)(x)``: x [B, 3, input_size, input_size] in [-1, 1] on the device -> unit embeddings fp32 [B, 512]."""

    def __init__(self, input_size=112, num_layers=50, mode="ir_se", drop_ratio=0.6, affine=True, weights=None, seed=None,
                 blocks=None):
        super().__init__()
        if blocks is None:
            if num_layers not in BLOCKS:
                raise NotImplementedError(f"num_layers must be one of {sorted(BLOCKS)}, got {num_layers!r}")
            blocks = BLOCKS[num_layers]
        if mode not in ("ir", "ir_se"):
            raise NotImplementedError(f"mode must be 'ir' or 'ir_se', got {mode!r}")
        if not affine:
            raise NotImplementedError("affine=False (an output batch norm without weight and bias) is not supported")
        if input_size < 16 or input_size % 16 or len(blocks) != 4 or min(blocks) < 1:
            raise NotImplementedError(f"input_size must be a positive multiple of 16 and blocks four counts >= 1, got {input_size}, {blocks}")
        self.input_size, self.mode, self.blocks = int(input_size), mode, tuple(int(b) for b in blocks)
        side = self.input_size // 16
        self.input_layer = nn.Sequential(nn.Conv2d(3, 64, 3, 1, 1, bias=False), nn.BatchNorm2d(64), nn.PReLU(64))
        self.output_layer = nn.Sequential(nn.BatchNorm2d(512), nn.Dropout(drop_ratio), nn.Flatten(),
                                          nn.Linear(512 * side * side, EMBED_DIM), nn.BatchNorm1d(EMBED_DIM))
        self.body = nn.Sequential(*[bottleneck_IR(i, d, s, mode == "ir_se") for i, d, s in unit_specs(self.blocks)])
        self.eval()
        self._missing = None
        if seed is not None:
            self._seed(seed)
        elif weights is not None:
            if not os.path.exists(weights):
                raise FileNotFoundError(f"ArcFace weights not found at {weights}: pass weights= (the state dict of "
                                        "InsightFace_Pytorch's Backbone, e.g. model_ir_se50.pth) or seed=; uspace_amd never downloads")
            self.load_state_dict(torch.load(weights, map_location="cpu"))
        else:
            self._missing = ("this ArcFace Backbone has no weights: pass weights= (the state dict of InsightFace_Pytorch's "
                             "Backbone, e.g. model_ir_se50.pth, saved with torch.save), seed=, or call load_state_dict; "
                             "uspace_amd never downloads")
        for p in self.parameters():
            p.requires_grad = False
        self.cfg = _hip.IdnetConfig(self.input_size, (ctypes.c_int * 4)(*self.blocks), 1 if mode == "ir_se" else 0)
        self._packed = PackedWeights("uspace_idnet_", f"ArcFace Backbone({mode}, {self.blocks})", self._canonical_params, cfg=self.cfg)
        self._ws = WorkspaceCache(2)

    @torch.no_grad()
    def _seed(self, seed):
        """The well-conditioned seeded weights of the module docstring."""
        g = torch.Generator().manual_seed(int(seed))
        for name, m in self.named_modules():
            if isinstance(m, (nn.Conv2d, nn.Linear)):
                fan_in = m.weight[0].numel()
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / fan_in) ** 0.5)
                if getattr(m, "bias", None) is not None:
                    m.bias.copy_(0.2 * torch.randn(m.bias.shape, generator=g))
            elif isinstance(m, (nn.BatchNorm2d, nn.BatchNorm1d)):
                k = 0.3 if name.endswith("res_layer.4") else 1.0
                m.weight.copy_(k * (0.7 + 0.6 * torch.rand(m.weight.shape, generator=g)))
                m.bias.copy_(k * 0.2 * torch.randn(m.bias.shape, generator=g))
                m.running_mean.copy_(0.2 * torch.randn(m.running_mean.shape, generator=g))
                m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, generator=g))
            elif isinstance(m, nn.PReLU):
                m.weight.copy_(0.05 + 0.4 * torch.rand(m.weight.shape, generator=g))

    def load_state_dict(self, state_dict, strict=True, assign=False):
        """Strict: a missing or unexpected key, or a wrong shape, raises (the published keys, ``num_batches_tracked`` included)."""
        out = super().load_state_dict(state_dict, strict=True, assign=assign)
        self._missing = None
        return out

    def train(self, mode=True):
        """Eval only: the kernels use the running statistics and no dropout."""
        return super().train(False)

    def invalidate_packed(self):
        """Forget the packed weight blob; needed only after in-place edits through ``p.data`` (``PackedWeights.invalidate``)."""
        self._packed.invalidate()

    # ------------------------------------------------------------------------------------------------ kernels
    def _canonical_params(self):
        return [v for k, v in self.state_dict().items() if not k.endswith("num_batches_tracked")]

    def _blob(self, device):
        if self._missing:
            raise FileNotFoundError(self._missing)
        return self._packed.blob(device)

    def _workspace(self, B, device):
        nbytes = _hip.lib().uspace_idnet_workspace_bytes(ctypes.byref(self.cfg), B)
        if nbytes == 0:
            raise _hip.UspaceHipError(f"ArcFace Backbone cannot take {B} images in one launch sequence: pass a smaller chunk=")
        return self._ws.take(B, device, nbytes)

    @torch.no_grad()
    def preprocess(self, images, normalize=False, crop=True):
        """images fp32 [B, 3, H, W] on the device -> NHWC fp32 [B, input_size, input_size, 3] (``uspace_idnet_preprocess``):
        ``normalize`` maps [0, 1] to [-1, 1] first; ``crop`` is the pool to 256 x 256, crop [35:223, 32:220], pool of pSp / e4e;
        without it the whole image is pooled to ``input_size``."""
        _hip.require_device(images, "images")
        if images.dim() != 4 or images.shape[1] != 3 or images.shape[0] < 1:
            raise ValueError(f"expected images [B, 3, H, W], got {tuple(images.shape)}")
        x = images.detach().to(torch.float32).contiguous()
        B, _, H, W = x.shape
        out = torch.empty(B, self.input_size, self.input_size, 3, dtype=torch.float32, device=x.device)
        _hip.check(_hip.lib().uspace_idnet_preprocess(_hip.ptr(x), B, H, W, 1 if normalize else 0, 1 if crop else 0, self.input_size,
                                                      _hip.ptr(out), _hip.stream_ptr()), "uspace_idnet_preprocess")
        return out

    def _nhwc(self, x_nhwc):
        _hip.require_device(x_nhwc, "x_nhwc")
        S = self.input_size
        if x_nhwc.dim() != 4 or tuple(x_nhwc.shape[1:]) != (S, S, 3) or x_nhwc.shape[0] < 1 or x_nhwc.dtype != torch.float32:
            raise ValueError(f"expected fp32 NHWC [B, {S}, {S}, 3], got {x_nhwc.dtype} {tuple(x_nhwc.shape)}")
        return x_nhwc.contiguous()

    @torch.no_grad()
    def embed_nhwc(self, x_nhwc, chunk=32):
        """``preprocess``'s output -> unit embeddings fp32 [B, 512]; ``chunk`` images per launch sequence (an image's embedding
        does not depend on it)."""
        x = self._nhwc(x_nhwc)
        B, dev = x.shape[0], x.device
        blob = self._blob(dev)
        chunk = max(1, min(int(chunk), B))
        ws = self._workspace(chunk, dev)
        out = torch.empty(B, EMBED_DIM, dtype=torch.float32, device=dev)
        L = _hip.lib()
        for lo in range(0, B, chunk):
            n = min(chunk, B - lo)
            _hip.check(L.uspace_idnet_forward(ctypes.byref(self.cfg), _hip.ptr(blob), _hip.ptr(ws), ws.numel(), _hip.ptr(x[lo:lo + n]), n,
                                              _hip.ptr(out[lo:lo + n]), _hip.stream_ptr()), "uspace_idnet_forward")
        return out

    def _aligned(self, x):
        _hip.require_device(x, "x")
        S = self.input_size
        if x.dim() != 4 or tuple(x.shape[1:]) != (3, S, S) or x.shape[0] < 1:
            raise ValueError(f"expected x [B, 3, {S}, {S}], got {tuple(x.shape)}")
        return self.preprocess(x, normalize=False, crop=False)      # windows of one pixel: the NCHW -> NHWC copy

    def forward(self, x, chunk=32):
        return self.embed_nhwc(self._aligned(x), chunk)

    @torch.no_grad()
    def tap(self, x, stage):
        """Test aid (``uspace_idnet_tap``): x as in ``forward`` (or NHWC fp32 [B, S, S, 3]) -> stage 0 ``input_layer``, 1 + u unit u
        (NHWC fp32 [B, h, w, c]), the last stage the 512-vector before the l2 normalisation [B, 512]."""
        xn = self._nhwc(x) if x.shape[-1] == 3 and x.shape[1] != 3 else self._aligned(x)
        B, dev = xn.shape[0], xn.device
        blob = self._blob(dev)
        shapes = stage_shapes(self.input_size, self.blocks)
        out = torch.empty((B,) + (shapes[stage] if 0 <= stage < len(shapes) else (EMBED_DIM,)), dtype=torch.float32, device=dev)
        ws = self._workspace(B, dev)
        _hip.check(_hip.lib().uspace_idnet_tap(ctypes.byref(self.cfg), _hip.ptr(blob), _hip.ptr(ws), ws.numel(), _hip.ptr(xn), B,
                                               int(stage), _hip.ptr(out), _hip.stream_ptr()), "uspace_idnet_tap")
        return out

    @torch.no_grad()
    def unit(self, index, x_nhwc):
        """Test aid (``uspace_idnet_unit``): unit ``index`` alone on any map NHWC fp32 [B, H, W, in] -> [B, ho, wo, depth]."""
        _hip.require_device(x_nhwc, "x_nhwc")
        specs = unit_specs(self.blocks)
        if not 0 <= index < len(specs):
            raise ValueError(f"unit index {index} outside 0 .. {len(specs) - 1}")
        cin, depth, stride = specs[index]
        if x_nhwc.dim() != 4 or x_nhwc.shape[3] != cin or x_nhwc.dtype != torch.float32 or x_nhwc.shape[0] < 1:
            raise ValueError(f"expected fp32 NHWC [B, H, W, {cin}], got {x_nhwc.dtype} {tuple(x_nhwc.shape)}")
        x = x_nhwc.contiguous()
        B, H, W, _ = x.shape
        blob = self._blob(x.device)
        L = _hip.lib()
        nbytes = L.uspace_idnet_unit_workspace_bytes(ctypes.byref(self.cfg), index, B, H, W)
        if nbytes == 0:
            raise _hip.UspaceHipError(f"uspace_idnet_unit_workspace_bytes({index}, {B}, {H}, {W}): invalid sizes")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        out = torch.empty(B, (H - 1) // stride + 1, (W - 1) // stride + 1, depth, dtype=torch.float32, device=x.device)
        _hip.check(L.uspace_idnet_unit(ctypes.byref(self.cfg), _hip.ptr(blob), _hip.ptr(ws), nbytes, index, _hip.ptr(x), B, H, W,
                                       _hip.ptr(out), _hip.stream_ptr()), "uspace_idnet_unit")
        return out


def similarity(ea, eb):
    """fp64 [B] on the device: the dot products of two sets of embeddings fp32 [B, 512] (``uspace_idnet_similarity_f64``)."""
    for t, name in ((ea, "ea"), (eb, "eb")):
        _hip.require_device(t, name)
        if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != EMBED_DIM or not t.is_contiguous() or t.shape[0] < 1:
            raise _hip.UspaceHipError(f"{name} must be a contiguous fp32 [B, {EMBED_DIM}] tensor, got {t.dtype} {tuple(t.shape)}")
    if ea.shape != eb.shape:
        raise _hip.UspaceHipError(f"embedding sets of different shapes: {tuple(ea.shape)} and {tuple(eb.shape)}")
    out = torch.empty(ea.shape[0], dtype=torch.float64, device=ea.device)
    _hip.check(_hip.lib().uspace_idnet_similarity_f64(_hip.ptr(ea), _hip.ptr(eb), ea.shape[0], _hip.ptr(out), _hip.stream_ptr()),
               "uspace_idnet_similarity_f64")
    return out


__all__ = ["Backbone", "IR_SE50", "BLOCKS", "EMBED_DIM", "unit_specs", "stage_shapes", "similarity"]
