"""Attribute-classifier tower on the gfx950 kernels of csrc/resnet.hip: a torchvision-layout ResNet (``BasicBlock`` or the "v1.5"
``Bottleneck``, groups 1) in eval mode -- the form the CelebA-40 attribute classifiers come in (ResNet-18 / 34 / 50 with an ``fc``
of 40 outputs); ``tools/attr_metrics.py`` builds the effect of an attribute edit on it.

The module is assembled from torch's own layer classes in torchvision's nesting, so its ``state_dict`` has exactly torchvision's
keys (``conv1.weight``, ``bn1.running_mean``, ``layer2.0.downsample.1.running_var``, ``fc.bias``, ..., the ``num_batches_tracked``
buffers included) and ``load_state_dict`` is strict.  The layers only hold the tensors: ``forward`` runs the kernels, there is no
CPU path, and the batch norms use their running statistics.  Nothing is ever downloaded: weights come from ``weights=`` (a state
dict saved with ``torch.save``), ``seed=`` or ``ResNet.from_hf`` (a ``transformers`` ``ResNetForImageClassification`` held in
memory); a module built with neither says what is missing at first use, or takes ``load_state_dict``.

Images run at their own size: any H, W >= 32.  ``forward`` takes images in [0, 1] and applies ``(x - mean) / std`` per channel
(ImageNet's values by default) before ``conv1``, which zero-pads the normalised image as torchvision's pipeline does.

Seeded weights (``seed=``) are for tests and benchmarks and are chosen to be well conditioned, by the recipe of
``libs/arcface.py``: He-normal convolution weights; batch norm weights U(0.7, 1.3), running means N(0, 0.2^2), running variances
U(0.5, 1.5), biases N(0, 0.2^2); a block's last batch norm (``bn2`` of a BasicBlock, ``bn3`` of a Bottleneck) with weight and bias
scaled by 0.3, so a block moves its input instead of replacing it; ``fc`` weights N(0, 1 / F), its bias N(0, 0.2^2).  On the
float64 restatement of tests/resnet_stages.py, ``ResNet(**RESNET50, seed=0)`` at 64 x 64 gives logits with a standard deviation
of 0.24 - 0.83 per attribute over 8 unrelated smooth images (mean absolute logit 3.3: the pooled features are positive, so the
logits share an offset), and a copy perturbed at amplitude 0.001, 0.1 and 1.0 moves the logit vector by 0.0012, 0.11 and 1.4
times the mean distance between unrelated images: the response is close to linear, neither chaotic nor constant
(tests/test_resnet_host.py asserts both ends)."""
import ctypes
import os

import torch
import torch.nn as nn

from uspace_amd import _hip
from uspace_amd._blob import PackedWeights, WorkspaceCache

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
RESNET18 = dict(block="basic", layers=(2, 2, 2, 2))
RESNET34 = dict(block="basic", layers=(3, 4, 6, 3))
RESNET50 = dict(block="bottleneck", layers=(3, 4, 6, 3))
RESNET101 = dict(block="bottleneck", layers=(3, 4, 23, 3))


def block_specs(block, layers, planes, stem):
    """[(in, planes, out, stride, downsample)] of the blocks ``layer1.0`` ..: the first block of layers 2 - 4 has stride 2; a
    block has ``downsample`` exactly when stride != 1 or in != out."""
    exp = 4 if block == "bottleneck" else 1
    out, cin = [], stem
    for l, (p, n) in enumerate(zip(planes, layers)):
        for j in range(n):
            s = 2 if (j == 0 and l > 0) else 1
            out.append((cin, p, p * exp, s, s != 1 or cin != p * exp))
            cin = p * exp
    return out


def stage_shapes(H, W, block, layers, planes, stem):
    """[(h, w, c)] of tap stages 0 .. number of blocks (``uspace_resnet_tap``; the last stage, the pooled vector, is not a map)."""
    h, w = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
    h, w = (h + 2 - 3) // 2 + 1, (w + 2 - 3) // 2 + 1
    out = [(h, w, stem)]
    for _cin, _p, cout, s, _ds in block_specs(block, layers, planes, stem):
        h, w = (h - 1) // s + 1, (w - 1) // s + 1
        out.append((h, w, cout))
    return out


def _downsample(cin, cout, stride):
    return nn.Sequential(nn.Conv2d(cin, cout, 1, stride, bias=False), nn.BatchNorm2d(cout))


class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, inplanes, planes, stride, downsample):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(planes, planes, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = _downsample(inplanes, planes, stride) if downsample else None


class Bottleneck(nn.Module):
    """The stride sits on the 3 x 3 convolution (torchvision's "v1.5")."""
    expansion = 4

    def __init__(self, inplanes, planes, stride, downsample):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = _downsample(inplanes, planes * 4, stride) if downsample else None


_HF_PREFIXES = (("resnet.embedder.embedder.convolution.", "conv1."), ("resnet.embedder.embedder.normalization.", "bn1."),
                ("classifier.1.", "fc."))


def hf_key(key):
    """The torchvision name of a ``transformers`` ``ResNetForImageClassification`` state-dict key."""
    for a, b in _HF_PREFIXES:
        if key.startswith(a):
            return b + key[len(a):]
    parts = key.split(".")
    if parts[:3] != ["resnet", "encoder", "stages"] or parts[4] != "layers":
        raise KeyError(f"not a ResNetForImageClassification key: {key!r}")
    head = f"layer{int(parts[3]) + 1}.{parts[5]}."
    rest = parts[6:]
    if rest[0] == "shortcut":
        return head + ("downsample.0." if rest[1] == "convolution" else "downsample.1.") + ".".join(rest[2:])
    if rest[0] == "layer":
        j = int(rest[1]) + 1
        return head + (f"conv{j}." if rest[2] == "convolution" else f"bn{j}.") + ".".join(rest[3:])
    raise KeyError(f"not a ResNetForImageClassification key: {key!r}")


class ResNet(nn.Module):
    """``ResNet(...)(images)``: images [B, 3, H, W] in [0, 1] on the device, any H, W >= 32 -> logits fp32 [B, num_classes]."""

    def __init__(self, block="bottleneck", layers=(3, 4, 6, 3), num_classes=40, planes=(64, 128, 256, 512), stem=64,
                 mean=IMAGENET_MEAN, std=IMAGENET_STD, weights=None, seed=None):
        super().__init__()
        if block not in ("basic", "bottleneck"):
            raise NotImplementedError(f"block must be 'basic' or 'bottleneck', got {block!r} (no groups, no wide variants)")
        layers, planes = tuple(int(n) for n in layers), tuple(int(p) for p in planes)
        exp = 4 if block == "bottleneck" else 1
        if len(layers) != 4 or len(planes) != 4 or min(layers) < 1:
            raise NotImplementedError(f"layers and planes must be four counts, every layer >= 1, got {layers}, {planes}")
        if any(c < 4 or c % 4 or c * e > 2048 for c, e in [(int(stem), 1)] + [(p, exp) for p in planes]):
            raise NotImplementedError(f"channel counts must be multiples of 4 and at most 2048, got stem {stem}, planes {planes} x {exp}")
        if int(num_classes) < 1:
            raise NotImplementedError(f"num_classes must be >= 1, got {num_classes}")
        if len(mean) != 3 or len(std) != 3 or min(std) <= 0:
            raise ValueError(f"mean and std must be three values, std positive, got {mean}, {std}")
        self.block, self.layers, self.planes, self.stem = block, layers, planes, int(stem)
        self.num_classes, self.features_dim = int(num_classes), planes[3] * exp
        self.mean, self.std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
        self.conv1 = nn.Conv2d(3, self.stem, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(self.stem)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        cls = Bottleneck if block == "bottleneck" else BasicBlock
        specs = iter(block_specs(block, layers, planes, self.stem))
        for l, n in enumerate(layers):
            blocks = []
            for _ in range(n):
                cin, p, _cout, s, ds = next(specs)
                blocks.append(cls(cin, p, s, ds))
            setattr(self, f"layer{l + 1}", nn.Sequential(*blocks))
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(self.features_dim, self.num_classes)
        self.eval()
        self._missing = None
        if seed is not None:
            self._seed(seed)
        elif weights is not None:
            if not os.path.exists(weights):
                raise FileNotFoundError(f"ResNet weights not found at {weights}: pass weights= (a torchvision-layout state dict "
                                        "saved with torch.save) or seed=; uspace_amd never downloads")
            self.load_state_dict(torch.load(weights, map_location="cpu"))
        else:
            self._missing = ("this ResNet has no weights: pass weights= (a torchvision-layout state dict saved with torch.save), "
                             "seed=, or call load_state_dict; uspace_amd never downloads")
        for p in self.parameters():
            p.requires_grad = False
        self.cfg = _hip.ResnetConfig(self.stem, (ctypes.c_int * 4)(*planes), (ctypes.c_int * 4)(*layers),
                                     1 if block == "bottleneck" else 0, self.num_classes)
        self._packed = PackedWeights("uspace_resnet_", f"ResNet({block}, {layers})", self._canonical_params, cfg=self.cfg)
        self._ws = WorkspaceCache(2)

    @classmethod
    def from_hf(cls, model, mean=IMAGENET_MEAN, std=IMAGENET_STD):
        """From a ``transformers`` ``ResNetForImageClassification`` held in memory (nothing is fetched).  Only the torchvision
        form converts: ReLU, the stride on the 3 x 3 (``downsample_in_bottleneck=False``), no stride in the first stage."""
        c = model.config
        if c.hidden_act != "relu" or c.downsample_in_bottleneck or c.downsample_in_first_stage or c.num_channels != 3:
            raise NotImplementedError("only hidden_act='relu', downsample_in_bottleneck=False, downsample_in_first_stage=False, "
                                      "num_channels=3 convert to the torchvision layout")
        if c.layer_type not in ("basic", "bottleneck"):
            raise NotImplementedError(f"layer_type {c.layer_type!r}")
        exp = 4 if c.layer_type == "bottleneck" else 1
        if any(h % exp for h in c.hidden_sizes):
            raise NotImplementedError(f"hidden_sizes {c.hidden_sizes} are not multiples of the bottleneck reduction 4")
        m = cls(c.layer_type, tuple(c.depths), c.num_labels, tuple(h // exp for h in c.hidden_sizes), c.embedding_size, mean, std)
        m.load_state_dict({hf_key(k): (v.detach().float() if v.is_floating_point() else v.detach().clone())
                           for k, v in model.state_dict().items()})
        return m

    @torch.no_grad()
    def _seed(self, seed):
        """The well-conditioned seeded weights of the module docstring."""
        g = torch.Generator().manual_seed(int(seed))
        last = "bn3" if self.block == "bottleneck" else "bn2"
        for name, m in self.named_modules():
            if isinstance(m, nn.Conv2d):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / m.weight[0].numel()) ** 0.5)
            elif isinstance(m, nn.Linear):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (1.0 / m.weight.shape[1]) ** 0.5)
                m.bias.copy_(0.2 * torch.randn(m.bias.shape, generator=g))
            elif isinstance(m, nn.BatchNorm2d):
                k = 0.3 if name.startswith("layer") and name.endswith("." + last) else 1.0
                m.weight.copy_(k * (0.7 + 0.6 * torch.rand(m.weight.shape, generator=g)))
                m.bias.copy_(k * 0.2 * torch.randn(m.bias.shape, generator=g))
                m.running_mean.copy_(0.2 * torch.randn(m.running_mean.shape, generator=g))
                m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, generator=g))

    def load_state_dict(self, state_dict, strict=True, assign=False):
        """Strict: a missing or unexpected key, or a wrong shape, raises (torchvision's keys, ``num_batches_tracked`` included)."""
        out = super().load_state_dict(state_dict, strict=True, assign=assign)
        self._missing = None
        return out

    def train(self, mode=True):
        """Eval only: the kernels use the running statistics."""
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

    def _workspace(self, B, H, W, device):
        nbytes = _hip.lib().uspace_resnet_workspace_bytes(ctypes.byref(self.cfg), B, H, W)
        if nbytes == 0:
            raise _hip.UspaceHipError(f"ResNet cannot take {B} images of {H} x {W} in one launch sequence: H and W must be 32 .. 16384; "
                                      "for many large images pass a smaller chunk=")
        return self._ws.take((B, H, W), device, nbytes)

    def stage_shapes(self, H, W):
        return stage_shapes(H, W, self.block, self.layers, self.planes, self.stem)

    @torch.no_grad()
    def preprocess(self, images):
        """images [B, 3, H, W] in [0, 1] on the device -> NHWC fp32 [B, H, W, 3], ``(x - mean_c) / std_c``
        (``uspace_resnet_preprocess``)."""
        _hip.require_device(images, "images")
        if images.dim() != 4 or images.shape[1] != 3 or images.shape[0] < 1:
            raise ValueError(f"expected images [B, 3, H, W], got {tuple(images.shape)}")
        x = images.detach().to(torch.float32).contiguous()
        B, _, H, W = x.shape
        out = torch.empty(B, H, W, 3, dtype=torch.float32, device=x.device)
        mean, std = (ctypes.c_float * 3)(*self.mean), (ctypes.c_float * 3)(*self.std)
        _hip.check(_hip.lib().uspace_resnet_preprocess(_hip.ptr(x), B, H, W, mean, std, _hip.ptr(out), _hip.stream_ptr()),
                   "uspace_resnet_preprocess")
        return out

    @torch.no_grad()
    def forward(self, images, chunk=32, return_pooled=False):
        """Logits fp32 [B, num_classes] (with ``return_pooled`` also the pooled features fp32 [B, F]); ``chunk`` images per launch
        sequence (an image's logits do not depend on it)."""
        x = self.preprocess(images)
        B, H, W, _ = x.shape
        dev = x.device
        blob = self._blob(dev)
        chunk = max(1, min(int(chunk), B))
        ws = self._workspace(chunk, H, W, dev)
        logits = torch.empty(B, self.num_classes, dtype=torch.float32, device=dev)
        pooled = torch.empty(B, self.features_dim, dtype=torch.float32, device=dev) if return_pooled else None
        L = _hip.lib()
        for lo in range(0, B, chunk):
            n = min(chunk, B - lo)
            _hip.check(L.uspace_resnet_forward(ctypes.byref(self.cfg), _hip.ptr(blob), _hip.ptr(ws), ws.numel(), _hip.ptr(x[lo:lo + n]), n,
                                               H, W, _hip.ptr(pooled[lo:lo + n]) if return_pooled else None,
                                               _hip.ptr(logits[lo:lo + n]), _hip.stream_ptr()), "uspace_resnet_forward")
        return (logits, pooled) if return_pooled else logits

    @torch.no_grad()
    def tap(self, images, stage):
        """Test aid (``uspace_resnet_tap``): images as in ``forward`` -> stage 0 the stem after the max pool, 1 + u block u (NHWC
        fp32 [B, h, w, c]), the last stage the pooled vector [B, F]."""
        x = self.preprocess(images)
        B, H, W, _ = x.shape
        dev = x.device
        blob = self._blob(dev)
        shapes = self.stage_shapes(H, W)
        out = torch.empty((B,) + (shapes[stage] if 0 <= stage < len(shapes) else (self.features_dim,)), dtype=torch.float32, device=dev)
        ws = self._workspace(B, H, W, dev)
        _hip.check(_hip.lib().uspace_resnet_tap(ctypes.byref(self.cfg), _hip.ptr(blob), _hip.ptr(ws), ws.numel(), _hip.ptr(x), B, H, W,
                                                int(stage), _hip.ptr(out), _hip.stream_ptr()), "uspace_resnet_tap")
        return out


__all__ = ["ResNet", "RESNET18", "RESNET34", "RESNET50", "RESNET101", "IMAGENET_MEAN", "IMAGENET_STD", "block_specs", "stage_shapes",
           "hf_key"]
