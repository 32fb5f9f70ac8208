"""The FID Inception-v3 feature extractor (reference tools/inception.py: InceptionV3 over fid_inception_v3) on the gfx950
kernels of csrc/inception.hip.  There is no CPU path and nothing is ever downloaded: the weights are read from ``weights=``
or from pytorch-fid's cache, ``torch.hub.get_dir()/checkpoints/pt_inception-2015-12-05-6726825d.pth``.

The module's state_dict uses the keys of torchvision's ``Inception3`` (``Conv2d_1a_3x3.conv.weight``,
``Mixed_5b.branch1x1.bn.running_var``, ...), so the pytorch-fid weight file loads directly; its ``fc.*`` and
``*.num_batches_tracked`` entries are accepted and ignored."""
import os

import torch
import torch.nn as nn

from uspace_amd import _hip
from uspace_amd._blob import PackedWeights, WorkspaceCache

FID_WEIGHTS_FILE = "pt_inception-2015-12-05-6726825d.pth"


def _arch():
    """[(name, cin, cout, (kh, kw), stride, (ph, pw))] of the 94 BasicConv2d in torchvision's state_dict order."""
    convs = []

    def c(name, ci, co, k, s=1, p=(0, 0)):
        convs.append((name, ci, co, k, s, p))

    c("Conv2d_1a_3x3", 3, 32, (3, 3), 2)
    c("Conv2d_2a_3x3", 32, 32, (3, 3))
    c("Conv2d_2b_3x3", 32, 64, (3, 3), 1, (1, 1))
    c("Conv2d_3b_1x1", 64, 80, (1, 1))
    c("Conv2d_4a_3x3", 80, 192, (3, 3))
    for blk, cin, pool in (("Mixed_5b", 192, 32), ("Mixed_5c", 256, 64), ("Mixed_5d", 288, 64)):
        c(f"{blk}.branch1x1", cin, 64, (1, 1))
        c(f"{blk}.branch5x5_1", cin, 48, (1, 1))
        c(f"{blk}.branch5x5_2", 48, 64, (5, 5), 1, (2, 2))
        c(f"{blk}.branch3x3dbl_1", cin, 64, (1, 1))
        c(f"{blk}.branch3x3dbl_2", 64, 96, (3, 3), 1, (1, 1))
        c(f"{blk}.branch3x3dbl_3", 96, 96, (3, 3), 1, (1, 1))
        c(f"{blk}.branch_pool", cin, pool, (1, 1))
    c("Mixed_6a.branch3x3", 288, 384, (3, 3), 2)
    c("Mixed_6a.branch3x3dbl_1", 288, 64, (1, 1))
    c("Mixed_6a.branch3x3dbl_2", 64, 96, (3, 3), 1, (1, 1))
    c("Mixed_6a.branch3x3dbl_3", 96, 96, (3, 3), 2)
    for blk, c7 in (("Mixed_6b", 128), ("Mixed_6c", 160), ("Mixed_6d", 160), ("Mixed_6e", 192)):
        c(f"{blk}.branch1x1", 768, 192, (1, 1))
        c(f"{blk}.branch7x7_1", 768, c7, (1, 1))
        c(f"{blk}.branch7x7_2", c7, c7, (1, 7), 1, (0, 3))
        c(f"{blk}.branch7x7_3", c7, 192, (7, 1), 1, (3, 0))
        c(f"{blk}.branch7x7dbl_1", 768, c7, (1, 1))
        c(f"{blk}.branch7x7dbl_2", c7, c7, (7, 1), 1, (3, 0))
        c(f"{blk}.branch7x7dbl_3", c7, c7, (1, 7), 1, (0, 3))
        c(f"{blk}.branch7x7dbl_4", c7, c7, (7, 1), 1, (3, 0))
        c(f"{blk}.branch7x7dbl_5", c7, 192, (1, 7), 1, (0, 3))
        c(f"{blk}.branch_pool", 768, 192, (1, 1))
    c("Mixed_7a.branch3x3_1", 768, 192, (1, 1))
    c("Mixed_7a.branch3x3_2", 192, 320, (3, 3), 2)
    c("Mixed_7a.branch7x7x3_1", 768, 192, (1, 1))
    c("Mixed_7a.branch7x7x3_2", 192, 192, (1, 7), 1, (0, 3))
    c("Mixed_7a.branch7x7x3_3", 192, 192, (7, 1), 1, (3, 0))
    c("Mixed_7a.branch7x7x3_4", 192, 192, (3, 3), 2)
    for blk, cin in (("Mixed_7b", 1280), ("Mixed_7c", 2048)):
        c(f"{blk}.branch1x1", cin, 320, (1, 1))
        c(f"{blk}.branch3x3_1", cin, 384, (1, 1))
        c(f"{blk}.branch3x3_2a", 384, 384, (1, 3), 1, (0, 1))
        c(f"{blk}.branch3x3_2b", 384, 384, (3, 1), 1, (1, 0))
        c(f"{blk}.branch3x3dbl_1", cin, 448, (1, 1))
        c(f"{blk}.branch3x3dbl_2", 448, 384, (3, 3), 1, (1, 1))
        c(f"{blk}.branch3x3dbl_3a", 384, 384, (1, 3), 1, (0, 1))
        c(f"{blk}.branch3x3dbl_3b", 384, 384, (3, 1), 1, (1, 0))
        c(f"{blk}.branch_pool", cin, 192, (1, 1))
    return convs


ARCH = _arch()
# tap stage of each output block (0: first max pool, 1: second max pool, 2: Mixed_6e, 3: Mixed_7c) and its channels
BLOCK_STAGE = (4, 7, 15, 18)
BLOCK_DIMS = (64, 192, 768, 2048)
# output of every tap stage at 299 x 299 (H, W, C); stage 19 is the global mean [B, 2048]
STAGE_SHAPES = ([(299, 299, 3), (149, 149, 32), (147, 147, 32), (147, 147, 64), (73, 73, 64), (73, 73, 80), (71, 71, 192),
                 (35, 35, 192), (35, 35, 256), (35, 35, 288), (35, 35, 288), (17, 17, 768)] + [(17, 17, 768)] * 4
                + [(8, 8, 1280), (8, 8, 2048), (8, 8, 2048), (1, 1, 2048)])
# 2 * MACs of the 94 convolutions at 299 x 299 (the FLOP count of one image)
GFLOP_PER_IMAGE = 11.42
MAX_CHUNK = 256     # images per launch sequence: every NHWC tensor stays far below 2^31 elements
# sFID's spatial features: the first SPATIAL_CHANNELS channels of tap stage SPATIAL_STAGE (Mixed_6d), 17 * 17 * 7 = 2023 values
SPATIAL_STAGE = 14
SPATIAL_CHANNELS = 7
NUM_CLASSES = 1008  # rows of fc.weight in the pytorch-fid weight file


def state_dict_layout():
    """[(key, shape)] of the module's state_dict: torchvision Inception3's keys, conv then BN per BasicConv2d."""
    out = []
    for name, ci, co, (kh, kw), _s, _p in ARCH:
        out.append((f"{name}.conv.weight", (co, ci, kh, kw)))
        for k in ("bn.weight", "bn.bias", "bn.running_mean", "bn.running_var"):
            out.append((f"{name}.{k}", (co,)))
    return out


def default_weights_path():
    return os.path.join(torch.hub.get_dir(), "checkpoints", FID_WEIGHTS_FILE)


class _Conv(nn.Module):
    def __init__(self, ci, co, k):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(co, ci, *k))


class _BN(nn.Module):
    """BatchNorm2d(eps=0.001) in eval form: weight, bias, running_mean, running_var (no num_batches_tracked)."""
    def __init__(self, c):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(c))
        self.bias = nn.Parameter(torch.zeros(c))
        self.register_buffer("running_mean", torch.zeros(c))
        self.register_buffer("running_var", torch.ones(c))


class BasicConv2d(nn.Module):
    def __init__(self, ci, co, k):
        super().__init__()
        self.conv = _Conv(ci, co, k)
        self.bn = _BN(co)


class InceptionV3(nn.Module):
    """Pretrained FID Inception-v3 returning feature maps (reference tools/inception.py), on the HIP kernels."""

    DEFAULT_BLOCK_INDEX = 3
    BLOCK_INDEX_BY_DIM = {64: 0, 192: 1, 768: 2, 2048: 3}

    def __init__(self, output_blocks=(DEFAULT_BLOCK_INDEX,), resize_input=True, normalize_input=True, requires_grad=False,
                 use_fid_inception=True, weights=None, seed=None):
        super().__init__()
        if not resize_input or not normalize_input:
            raise NotImplementedError("the kernels always resize to 299 x 299 and scale [0, 1] to [-1, 1] (the FID setting)")
        if not use_fid_inception:
            raise NotImplementedError("use_fid_inception=False (torchvision's ImageNet Inception) is not provided")
        self.resize_input = resize_input
        self.normalize_input = normalize_input
        self.output_blocks = sorted(output_blocks)
        self.last_needed_block = max(output_blocks)
        assert self.last_needed_block <= 3, "Last possible output block index is 3"
        for name, ci, co, k, _s, _p in ARCH:
            parent = self
            *path, leaf = name.split(".")
            for p in path:
                if not hasattr(parent, p):
                    parent.add_module(p, nn.Module())
                parent = getattr(parent, p)
            parent.add_module(leaf, BasicConv2d(ci, co, k))
        if seed is not None:
            self._seed(seed)
        else:
            path = weights if weights is not None else default_weights_path()
            if not os.path.exists(path):
                raise FileNotFoundError(
                    f"FID Inception weights not found at {path}: place pytorch-fid's {FID_WEIGHTS_FILE} there (or pass "
                    "weights=); uspace_amd never downloads")
            self.load_state_dict(torch.load(path, map_location="cpu"))
        for p in self.parameters():
            p.requires_grad = requires_grad
        self._packed = PackedWeights("uspace_inception_", "Inception", self._canonical_params)
        self._ws = WorkspaceCache(1)

    @torch.no_grad()
    def _seed(self, seed):
        """Seeded random weights for tests: He-scaled convolutions and BN statistics near identity, so activations stay
        O(1) through all 94 layers."""
        g = torch.Generator().manual_seed(int(seed))
        for name, ci, co, (kh, kw), _s, _p in ARCH:
            m = self.get_submodule(name)
            fan_in = ci * kh * kw
            m.conv.weight.copy_(torch.randn(co, ci, kh, kw, generator=g) * (2.0 / fan_in) ** 0.5)
            m.bn.weight.copy_(0.8 + 0.4 * torch.rand(co, generator=g))
            m.bn.bias.copy_(0.2 * torch.rand(co, generator=g) - 0.1)
            m.bn.running_mean.copy_(0.2 * torch.rand(co, generator=g) - 0.1)
            m.bn.running_var.copy_(0.8 + 0.4 * torch.rand(co, generator=g))

    def load_state_dict(self, state_dict, strict=True, assign=False):
        """Loads torchvision Inception3 keys strictly; ``fc.*`` and ``*.num_batches_tracked`` are dropped first.  Any other
        missing or unexpected key, or a wrong shape, raises and names it."""
        sd = {k: v for k, v in state_dict.items() if not (k.startswith("fc.") or k.endswith(".num_batches_tracked"))}
        own = self.state_dict()
        missing = [k for k in own if k not in sd]
        unexpected = [k for k in sd if k not in own]
        if missing or unexpected:
            raise KeyError(f"FID Inception state_dict: missing keys {missing}, unexpected keys {unexpected}")
        for k, v in sd.items():
            if tuple(v.shape) != tuple(own[k].shape):
                raise ValueError(f"FID Inception state_dict: {k} has shape {tuple(v.shape)}, expected {tuple(own[k].shape)}")
        return super().load_state_dict(sd, strict=True, assign=assign)

    def invalidate_packed(self):
        """Forget the packed weight blob; needed only after in-place edits through ``p.data`` (``PackedWeights.invalidate``)."""
        self._packed.invalidate()

    # ------------------------------------------------------------------------------------------------ kernels
    def _canonical_params(self):
        return list(self.state_dict().values())

    def _blob(self, device):
        return self._packed.blob(device)

    def _workspace(self, B, H, W, device):
        return self._ws.take(B, device, _hip.lib().uspace_inception_workspace_bytes(B, H, W))

    def _input(self, inp):
        _hip.require_device(inp, "input")
        if inp.dim() != 4 or inp.shape[1] != 3:
            raise ValueError(f"expected images [B, 3, H, W], got {tuple(inp.shape)}")
        return inp.detach().to(torch.float32).contiguous()

    def _chunks(self, B, chunk):
        chunk = max(1, min(chunk or MAX_CHUNK, MAX_CHUNK, B))
        return chunk, [(lo, min(chunk, B - lo)) for lo in range(0, B, chunk)]

    @torch.no_grad()
    def features(self, inp, block=None, chunk=None):
        """Global spatial mean of output block ``block`` (default: the last needed one): [B, 64 / 192 / 768 / 2048] fp32."""
        block = self.last_needed_block if block is None else int(block)
        x = self._input(inp)
        B, _, H, W = x.shape
        dev = x.device
        blob = self._blob(dev)
        out = torch.empty(B, BLOCK_DIMS[block], dtype=torch.float32, device=dev)
        chunk, parts = self._chunks(B, chunk)
        ws = self._workspace(chunk, H, W, dev)
        L = _hip.lib()
        for lo, n in parts:
            _hip.check(L.uspace_inception_forward(_hip.ptr(blob), _hip.ptr(ws), ws.numel(), _hip.ptr(x[lo:lo + n]), n, H, W,
                                                  block, _hip.ptr(out[lo:lo + n]), _hip.stream_ptr()),
                       "uspace_inception_forward")
        return out

    @torch.no_grad()
    def tap(self, inp, stage, chunk=None):
        """Output of tap stage ``stage`` (0 the resized, normalised input ... 18 Mixed_7c) as NHWC [B, H, W, C], or the
        global mean [B, 2048] for stage 19."""
        x = self._input(inp)
        B, _, H, W = x.shape
        dev = x.device
        blob = self._blob(dev)
        h, w, c = STAGE_SHAPES[stage]
        out = torch.empty((B, c) if stage == 19 else (B, h, w, c), dtype=torch.float32, device=dev)
        chunk, parts = self._chunks(B, chunk)
        ws = self._workspace(chunk, H, W, dev)
        L = _hip.lib()
        for lo, n in parts:
            _hip.check(L.uspace_inception_tap(_hip.ptr(blob), _hip.ptr(ws), ws.numel(), _hip.ptr(x[lo:lo + n]), n, H, W,
                                              int(stage), _hip.ptr(out[lo:lo + n]), _hip.stream_ptr()), "uspace_inception_tap")
        return out

    @torch.no_grad()
    def suite(self, inp, spatial=True, spatial_stage=SPATIAL_STAGE, spatial_channels=SPATIAL_CHANNELS, chunk=None):
        """(pool [B, 2048], spatial [B, h * w * spatial_channels] or None) from ONE walk of the network.

        pool is ``features(inp, 3)`` bit for bit.  spatial is, for image b, ``tap(inp, spatial_stage)[b, :, :, :spatial_channels]``
        flattened in (h, w, c) order, bit for bit.  With the defaults these are sFID's spatial features: stage 14 is Mixed_6d,
        whose concatenated output starts with branch1x1, so they are the first 7 channels of Mixed_6d.branch1x1 after BN and
        ReLU over the 17 x 17 map, 2023 values per image.  That is a reading of ADM's ``mixed_6/conv:0[..., :7]`` (TF's
        mixed_6 taken to be torchvision's Mixed_6d); it has not been checked against the TF graph, which is why both are
        parameters.  ``spatial=False`` skips the gather and returns None in its place."""
        stage, nch = int(spatial_stage), int(spatial_channels)
        x = self._input(inp)
        B, _, H, W = x.shape
        dev = x.device
        blob = self._blob(dev)
        pool = torch.empty(B, BLOCK_DIMS[3], dtype=torch.float32, device=dev)
        if not 1 <= stage <= 18 or not 1 <= nch <= STAGE_SHAPES[stage][2]:      # checked whether or not the gather is asked for
            raise _hip.UspaceHipError(f"spatial_stage must be in 1 .. 18 and spatial_channels in 1 .. the stage's channels, got "
                                      f"{spatial_stage} and {spatial_channels}")
        h, w, _c = STAGE_SHAPES[stage]
        sp = torch.empty(B, h * w * nch, dtype=torch.float32, device=dev) if spatial else None
        chunk, parts = self._chunks(B, chunk)
        ws = self._workspace(chunk, H, W, dev)
        L = _hip.lib()
        for lo, n in parts:
            _hip.check(L.uspace_inception_forward_suite(_hip.ptr(blob), _hip.ptr(ws), ws.numel(), _hip.ptr(x[lo:lo + n]), n, H, W,
                                                        _hip.ptr(pool[lo:lo + n]), _hip.ptr(sp[lo:lo + n]) if sp is not None else None,
                                                        stage, nch, _hip.stream_ptr()), "uspace_inception_forward_suite")
        return pool, sp

    def forward(self, inp):
        """List of the selected output blocks, ascending (reference InceptionV3.forward): blocks 0-2 as feature maps
        [B, C, H, W], block 3 as the pooled [B, 2048, 1, 1]."""
        outp = []
        for idx in self.output_blocks:
            if idx == 3:
                outp.append(self.features(inp, 3)[:, :, None, None])
            else:
                outp.append(self.tap(inp, BLOCK_STAGE[idx]).permute(0, 3, 1, 2))
        return outp


class _FC(nn.Module):
    def __init__(self, k, c):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(c, k))
        self.bias = nn.Parameter(torch.zeros(c))


class InceptionHead(nn.Module):
    """The classification layer of Inception-v3 (torchvision's ``fc``, 2048 -> 1008 in the pytorch-fid weight file), which
    ``InceptionV3`` drops: ``logits = pool @ fc.weight.T + fc.bias`` over the 2048-d pool features of block 3, on
    uspace_inception_logits (fp32 MFMA, a k-ordered fma chain per logit, no activation).

    ``InceptionHead(weights=path_or_None)`` reads ``fc.*`` from the same file as ``InceptionV3`` (``weights=`` or pytorch-fid's
    cache; never downloaded); ``InceptionHead(num_classes=..., seed=..., std=...)`` makes seeded weights for tests.  The number
    of classes is taken from the weight.  These are the logits of the pytorch-fid port of the network, not of the TF graph."""

    def __init__(self, weights=None, num_classes=NUM_CLASSES, seed=None, std=None, in_features=BLOCK_DIMS[3]):
        super().__init__()
        if seed is not None:
            g = torch.Generator().manual_seed(int(seed))
            std = 2.0 / in_features ** 0.5 if std is None else float(std)
            self.fc = _FC(in_features, int(num_classes))
            with torch.no_grad():
                self.fc.weight.copy_(torch.randn(int(num_classes), in_features, generator=g) * std)
                self.fc.bias.copy_(torch.randn(int(num_classes), generator=g) * 0.5)
        else:
            path = weights if weights is not None else default_weights_path()
            if not os.path.exists(path):
                raise FileNotFoundError(
                    f"FID Inception weights not found at {path}: place pytorch-fid's {FID_WEIGHTS_FILE} there (or pass "
                    "weights=); uspace_amd never downloads")
            self.fc = _FC(1, 1)
            self.load_state_dict(torch.load(path, map_location="cpu"))
        for p in self.parameters():
            p.requires_grad = False

    @property
    def num_classes(self):
        return self.fc.weight.shape[0]

    def load_state_dict(self, state_dict, strict=True, assign=False):
        """Keeps ``fc.weight`` [C, K] and ``fc.bias`` [C] of a full torchvision / pytorch-fid state dict and ignores every other
        key.  A dict without ``fc.weight`` or ``fc.bias`` raises KeyError and names the key; a wrong shape raises ValueError."""
        for k in ("fc.weight", "fc.bias"):
            if k not in state_dict:
                raise KeyError(f"Inception head state_dict: missing key {k!r}")
        w, b = torch.as_tensor(state_dict["fc.weight"]), torch.as_tensor(state_dict["fc.bias"])
        if w.dim() != 2 or b.dim() != 1 or b.shape[0] != w.shape[0]:
            raise ValueError(f"Inception head state_dict: fc.weight {tuple(w.shape)} and fc.bias {tuple(b.shape)} do not fit")
        dev = self.fc.weight.device
        self.fc = _FC(w.shape[1], w.shape[0]).to(dev)
        for p in self.fc.parameters():
            p.requires_grad = False
        return super().load_state_dict({"fc.weight": w.detach().float(), "fc.bias": b.detach().float()}, strict=True, assign=assign)

    @torch.no_grad()
    def logits(self, pool, bias=True):
        """fp32 [B, C] = pool @ fc.weight.T + fc.bias for device pool features [B, 2048].  ``bias=False`` drops the bias
        (believed to be torch-fidelity's "unbiased logits" convention; unverified, an option and not a parity claim)."""
        _hip.require_device(pool, "pool features")
        pool = pool.detach().to(torch.float32).contiguous()
        if pool.dim() != 2 or pool.shape[1] != self.fc.weight.shape[1]:
            raise ValueError(f"expected pool features [B, {self.fc.weight.shape[1]}], got {tuple(pool.shape)}")
        w = self.fc.weight.detach()
        if w.device != pool.device:
            raise _hip.UspaceHipError(f"the head lives on {w.device}, the features on {pool.device}: move the head with .to()")
        if pool.shape[0] == 0:
            return torch.empty(0, w.shape[0], dtype=torch.float32, device=pool.device)
        return _hip.inception_logits(pool, w.contiguous(), self.fc.bias.detach().contiguous() if bias else None)

    def forward(self, pool):
        return self.logits(pool)


def fid_inception_v3(weights=None):
    """The FID network up to Mixed_7c with pretrained weights from the local cache (never downloaded)."""
    return InceptionV3(weights=weights)
