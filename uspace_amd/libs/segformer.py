"""SegFormer on the gfx950 kernels of csrc/segformer.hip and csrc/attention_kv.hip: the MiT encoder (B1 .. B5: head dim 64) with
the all-MLP decode head, in the layout of ``transformers``' ``SegformerForSemanticSegmentation`` in eval mode -- the form the
published face-parsing (CelebAMask-HQ, 19 classes), ADE20K and Cityscapes checkpoints come in.  ``tools/seg_metrics.py`` builds
the segmentation consistency of an edit on its label maps.

The module is assembled from torch's own layer classes in that model's nesting, so its ``state_dict`` has exactly its keys and
shapes (``segformer.stages.2.blocks.0.attention.sequence_reduction.layer_norm.weight``, ``decode_head.batch_norm.running_var``,
..., ``num_batches_tracked`` included) and ``load_state_dict`` is strict.  The layers only hold the tensors: the methods run the
kernels, there is no CPU path, the batch norm uses its running statistics, and every epsilon is read, at every call, from the
module that holds it (the norms of one kind -- patch embeddings, blocks, sequence reductions, stage ends -- must agree).  Nothing
is ever downloaded: weights come from ``weights=`` (a state dict saved with ``torch.save``), ``seed=`` or ``SegFormer.from_hf``
(a model held in memory); a module built with none of these says what is missing at first use, or takes
``load_state_dict``.

Images are [B, 3, H, W] in [0, 1], normalised with ImageNet's mean and std, and run at their own size (H, W from 32; every
reduced key map at most 336 positions, which is images up to about 576^2 with the published ``sr_ratios``); no resize is applied
(INTEGRATION.md says what ``transformers``' image processor would do).  ``logits`` are fp32 [B, L, H/4, W/4]; ``labels`` is
``post_process_semantic_segmentation``: bilinear resize of the logits to the image size (``align_corners=False``), then argmax
with the lowest index on ties, fused in one kernel that never stores the full-size logits.

Refused with ``NotImplementedError``: a head dim other than 64 (MiT-B0), hidden sizes that are no multiple of 64, more than 256
labels; at first use: images below 32 or whose reduced key map exceeds 336 positions.

Seeded weights (``seed=``) are for tests and benchmarks and are chosen to be well conditioned, by the recipe of
``libs/resnet.py``: Linear and convolution weights N(0, 1 / fan_in) (``o_proj``, ``fc2`` scaled by 0.5 so that a block moves its
input instead of replacing it), biases N(0, 0.1^2); LayerNorm weights U(0.8, 1.2), biases N(0, 0.1^2); the batch norm's weight
U(0.7, 1.3), bias N(0, 0.2^2), running mean N(0, 0.2^2), running variance U(0.5, 1.5).  tests/test_segformer_host.py asserts on
the float64 restatement that the label maps of smooth test images are not degenerate."""
import ctypes
import os

import torch
import torch.nn as nn

from uspace_amd import _hip
from uspace_amd._blob import PackedWeights, WorkspaceCache
from uspace_amd.libs.resnet import IMAGENET_MEAN, IMAGENET_STD

_MIT = dict(num_attention_heads=(1, 2, 5, 8), sr_ratios=(8, 4, 2, 1), mlp_ratios=(4, 4, 4, 4), hidden_sizes=(64, 128, 320, 512))
MIT_B1 = dict(_MIT, depths=(2, 2, 2, 2), decoder_hidden_size=256)
MIT_B2 = dict(_MIT, depths=(3, 4, 6, 3), decoder_hidden_size=768)
MIT_B3 = dict(_MIT, depths=(3, 4, 18, 3), decoder_hidden_size=768)
MIT_B4 = dict(_MIT, depths=(3, 8, 27, 3), decoder_hidden_size=768)
MIT_B5 = dict(_MIT, depths=(3, 6, 40, 3), decoder_hidden_size=768)


def stage_maps(H, W):
    """[(h, w)] of the four encoder stages for an H x W image."""
    out, h, w = [], H, W
    for i in range(4):
        k, s, p = (7, 4, 3) if i == 0 else (3, 2, 1)
        h, w = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
        out.append((h, w))
    return out


def _holder(**children):
    m = nn.Module()
    for k, v in children.items():
        m.add_module(k, v)
    return m


def _block(C, sr, hidden):
    att = _holder(q_proj=nn.Linear(C, C), k_proj=nn.Linear(C, C), v_proj=nn.Linear(C, C), o_proj=nn.Linear(C, C))
    if sr > 1:
        att.add_module("sequence_reduction", _holder(sequence_reduction=nn.Conv2d(C, C, sr, sr), layer_norm=nn.LayerNorm(C)))
    mlp = _holder(fc1=nn.Linear(C, hidden), dwconv=_holder(dwconv=nn.Conv2d(hidden, hidden, 3, 1, 1, groups=hidden)), fc2=nn.Linear(hidden, C))
    return _holder(layernorm_before=nn.LayerNorm(C), attention=att, layernorm_after=nn.LayerNorm(C), mlp=mlp)


class SegFormer(nn.Module):
    """``SegFormer(**MIT_B5, num_labels=19, weights=path)``: ``labels(images)`` uint8 [B, H, W], ``logits(images)`` fp32
    [B, L, H/4, W/4] for images [B, 3, H, W] in [0, 1] on the device."""

    def __init__(self, hidden_sizes=(64, 128, 320, 512), depths=(2, 2, 2, 2), num_attention_heads=(1, 2, 5, 8), sr_ratios=(8, 4, 2, 1),
                 mlp_ratios=(4, 4, 4, 4), decoder_hidden_size=256, num_labels=19, mean=IMAGENET_MEAN, std=IMAGENET_STD, weights=None,
                 seed=None):
        super().__init__()
        cfg = [tuple(int(v) for v in t) for t in (hidden_sizes, depths, num_attention_heads, sr_ratios, mlp_ratios)]
        if any(len(t) != 4 for t in cfg):
            raise NotImplementedError(f"four encoder stages are supported, got {cfg}")
        hidden, depths, heads, sr, mlp = cfg
        for C, h in zip(hidden, heads):
            if h < 1 or C != 64 * h:
                raise NotImplementedError(f"head dim {C}/{h}: the attention kernel has head dim 64 (hidden_sizes {hidden}, heads {heads}; "
                                          "MiT-B0 has 32 and is not supported)")
            if C > 2048:
                raise NotImplementedError(f"hidden size {C} exceeds 2048")
        if min(depths) < 1 or not all(1 <= s <= 16 for s in sr) or not all(1 <= m <= 8 for m in mlp):
            raise NotImplementedError(f"depths >= 1, sr_ratios 1 .. 16 and mlp_ratios 1 .. 8 are supported, got {depths}, {sr}, {mlp}")
        D, L = int(decoder_hidden_size), int(num_labels)
        if D < 4 or D % 4 or D > 2048:
            raise NotImplementedError(f"decoder_hidden_size must be a multiple of 4 up to 2048, got {D}")
        if not 1 <= L <= 256:
            raise NotImplementedError(f"num_labels must be 1 .. 256 (a label map is uint8), got {L}")
        if len(mean) != 3 or len(std) != 3 or min(std) <= 0:
            raise ValueError(f"mean and std must be three values, std positive, got {mean}, {std}")
        self.hidden_sizes, self.depths, self.num_attention_heads, self.sr_ratios, self.mlp_ratios = hidden, depths, heads, sr, mlp
        self.decoder_hidden_size, self.num_labels = D, L
        self.mean, self.std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
        stages = []
        for i in range(4):
            pe = _holder(proj=nn.Conv2d(3 if i == 0 else hidden[i - 1], hidden[i], 7 if i == 0 else 3, 4 if i == 0 else 2, 3 if i == 0 else 1),
                         layer_norm=nn.LayerNorm(hidden[i]))
            stages.append(_holder(patch_embeddings=pe, blocks=nn.ModuleList(_block(hidden[i], sr[i], hidden[i] * mlp[i]) for _ in range(depths[i])),
                                  layer_norm=nn.LayerNorm(hidden[i])))
        self.segformer = _holder(stages=nn.ModuleList(stages))
        self.decode_head = _holder(linear_projections=nn.ModuleList(_holder(proj=nn.Linear(hidden[i], D)) for i in range(4)),
                                   linear_fuse=nn.Conv2d(4 * D, D, 1, bias=False), batch_norm=nn.BatchNorm2d(D),
                                   classifier=nn.Conv2d(D, L, 1))
        self.eval()
        self._missing = None
        if seed is not None:
            self._seed(seed)
        elif weights is not None:
            if not os.path.exists(weights):
                raise FileNotFoundError(f"SegFormer weights not found at {weights}: pass weights= (a SegformerForSemanticSegmentation "
                                        "state dict saved with torch.save) or seed=; uspace_amd never downloads")
            self.load_state_dict(torch.load(weights, map_location="cpu"))
        else:
            self._missing = ("this SegFormer has no weights: pass weights= (a SegformerForSemanticSegmentation state dict saved with "
                             "torch.save), seed=, use SegFormer.from_hf, or call load_state_dict; uspace_amd never downloads")
        for p in self.parameters():
            p.requires_grad = False
        self._packed = PackedWeights("uspace_segformer_", f"SegFormer({hidden}, {depths})", self._canonical_params, cfg=self._c_cfg())
        self._ws = WorkspaceCache(2)

    @classmethod
    def from_hf(cls, model, mean=IMAGENET_MEAN, std=IMAGENET_STD):
        """From a ``transformers`` ``SegformerForSemanticSegmentation`` held in memory (nothing is fetched); its epsilons are taken
        over module by module."""
        c = model.config
        if c.num_encoder_blocks != 4 or c.num_channels != 3 or c.hidden_act != "gelu" or not c.reshape_last_stage:
            raise NotImplementedError("only num_encoder_blocks=4, num_channels=3, hidden_act='gelu', reshape_last_stage=True convert")
        if tuple(c.patch_sizes) != (7, 3, 3, 3) or tuple(c.strides) != (4, 2, 2, 2):
            raise NotImplementedError(f"patch_sizes {c.patch_sizes} / strides {c.strides}: only (7, 3, 3, 3) / (4, 2, 2, 2)")
        m = cls(c.hidden_sizes, c.depths, c.num_attention_heads, c.sr_ratios, c.mlp_ratios, c.decoder_hidden_size, c.num_labels, mean, std)
        m.load_state_dict({k: (v.detach().float() if v.is_floating_point() else v.detach().clone()) for k, v in model.state_dict().items()})
        mine = dict(m.named_modules())
        for name, mod in model.named_modules():
            if isinstance(mod, (nn.LayerNorm, nn.BatchNorm2d)):
                mine[name].eps = mod.eps
        return m

    @torch.no_grad()
    def _seed(self, seed):
        """The well-conditioned seeded weights of the module docstring."""
        g = torch.Generator().manual_seed(int(seed))
        for name, m in self.named_modules():
            if isinstance(m, (nn.Linear, nn.Conv2d)):
                k = 0.5 if name.endswith(("o_proj", "fc2")) else 1.0
                m.weight.copy_(k * torch.randn(m.weight.shape, generator=g) * (1.0 / m.weight[0].numel()) ** 0.5)
                if m.bias is not None:
                    m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
            elif isinstance(m, nn.LayerNorm):
                m.weight.copy_(0.8 + 0.4 * torch.rand(m.weight.shape, generator=g))
                m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
            elif isinstance(m, nn.BatchNorm2d):
                m.weight.copy_(0.7 + 0.6 * torch.rand(m.weight.shape, generator=g))
                m.bias.copy_(0.2 * torch.randn(m.bias.shape, generator=g))
                m.running_mean.copy_(0.2 * torch.randn(m.running_mean.shape, generator=g))
                m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, generator=g))

    def load_state_dict(self, state_dict, strict=True, assign=False):
        """Strict: a missing or unexpected key, or a wrong shape, raises (the model's keys, ``num_batches_tracked`` included)."""
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
    def _eps(self):
        """(embed, block, sr, stage, bn): each kind's epsilon, read from the modules; one kind must hold one value."""
        kinds = {"embed": set(), "block": set(), "sr": set(), "stage": set()}
        for name, m in self.named_modules():
            if isinstance(m, nn.LayerNorm):
                kind = ("embed" if "patch_embeddings" in name else "sr" if "sequence_reduction" in name else
                        "block" if "layernorm_" in name else "stage")
                kinds[kind].add(float(m.eps))
        kinds["sr"] = kinds["sr"] or kinds["block"]
        if any(len(v) != 1 for v in kinds.values()):
            raise NotImplementedError(f"the LayerNorms of one kind hold different epsilons: {kinds}")
        return tuple(next(iter(kinds[k])) for k in ("embed", "block", "sr", "stage")) + (float(self.decode_head.batch_norm.eps),)

    def _c_cfg(self):
        i4 = ctypes.c_int * 4
        return _hip.SegformerConfig(i4(*self.hidden_sizes), i4(*self.depths), i4(*self.num_attention_heads), i4(*self.sr_ratios),
                                    i4(*self.mlp_ratios), self.decoder_hidden_size, self.num_labels, *self._eps())

    def _canonical_params(self):
        return [v for k, v in self.state_dict().items() if not k.endswith("num_batches_tracked")]

    def _cfg(self):
        """The config struct the kernels get, with the epsilons the modules hold NOW: an epsilon set on a layer after construction
        is taken over here, and the blob (which holds the batch norm folded with its epsilon) is packed again."""
        eps = self._eps()
        c = self._packed.cfg
        if tuple(ctypes.c_float(e).value for e in eps) != (c.eps_embed, c.eps_block, c.eps_sr, c.eps_stage, c.eps_bn):
            self._packed.cfg = self._c_cfg()
            self._packed.invalidate()
        return self._packed.cfg

    def _blob(self, device):
        if self._missing:
            raise FileNotFoundError(self._missing)
        self._cfg()
        return self._packed.blob(device)

    def _workspace(self, B, H, W, device):
        nbytes = _hip.lib().uspace_segformer_workspace_bytes(ctypes.byref(self._cfg()), B, H, W)
        if nbytes == 0:
            keys = [(h // s) * (w // s) for (h, w), s in zip(stage_maps(H, W), self.sr_ratios)]
            raise NotImplementedError(f"SegFormer cannot take {B} images of {H} x {W} in one launch sequence: H and W must be 32 .. 16384 and "
                                      f"every reduced key map 1 .. 336 positions (here {keys}: the resident-key attention kernel); for "
                                      "many large images pass a smaller chunk=")
        return self._ws.take((B, H, W), device, nbytes)

    def stage_shapes(self, H, W):
        """[(h, w, c)] of the tap stages: per encoder stage its patch embedding, its blocks and its closing norm; then the
        concatenation, the fused map and the logits."""
        out = []
        for (h, w), C, n in zip(stage_maps(H, W), self.hidden_sizes, self.depths):
            out += [(h, w, C)] * (n + 2)
        h, w = stage_maps(H, W)[0]
        return out + [(h, w, 4 * self.decoder_hidden_size), (h, w, self.decoder_hidden_size), (h, w, self.num_labels)]

    @torch.no_grad()
    def preprocess(self, images):
        """images [B, 3, H, W] in [0, 1] on the device -> NHWC fp32 [B, H, W, 3], ``(x - mean_c) / std_c``
        (``uspace_resnet_preprocess``: the towers share the kernel)."""
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
    def logits_nhwc(self, images, chunk=8, ws_fill=None):
        """fp32 [B, H/4, W/4, L], the kernels' own layout; ``chunk`` images per launch sequence (an image's logits do not depend on
        it); ``ws_fill``: a byte the workspace is filled with first (a test aid: nothing of it is read before it is written)."""
        x = self.preprocess(images)
        B, H, W, _ = x.shape
        dev = x.device
        blob = self._blob(dev)
        chunk = max(1, min(int(chunk), B))
        ws = self._workspace(chunk, H, W, dev)
        if ws_fill is not None:
            ws.fill_(int(ws_fill))
        h, w = stage_maps(H, W)[0]
        out = torch.empty(B, h, w, self.num_labels, dtype=torch.float32, device=dev)
        L = _hip.lib()
        for lo in range(0, B, chunk):
            n = min(chunk, B - lo)
            _hip.check(L.uspace_segformer_forward(ctypes.byref(self._packed.cfg), _hip.ptr(blob), _hip.ptr(ws), ws.numel(),
                                                  _hip.ptr(x[lo:lo + n]), n, H, W, _hip.ptr(out[lo:lo + n]), _hip.stream_ptr()),
                       "uspace_segformer_forward")
        return out

    def logits(self, images, chunk=8):
        """fp32 [B, L, H/4, W/4] (the Hugging Face layout; a view of ``logits_nhwc``)."""
        return self.logits_nhwc(images, chunk).permute(0, 3, 1, 2)

    def forward(self, images, chunk=8):
        return self.logits(images, chunk)

    @torch.no_grad()
    def labels(self, images, chunk=8):
        """uint8 [B, H, W]: ``post_process_semantic_segmentation`` at the image's own size."""
        return _hip.seg_labels(self.logits_nhwc(images, chunk), images.shape[2:])

    @torch.no_grad()
    def tap(self, images, stage):
        """Test aid (``uspace_segformer_tap``): images as in ``logits`` -> tap stage ``stage`` (``stage_shapes``), NHWC fp32."""
        x = self.preprocess(images)
        B, H, W, _ = x.shape
        dev = x.device
        blob = self._blob(dev)
        shapes = self.stage_shapes(H, W)
        if not 0 <= int(stage) < len(shapes):
            raise ValueError(f"stage must be 0 .. {len(shapes) - 1}, got {stage}")
        out = torch.empty((B,) + shapes[stage], dtype=torch.float32, device=dev)
        ws = self._workspace(B, H, W, dev)
        _hip.check(_hip.lib().uspace_segformer_tap(ctypes.byref(self._packed.cfg), _hip.ptr(blob), _hip.ptr(ws), ws.numel(), _hip.ptr(x), B,
                                                   H, W, int(stage), _hip.ptr(out), _hip.stream_ptr()), "uspace_segformer_tap")
        return out


__all__ = ["SegFormer", "MIT_B1", "MIT_B2", "MIT_B3", "MIT_B4", "MIT_B5", "stage_maps"]
