"""DINO image towers on the gfx950 kernels of csrc/dino.hip: Hugging Face ``Dinov2Model`` in eval mode (``pooler_output``, hidden
states, the keys of a layer), and with ``layerscale=False`` the plain pre-LN ViT of HF ``ViTModel`` (DINO v1, ``facebook/dino-vitb8``).
The backbone of FD-DINOv2 and of the structure distance (``uspace_amd/tools/dino_metrics.py``).

Parameters carry the HF ``Dinov2Model`` names and order (``embeddings.cls_token``, ``embeddings.position_embeddings``,
``embeddings.patch_embeddings.projection.*``, ``encoder.layer.{i}.norm1 / attention.attention.{query,key,value} /
attention.output.dense / layer_scale1.lambda1 / norm2 / mlp.fc1 / mlp.fc2 / layer_scale2.lambda1``, ``layernorm``);
``embeddings.mask_token`` is dropped.  ``load_state_dict`` also takes a ``dinov2.`` / ``vit.`` prefix and HF ``ViTModel`` names
(``layernorm_before`` -> ``norm1``, ``layernorm_after`` -> ``norm2``, ``intermediate.dense`` -> ``mlp.fc1``, ``output.dense`` ->
``mlp.fc2``; ``pooler.*`` ignored), in the published files' spelling (``encoder.layer.{i}.attention.attention.query`` ...) and in
the one transformers 5 builds the model with (``layers.{i}.attention.q_proj`` ...).  The mapping is written from the installed ``transformers``' modules built from configs; it
has not been checked against any published weight file, none being available when this was written.

Position table: the module keeps the checkpoint's table (grid ``table_size / patch_size``); the table the kernels read is
interpolated to ``image_size / patch_size`` once, on the host, exactly as the installed transformers'
``Dinov2Embeddings.interpolate_pos_encoding`` does it (bicubic, ``align_corners=False``, output ``size=``), and packed with the
weights.  The original DINOv2 repository interpolates by ``scale_factor`` with ``interpolate_offset = 0.1``, which gives slightly
different tables; that form is not offered, and neither could be compared against features of the published weights.

Nothing is ever downloaded: weights come from ``weights=`` (a local state-dict file) or ``seed=``."""
import os

import torch
import torch.nn as nn

from .. import _hip
from ._tower import _ImageTower
from ._uvit_core import ParamGroup

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)

# table_size: the image side whose patch grid the checkpoint's position table covers (DINOv2 was trained at 518: 37 x 37)
DINOV2_L14 = dict(hidden_size=1024, num_attention_heads=16, num_hidden_layers=24, patch_size=14, image_size=224, table_size=518,
                  layerscale=True, layer_norm_eps=1e-6)                                     # facebook/dinov2-large
DINOV2_B14 = dict(DINOV2_L14, hidden_size=768, num_attention_heads=12, num_hidden_layers=12)   # facebook/dinov2-base
DINOV2_S14 = dict(DINOV2_L14, hidden_size=384, num_attention_heads=6, num_hidden_layers=12)    # facebook/dinov2-small
DINO_B8 = dict(hidden_size=768, num_attention_heads=12, num_hidden_layers=12, patch_size=8, image_size=224, table_size=224,
               layerscale=False, layer_norm_eps=1e-12)                                      # facebook/dino-vitb8 (HF ViTModel)

_VIT_TO_DINOV2 = (("layernorm_before.", "norm1."), ("layernorm_after.", "norm2."), ("intermediate.dense.", "mlp.fc1."))
# transformers 5 builds ViTModel with ``layers.{i}.attention.{q,k,v,o}_proj`` and ``mlp.fc1 / fc2``
_VIT5_TO_DINOV2 = ((".attention.q_proj.", ".attention.attention.query."), (".attention.k_proj.", ".attention.attention.key."),
                   (".attention.v_proj.", ".attention.attention.value."), (".attention.o_proj.", ".attention.output.dense."))


def map_state_dict_key(key):
    """The module's own key for a key of an HF ``Dinov2Model`` / ``ViTModel`` state dict (with or without its ``dinov2.`` /
    ``vit.`` prefix), or None for an entry the tower does not use (``mask_token``, ``pooler.*``, a classifier head)."""
    k = key
    for prefix in ("dinov2.", "vit."):
        if k.startswith(prefix):
            k = k[len(prefix):]
    if k.endswith("mask_token") or k.startswith(("pooler.", "classifier.")):
        return None
    if k.startswith("layers."):
        k = "encoder.layer." + k[len("layers."):]
    for old, new in _VIT_TO_DINOV2 + _VIT5_TO_DINOV2:
        k = k.replace(old, new)
    if ".output.dense." in k and ".attention.output.dense." not in k:       # ViTOutput, not ViTSelfOutput
        k = k.replace(".output.dense.", ".mlp.fc2.")
    return k


def interpolate_position_table(table, grid):
    """[1, n^2 + 1, D] -> [1, grid^2 + 1, D] fp32 on the host, as ``Dinov2Embeddings.interpolate_pos_encoding``: the class row is
    kept, the patch rows go through ``interpolate(size=(grid, grid), mode="bicubic", align_corners=False)`` in fp32; a table
    already at ``grid`` is returned as it is."""
    t = table.detach().to("cpu", torch.float32)
    n = int(round((t.shape[1] - 1) ** 0.5))
    if n * n != t.shape[1] - 1:
        raise ValueError(f"the position table has {t.shape[1] - 1} patch rows: not a square grid")
    if n == grid:
        return t
    D = t.shape[-1]
    patch = t[:, 1:].reshape(1, n, n, D).permute(0, 3, 1, 2)
    patch = nn.functional.interpolate(patch, size=(grid, grid), mode="bicubic", align_corners=False)
    return torch.cat((t[:, :1], patch.permute(0, 2, 3, 1).reshape(1, -1, D)), dim=1)


def _affine(group, name, *shape):
    c = group.child(name)
    c.add("weight", *shape)
    c.add("bias", shape[0])


class DinoVisionTransformer(_ImageTower):
    """HF ``Dinov2Model``'s computation in libuspace_hip.so (``uspace_dino_forward``).  ``image_size``: the side the tower runs
    at; ``table_size``: the side the checkpoint's position table was made for (default: ``image_size``)."""
    _SYMBOLS, _DISPLAY = "uspace_dino_", "DINO tower"

    def __init__(self, hidden_size=1024, num_attention_heads=16, num_hidden_layers=24, patch_size=14, image_size=224, table_size=None,
                 mlp_ratio=4, layerscale=True, layer_norm_eps=1e-6, hidden_act="gelu", use_swiglu_ffn=False, num_register_tokens=0,
                 num_channels=3, weights=None, seed=None, **_ignored):
        super().__init__()
        if use_swiglu_ffn:
            raise NotImplementedError("use_swiglu_ffn=True (DINOv2 ViT-g): the SwiGLU MLP is not supported, only the erf-GELU MLP")
        if num_register_tokens:
            raise NotImplementedError(f"num_register_tokens={num_register_tokens}: DINOv2 with registers is not supported")
        if hidden_act != "gelu":
            raise NotImplementedError(f"hidden_act={hidden_act!r}: the DINO towers use the exact (erf) gelu")
        if hidden_size != 64 * num_attention_heads or hidden_size % 64:
            raise NotImplementedError(f"head_dim must be 64: hidden_size {hidden_size} with {num_attention_heads} heads is not supported")
        ffn = int(hidden_size * mlp_ratio)
        if ffn % 64:
            raise NotImplementedError(f"the MLP width {ffn} must be a multiple of 64")
        table_size = image_size if table_size is None else table_size
        if num_channels != 3 or image_size % patch_size or table_size % patch_size:
            raise NotImplementedError(f"3 channels and image_size ({image_size}) / table_size ({table_size}) multiples of patch_size "
                                      f"({patch_size}) are required")
        self.cfg = dict(image=image_size, patch=patch_size, dim=hidden_size, heads=num_attention_heads, layers=num_hidden_layers,
                        ffn=ffn, layerscale=1 if layerscale else 0, eps=layer_norm_eps)
        self.grid = image_size // patch_size
        self.tokens = self.grid ** 2 + 1
        D = hidden_size
        emb = ParamGroup()
        emb.add("cls_token", 1, 1, D)
        emb.add("position_embeddings", 1, (table_size // patch_size) ** 2 + 1, D)
        _affine(emb.child("patch_embeddings"), "projection", D, 3, patch_size, patch_size)
        self.embeddings = emb
        layers = []
        for _ in range(num_hidden_layers):
            lyr = ParamGroup()
            _affine(lyr, "norm1", D)
            att = lyr.child("attention")
            inner = att.child("attention")
            for name in ("query", "key", "value"):
                _affine(inner, name, D, D)
            _affine(att.child("output"), "dense", D, D)
            if layerscale:
                lyr.child("layer_scale1").add("lambda1", D)
            _affine(lyr, "norm2", D)
            mlp = lyr.child("mlp")
            _affine(mlp, "fc1", ffn, D)
            _affine(mlp, "fc2", D, ffn)
            if layerscale:
                lyr.child("layer_scale2").add("lambda1", D)
            layers.append(lyr)
        self.encoder = ParamGroup()
        self.encoder.add_module("layer", nn.ModuleList(layers))
        self.layernorm = ParamGroup()
        self.layernorm.add("weight", D)
        self.layernorm.add("bias", D)
        if seed is not None:
            self._seed(seed)
        else:
            if weights is None or not os.path.exists(weights):
                raise FileNotFoundError(
                    f"DINO tower weights not found at {weights}: pass weights= (a state dict of HF Dinov2Model or ViTModel saved "
                    "with torch.save) or seed=; uspace_amd never downloads")
            self.load_state_dict(torch.load(weights, map_location="cpu"))
        self._pos = None           # ((data_ptr, version, device), interpolated table)
        self._finish_init()

    @torch.no_grad()
    def _seed(self, seed):
        """Seeded weights for tests and benchmarks: branches that move the residual stream, non-trivial norms, biases and
        LayerScale factors."""
        g = torch.Generator().manual_seed(int(seed))
        for name, p in self.named_parameters():
            r = torch.randn(p.shape, generator=g)
            if name.endswith("lambda1"):
                p.copy_(0.05 + 1.45 * torch.rand(p.shape, generator=g))
            elif "norm" in name and name.endswith("weight"):
                p.copy_(1.0 + 0.2 * r)
            elif name.endswith("bias"):
                p.copy_(0.1 * r)
            elif name.endswith(("cls_token", "position_embeddings")):
                p.copy_(0.3 * r)
            else:
                p.copy_(r / (p[0].numel() ** 0.5))

    def load_state_dict(self, state_dict, strict=True, assign=False):
        """Accepts HF ``Dinov2Model`` and ``ViTModel`` state dicts (see the module docstring); entries the tower does not use
        are dropped."""
        sd = {}
        for k, v in state_dict.items():
            own = map_state_dict_key(k)
            if own is not None:
                sd[own] = v
        return super().load_state_dict(sd, strict=strict, assign=assign)

    def invalidate_packed(self):
        """Forget the packed weight blob and the interpolated table; needed only after in-place edits through ``p.data``."""
        super().invalidate_packed()
        self._pos = None

    def position_table(self):
        """The table the kernels read: ``embeddings.position_embeddings`` interpolated to this tower's grid (fp32, on the
        parameters' device); recomputed when the parameter changed."""
        p = self.embeddings.position_embeddings
        key = (p.data_ptr(), p._version, str(p.device))
        if self._pos is None or self._pos[0] != key:
            self._pos = (key, interpolate_position_table(p, self.grid).to(p.device).contiguous())
        return self._pos[1]

    def _canonical_params(self):
        pos = self.embeddings.position_embeddings
        return [self.position_table() if p is pos else p for p in self.parameters()]

    def _c_cfg(self):
        c = self.cfg
        return _hip.DinoConfig(c["image"], c["patch"], c["dim"], c["heads"], c["layers"], c["ffn"], c["layerscale"], c["eps"])

    def preprocess(self, images, quantize=True, mean=IMAGENET_MEAN, std=IMAGENET_STD):
        """images [B, 3, H, H] fp32 in [0, 1] on the device -> pixel_values [B, 3, image_size, image_size]: ``save_image``'s
        rounding (``quantize``), antialiased bicubic resize (``uspace_clip_preprocess``), ImageNet mean and std."""
        return self._preprocess(images, quantize, mean, std)

    def _run(self, pixel_values, stop, key_layer, want_pooler):
        B = self._check_pixel_values(pixel_values)
        D = self.cfg["dim"]
        tap = self._out(pixel_values, self.tokens, D) if (stop != -1 and key_layer < 0) else None
        pooled = self._out(pixel_values, D) if want_pooler else None
        keys = self._out(pixel_values, self.tokens, D, dtype=torch.bfloat16) if key_layer >= 0 else None
        if B:
            L, lead = self._forward_args(B, pixel_values.device)
            pv = pixel_values.detach().to(torch.float32).contiguous()
            _hip.check(L.uspace_dino_forward(*lead, _hip.ptr(pv), _hip.ptr(pooled), B, stop, _hip.ptr(tap), key_layer, _hip.ptr(keys),
                                             _hip.stream_ptr()), "uspace_dino_forward")
        return pooled, tap, keys

    @torch.no_grad()
    def forward(self, pixel_values, hidden_state=None):
        """pixel_values [B, 3, S, S] -> ``pooler_output`` [B, D] fp32 (the final LayerNorm of the class token).
        ``hidden_state=k``: the residual stream [B, tokens, D] after k layers instead (HF ``hidden_states[k]``; 0 or
        "embeddings": the embeddings)."""
        stop = self._stop(hidden_state)
        pooled, tap, _ = self._run(pixel_values, stop, -1, stop == -1)
        return pooled if stop == -1 else tap

    @torch.no_grad()
    def keys(self, pixel_values, layer=-1):
        """The keys of one layer, ``LN1(x_l) Wk^T + bk`` with the heads concatenated: bf16 [B, tokens, D], as the tower's q|k|v
        GEMM stored them.  ``layer``: 0-based, negative from the end (-1: the last layer).  Only the layers up to it run."""
        n = self.cfg["layers"]
        l = int(layer) + n if int(layer) < 0 else int(layer)
        if not 0 <= l < n:
            raise ValueError(f"layer {layer} outside the tower's {n} layers")
        return self._run(pixel_values, l + 1, l, False)[2]


__all__ = ["DinoVisionTransformer", "DINOV2_L14", "DINOV2_B14", "DINOV2_S14", "DINO_B8", "IMAGENET_MEAN", "IMAGENET_STD",
           "map_state_dict_key", "interpolate_position_table"]
