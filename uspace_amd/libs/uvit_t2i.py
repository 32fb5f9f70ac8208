"""Drop-in for the reference's text-conditioned U-ViT (libs/uvit_t2i.py:192-342).

    nnet(x, timesteps, context=ctx, **kwargs) -> (pred, None)

77 CLIP context tokens are embedded by the HIP GEMM and prepended after the time token.
Classifier-free guidance (``cfg_scale=s, empty_context=...``: v_c + s (v_c - v_u), the configs'
``sample.scale``) runs both branches of every sample in one evaluation over 2B rows.
The prompt-to-prompt attention-map edit (dissect_name in {p2p, local_prompt,
sampled_image_editing}) is applied inside the fused attention kernel as a per-key factor.
The map itself -- the reference's ``vis_am_path`` pictures (tools/utils_t2i.py:141-193) and
``attention_maps`` -- comes from a kernel of its own (csrc/attention_map.hip): the fused kernel
never holds it.
"""
import numpy as np
import torch
import torch.nn as nn

from .. import _hip
from ..tools import utils_t2i
from ._uvit_core import ParamGroup, UViTBase, guidance_scales, host_timestep, timestep_digit


class UViT(UViTBase):
    def __init__(self, img_size=224, patch_size=16, in_chans=3, embed_dim=768, depth=12, num_heads=12,
                 mlp_ratio=4.0, qkv_bias=False, qk_scale=None, norm_layer=nn.LayerNorm, mlp_time_embed=False,
                 use_checkpoint=False, clip_dim=768, num_clip_token=77, conv=True, skip=True, use_latent1d=False):
        if qk_scale is not None:
            raise NotImplementedError("qk_scale override is not used by any reference config")
        if norm_layer is not nn.LayerNorm:
            raise NotImplementedError("only nn.LayerNorm")
        if clip_dim % 64:
            raise NotImplementedError("clip_dim must be a multiple of 64 (768 in every reference config)")
        self.clip_dim, self.num_clip_token = clip_dim, num_clip_token
        super().__init__(img_size=img_size, patch_size=patch_size, in_chans=in_chans, embed_dim=embed_dim,
                         depth=depth, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias,
                         mlp_time_embed=mlp_time_embed, conv=conv, skip=skip,
                         n_extra=num_clip_token, clip_dim=clip_dim, time_first=1)
        self.use_checkpoint = bool(use_checkpoint)    # no effect on sampling (no backward here); kept for compat/_training.py's twin

        def extras():
            self.context_embed = ParamGroup()
            self.context_embed.add("weight", embed_dim, clip_dim)
            self.context_embed.add("bias", embed_dim)

        self._build_tree(extras)
        self._reference_init_([(self.context_embed.weight, self.context_embed.bias,
                                lambda: nn.Linear(clip_dim, embed_dim))])
        self._ks_cache = None

    def _extra_canonical(self):
        return [self.context_embed.weight, self.context_embed.bias]

    def _prepare(self, x, timesteps, context, kwargs, paired=False):
        """What ``forward`` and ``attention_maps`` share: the checked fp32 context, this step's key_scale table (or None) and the
        timestep digit (None off the attention-edit path).  One place, so that a map always sees the edit ``forward`` applies.
        ``paired``: the table of a guided evaluation, [depth + 1, 2B, L] -- the edit on the conditional rows, ones on the
        unconditional ones (as in prompt-to-prompt, the edit acts on the conditional branch only)."""
        _hip.require_device(x, "x")
        B = x.shape[0]
        dev = x.device
        if context.dim() != 3 or context.shape[0] != B or context.shape[1] != self.num_clip_token \
                or context.shape[2] != self.clip_dim:
            raise ValueError(f"context must be [{B},{self.num_clip_token},{self.clip_dim}], got {tuple(context.shape)}")
        ctx = context.detach().to(device=dev, dtype=torch.float32).contiguous()   # libs/uvit_t2i.py:318
        key_scale = digit = None
        if utils_t2i.uses_attention_edit_path(kwargs):
            digit = timestep_digit(host_timestep(timesteps, kwargs))
            table = utils_t2i.key_scale_table(self.depth + 1, B, self.seq_len, digit, kwargs)
            if table is not None:
                if paired:
                    table = np.concatenate([table, np.ones_like(table)], axis=1)
                key_scale = self._device_table(table, dev)
        return ctx, key_scale, digit

    def _guidance(self, B, cfg_scale, empty_context):
        """The checked guidance arguments of ``forward``: (scale, per-sample scales or None, empty context, batched flag).  Host work
        only."""
        scale, rows = guidance_scales(cfg_scale, B)
        if empty_context is None:
            raise ValueError("cfg_scale needs empty_context: the context of the empty prompt (the feature datasets' empty_context.npy)")
        empty = torch.as_tensor(empty_context)
        want = (self.num_clip_token, self.clip_dim)
        if tuple(empty.shape) != want and tuple(empty.shape) != (B,) + want:
            raise ValueError(f"empty_context must be {list(want)} or {[B] + list(want)}, got {list(empty.shape)}")
        return scale, rows, empty, empty.dim() == 3

    def forward(self, x, timesteps, context, **kwargs):
        """kwargs: the reference's, and ``cfg_scale`` (None: no guidance; a number; or B per-sample values -- a guidance sweep in one
        solve) with ``empty_context`` ([77, clip_dim] or [B, 77, clip_dim]); ``maps_window=(q0, nq, k0, nk)`` (opt-in, what a paired
        local edit with an ``AttentionWordMask`` passes): return ``(pred, maps)`` with the head-mean attention maps
        [depth + 1, B, nq, nk] of this very evaluation, as ``attention_maps`` gives them."""
        window = kwargs.get("maps_window")
        if window is not None:
            if kwargs.get("cfg_scale") is not None or kwargs.get("vis_am_path") is not None:
                raise ValueError("maps_window is not available under cfg_scale or together with vis_am_path")
            ctx, key_scale, _ = self._prepare(x, timesteps, context, kwargs)
            return self._run(x, timesteps, context=ctx, key_scale=key_scale, attn_maps=tuple(int(v) for v in window))
        guide = None
        if kwargs.get("cfg_scale") is not None:
            guide = self._guidance(x.shape[0], kwargs["cfg_scale"], kwargs.get("empty_context"))
        ctx, key_scale, digit = self._prepare(x, timesteps, context, kwargs, paired=guide is not None)
        # tools/utils_t2i.py:279-283: on the edit path the decode direction shows the map (before the edit) when vis_am_path is set
        vis = digit in utils_t2i.VIS_DIGITS and kwargs.get("fm_direction") == "decode" and kwargs.get("vis_am_path") is not None
        if guide is not None:
            if vis:
                raise ValueError("vis_am_path pictures under cfg_scale are not supported: draw the maps in an unguided solve")
            scale, rows, empty, batched = guide
            empty = empty.detach().to(device=x.device, dtype=torch.float32).contiguous()
            cfg = (empty, batched, scale, self._guidance_rows(rows, x.device), False)
            return self._run(x, timesteps, context=ctx, key_scale=key_scale, cfg=cfg), None
        if not vis:
            return self._run(x, timesteps, context=ctx, key_scale=key_scale), None
        window = self.token_range("image") + self.token_range("context")
        out, maps = self._run(x, timesteps, context=ctx, key_scale=key_scale, attn_maps=window)
        kw = {k: v for k, v in kwargs.items() if k != "grid"}
        utils_t2i.vis_attention_map(maps, digit, grid=self.img_size // self.patch_size, **kw)
        return out, None

    def token_range(self, name):
        """(first token, count) of ``"image"``, ``"context"``, ``"time"`` or ``"all"`` in this network's token order: time (1),
        context (``num_clip_token``), image."""
        return utils_t2i.token_range(name, self.num_clip_token, self.num_patches)

    def attention_maps(self, x, timesteps, context, queries="image", keys="context", **kwargs):
        """Head-mean attention map of every block, [depth + 1, B, nq, nk] fp32 (block order: in-blocks, mid, out-blocks = the
        reference's ``_counter["block_id"]``): rows ``queries``, columns ``keys`` of the [L, L] softmax, each ``"image"``, ``"context"``,
        ``"time"``, ``"all"`` or an explicit ``(first, count)``.  The softmax runs over all L keys.  ``kwargs`` are those of
        ``forward``: a live p2p edit acts on the prediction and on the later blocks, the map of a block is always the one before its
        edit.  With ``queries="image", keys="image"`` this is the input of the reference's tools/attention_vis.py:54
        show_self_attention_comp.  Nothing is written, whatever ``vis_am_path`` says.  Maps under guidance (``cfg_scale``) are not
        available: ValueError."""
        if kwargs.get("cfg_scale") is not None:
            raise ValueError("attention_maps under cfg_scale is not supported: the maps of a guided evaluation are out of scope")
        ctx, key_scale, _ = self._prepare(x, timesteps, context, kwargs)
        window = self.token_range(queries) + self.token_range(keys)
        return self._run(x, timesteps, context=ctx, key_scale=key_scale, attn_maps=window)[1]

    def _device_table(self, table, dev):
        key = (table.shape, hash(table.tobytes()), str(dev))
        if self._ks_cache is None or self._ks_cache[0] != key:
            self._ks_cache = (key, torch.from_numpy(table).to(dev))
        return self._ks_cache[1]
