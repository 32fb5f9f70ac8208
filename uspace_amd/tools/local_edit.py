"""Local edits: keep the outside of a region fixed while an edit acts inside it.

Every edit of this package -- the u-space write (``write_attr`` / ``write_pca``), the p2p column rescale, a replaced prompt -- acts
on every latent position.  ``CNF.decode_local`` (flow_matching.py / flow_matching_t2i.py) runs the source and the edited branch of
every sample in one solve over 2B rows and replaces the edited branch's *velocity* by the source's wherever a mask is 0
(``uspace_pair_blend``); with both branches started from the same noise the edited latents outside the mask are then bit-equal
to the source's under every solver.  This file makes the masks:

* ``LabelRegionMask(tower, region, dilate=1, threshold=0.0, soft=False).of(images, S)`` -- from a parser (``libs.segformer.SegFormer``
  or ``tools.seg_metrics.LogitsParser``): per latent cell the share of pixels whose label is in ``region``, the maximum of the
  shares over the (2 dilate + 1)^2 cells around it (clipped at the border), then ``share > threshold`` (``soft``: the share itself).
  ``uspace_mask_from_labels``; integer counts and one fp32 division, exact.
* ``AttentionWordMask(words | token_ids=, blocks="all", threshold=0.3, from_t=0.2)`` -- text-to-image only, after prompt-to-prompt's
  LocalBlend: at every evaluation, from that evaluation's own head-mean image x word attention maps, the chosen words' token
  columns summed over the chosen blocks, 3 x 3 max-pooled over the token grid, divided by the sample's maximum, thresholded, spread
  over the patch's latent cells (``uspace_mask_from_maps``); the source rows' mask (the source caption's columns) and the edited
  rows' mask (the edited caption's) are united with a maximum.  Stateless: nothing is carried from one evaluation to the next, so
  the rejected attempts of an adaptive solve leave no trace.  Before ``from_t`` the mask is all ones (the layout forms first).
* ``edit_region(cnf, vae, z, cond, region_mask, **kwargs)`` -- plain decode, ``vae.decode``, the parser's mask of that source
  image, ``decode_local``.

These definitions are this project's own (INTEGRATION.md §A "Local edits"); the attention mask follows LocalBlend as remembered
and is unverified against that code."""
import numpy as np
import torch

from uspace_amd import _hip
from uspace_amd.tools import utils_t2i

MAX_MAP_TOKENS = 336       # the map kernel's limit (uspace_attention_map_bf16)


class LabelRegionMask:
    """``region``: the label ids of the part the edit may change.  ``of(images, S)`` -> a copy bound to ``images`` ([B, 3, H, W] in
    [0, 1] on the device; H and W multiples of the latent side ``S``) whose ``mask`` is fp32 [B, S, S]."""

    def __init__(self, tower, region, dilate=1, threshold=0.0, soft=False):
        n = int(tower.num_labels)
        ids = sorted({int(r) for r in region})
        if not ids or not all(0 <= r < n for r in ids):
            raise ValueError(f"region must hold label ids from 0 to {n - 1}, got {ids}")
        if isinstance(dilate, bool) or int(dilate) != dilate or not 0 <= int(dilate) <= 4:
            raise ValueError(f"dilate must be an integer from 0 to 4, got {dilate!r}")
        self.tower, self.region, self.dilate, self.threshold, self.soft = tower, ids, int(dilate), float(threshold), bool(soft)
        member = np.zeros(256, dtype=np.uint8)
        member[ids] = 1
        self._member = torch.from_numpy(member)
        self.mask = self.labels = None

    @torch.no_grad()
    def of(self, images, S):
        _hip.require_device(images, "images")
        S = int(S)
        if images.dim() != 4 or images.shape[2] % S or images.shape[3] % S:
            raise ValueError(f"expected images [B, 3, H, W] with H and W multiples of the latent side {S}, got {tuple(images.shape)}")
        bound = LabelRegionMask(self.tower, self.region, self.dilate, self.threshold, self.soft)
        bound.labels = self.tower.labels(images)
        bound.mask = _hip.mask_from_labels(bound.labels.contiguous(), self._member.to(images.device), S, self.dilate, self.threshold,
                                           self.soft)
        return bound


def _columns(ids, B, nk, what):
    """fp32 [B, nk], 1 on every sample's token columns; ``ids``: one index array for all samples or B of them."""
    if ids is None:
        raise ValueError(f"the {what} token columns are not set: give token_ids=, or words= and call for_captions")
    if len(ids) == 0 or np.ndim(ids[0]) == 0:
        ids = [ids] * B
    if len(ids) != B:
        raise ValueError(f"{what} token_ids holds {len(ids)} lists for a batch of {B}")
    cols = np.zeros((B, nk), np.float32)
    for b, tid in enumerate(ids):
        tid = np.asarray(tid).astype(np.int64).reshape(-1)
        if tid.size and (tid.min() < 0 or tid.max() >= nk):
            raise ValueError(f"{what} token ids of sample {b} lie outside the {nk} context tokens: {tid.tolist()}")
        cols[b, tid] = 1.0
    return cols


class AttentionWordMask:
    """``words``: a word (or word index, as ``FrozenCLIPEmbedder.get_word_inds`` takes it), or a ``(source, edited)`` pair where the
    two captions differ in it; ``for_captions(embedder, source_captions, edited_captions)`` turns them into token columns.  Or
    ``token_ids=(source, edited)`` directly: per branch one index array for all samples, or one per sample (positions among the
    context tokens, ``<bos>`` at 0).  ``blocks``: ``"all"``, a block id or a list of them (in-blocks, mid, out-blocks).
    ``record``: a list that receives ``(t, mask [B, S, S])`` of every evaluation (a test aid; the mask itself keeps no state)."""

    def __init__(self, words=None, token_ids=None, blocks="all", threshold=0.3, from_t=0.2, record=None):
        if (words is None) == (token_ids is None):
            raise ValueError("give exactly one of words= and token_ids=")
        self.words = words
        self.src_ids = self.edit_ids = None
        if token_ids is not None:
            if not isinstance(token_ids, (tuple, list)) or len(token_ids) != 2:
                raise ValueError("token_ids must be a (source, edited) pair")
            self.src_ids, self.edit_ids = token_ids
        self.blocks, self.threshold, self.from_t, self.record = blocks, float(threshold), float(from_t), record
        self._dev = None

    def for_captions(self, embedder, source_captions, edited_captions):
        if self.words is None:
            raise ValueError("for_captions needs words=")
        ws, we = self.words if isinstance(self.words, (tuple, list)) and len(self.words) == 2 else (self.words, self.words)
        self.src_ids = [np.asarray(embedder.get_word_inds(c, ws)) for c in source_captions]
        self.edit_ids = [np.asarray(embedder.get_word_inds(c, we)) for c in edited_captions]
        self._dev = None
        return self

    # -- what CNFBase._decode_local calls
    def check(self, net, B):
        if not hasattr(net, "num_clip_token"):
            raise ValueError("an AttentionWordMask needs a text-to-image network: this one has no context tokens")
        if net.seq_len > MAX_MAP_TOKENS:
            raise ValueError(f"attention maps are available up to {MAX_MAP_TOKENS} tokens, this network has {net.seq_len}")
        self._operands(net, B, None)

    def window(self, net):
        return net.token_range("image") + net.token_range("context")

    def all_ones_at(self, t):
        return float(t) < self.from_t

    def _operands(self, net, B, dev):
        key = (B, net.depth, net.num_clip_token, str(dev))
        if self._dev is None or self._dev[0] != key:
            nk = net.num_clip_token
            cols = np.concatenate([_columns(self.src_ids, B, nk, "source"), _columns(self.edit_ids, B, nk, "edited")])
            w = np.array([1.0 if utils_t2i.block_selected(self.blocks, i) else 0.0 for i in range(net.depth + 1)], np.float32)
            if dev is None:
                return None
            self._dev = (key, torch.from_numpy(w).to(dev), torch.from_numpy(cols).to(dev))
        return self._dev[1], self._dev[2]

    def from_maps(self, net, maps, t=None):
        """maps [depth + 1, 2B, G * G, nk] of one evaluation over the 2B rows -> the united mask fp32 [B, S * S]."""
        B = maps.shape[1] // 2
        w, cols = self._operands(net, B, maps.device)
        G = net.img_size // net.patch_size
        both = _hip.mask_from_maps(maps, w, cols, G, net.patch_size, self.threshold, False)
        m = torch.maximum(both[:B], both[B:]).reshape(B, -1)
        if self.record is not None:
            self.record.append((t, m.reshape(B, net.img_size, net.img_size).clone()))
        return m


def edit_region(cnf, vae, z, cond, region_mask, source=None, **kwargs):
    """The whole flow for a parser's mask: a plain decode of ``z`` (the solver keywords of ``kwargs``, no edit; under the source's
    condition where ``source`` gives one), ``vae.decode``, ``region_mask.of`` that source image, then ``cnf.decode_local`` with the
    edit of ``kwargs`` -> (edited latents, source latents, mask [B, S, S]).  ``cond``: ``y`` or the context, as the driver takes
    it."""
    from uspace_amd import flow_matching_t2i
    t2i = isinstance(cnf, flow_matching_t2i.CNF)
    plain = {k: kwargs[k] for k in ("solver_kwargs", "t_edit") if k in kwargs}
    plain.update(dissect_name="none", edit_loc=None)
    src_cond = (source or {}).get("context" if t2i else "y", cond)
    first = cnf.decode(z, context=src_cond, **plain) if t2i else cnf.decode(z, src_cond, **plain)
    images = vae.decode(first).to(torch.float32).mul_(0.5).add_(0.5).clamp_(0.0, 1.0)
    bound = region_mask.of(images, z.shape[-1])
    if t2i:
        edited, src = cnf.decode_local(z, context=cond, mask=bound, source=source, **kwargs)
    else:
        edited, src = cnf.decode_local(z, cond, mask=bound, source=source, **kwargs)
    return edited, src, bound.mask
