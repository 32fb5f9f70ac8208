"""Drop-in for the reference's text conditioning encoder (libs/clip.py:40-91 ``FrozenCLIPEmbedder``): prompts ->
``[B, 77, 768]`` context for ``uvit_t2i``.  The transformer (Hugging Face ``CLIPTextModel`` in the reference) runs in
libuspace_hip.so (``uspace_clip_text_forward``); the parameters carry the HF ``state_dict`` names, so
``load_state_dict(CLIPTextModel.from_pretrained(...).state_dict())`` (with or without the ``text_model.`` prefix)
works.  Tokenisation stays on the host with the HF tokenizer, exactly as the reference does it; the module is meant to
be created once and kept (the reference re-instantiates the encoder on every call, tools/utils_t2i.py:25-39).
SURVEY.md 8(f) rank 4.
"""
import numpy as np
import torch
import torch.nn as nn

from .. import _hip
from ._tower import _ImageTower, _Tower
from ._uvit_core import ParamGroup

CLIP_L_TEXT = dict(vocab_size=49408, hidden_size=768, intermediate_size=3072, num_hidden_layers=12,
                   num_attention_heads=12, max_position_embeddings=77, layer_norm_eps=1e-5)   # openai/clip-vit-large-patch14


def _word_piece_spans(words, pieces):
    """Half-open piece ranges ``[lo, hi)`` of every word: a word takes pieces until their characters cover its length
    (at least one piece, also for an empty word); words beyond the last piece get empty ranges."""
    spans, pos = [], 0
    for w in words:
        lo, covered = pos, 0
        while pos < len(pieces):
            covered += len(pieces[pos])
            pos += 1
            if covered >= len(w):
                break
        spans.append((lo, pos))
    return spans


def get_word_inds(text, word_place, tokenizer):
    """Token positions of the selected word(s) of ``text`` in the tokenizer's output, counted with ``<bos>`` at
    position 0 -- the indices the prompt-to-prompt hooks address in the ``[B, H, L, 77]`` cross-attention maps.
    ``word_place`` is a word (every occurrence counts), a word index, or a list of word indices.
    Same results as the reference's helper of this name (libs/clip.py:6-27), pinned by
    ``tests/golden/word_inds.json``; here the words are first mapped to ranges of word pieces."""
    words = text.split(" ")
    if isinstance(word_place, str):
        wanted = [k for k, w in enumerate(words) if w == word_place]
    elif isinstance(word_place, (int, np.integer)):
        wanted = [int(word_place)]
    else:
        wanted = [int(k) for k in word_place]
    if not wanted:
        return np.array([])
    ids = tokenizer.encode(text)[1:-1]                       # without <bos> / <eos>
    pieces = [tokenizer.decode([t]).strip("#") for t in ids]
    spans = _word_piece_spans(words, pieces)
    picked = sorted({p for k in wanted if 0 <= k < len(spans) for p in range(*spans[k])})
    return np.array([p + 1 for p in picked])


def _linear(group, name, nout, nin):
    c = group.child(name)
    c.add("weight", nout, nin)
    c.add("bias", nout)


def _norm(group, name, n):
    c = group.child(name)
    c.add("weight", n)
    c.add("bias", n)


def _encoder_layers(n, hidden_size, intermediate_size):
    """The ``ModuleList`` of ``n`` HF CLIPEncoderLayer parameter groups (the same in both towers), in state_dict order."""
    layers = []
    for _ in range(n):
        lyr = ParamGroup()
        att = lyr.child("self_attn")
        for name in ("k_proj", "v_proj", "q_proj", "out_proj"):
            _linear(att, name, hidden_size, hidden_size)
        _norm(lyr, "layer_norm1", hidden_size)
        mlp = lyr.child("mlp")
        _linear(mlp, "fc1", intermediate_size, hidden_size)
        _linear(mlp, "fc2", hidden_size, intermediate_size)
        _norm(lyr, "layer_norm2", hidden_size)
        layers.append(lyr)
    return nn.ModuleList(layers)


class _CLIPTower(_Tower):
    """What the two CLIP towers add to ``_Tower``: the checks of the encoder's shape and HF's initialisation.  A subclass also
    names itself for the messages (``_WHICH``); its constructor builds the parameters between ``super().__init__(...)`` and
    ``self._finish_init()``."""
    _WHICH = None

    def __init__(self, hidden_act, hidden_size, num_attention_heads, intermediate_size):
        super().__init__()
        if hidden_act != "quick_gelu":
            raise NotImplementedError(f"hidden_act={hidden_act!r}: {self._WHICH} uses quick_gelu")
        if hidden_size != 64 * num_attention_heads or hidden_size % 64 or intermediate_size % 64:
            raise NotImplementedError("head_dim must be 64 and the widths multiples of 64")

    def _finish_init(self):
        with torch.no_grad():                                  # HF _init_weights: normal tables / projections, unit norms
            for name, prm in self.named_parameters():
                if "norm" in name and name.endswith("weight"):
                    prm.fill_(1.0)
                elif name.endswith("bias"):
                    prm.zero_()
                else:
                    prm.normal_(0.0, 0.02)
        super()._finish_init()


class CLIPTextTransformer(_CLIPTower):
    """HF CLIPTextModel's computation given token ids; parameters in the HF state_dict order and naming."""
    _SYMBOLS, _DISPLAY, _WHICH = "uspace_clip_", "CLIP", "the CLIP text encoder the reference loads"

    def __init__(self, vocab_size=49408, hidden_size=768, intermediate_size=3072, num_hidden_layers=12,
                 num_attention_heads=12, max_position_embeddings=77, layer_norm_eps=1e-5, hidden_act="quick_gelu", **_ignored):
        super().__init__(hidden_act, hidden_size, num_attention_heads, intermediate_size)
        self.cfg = dict(vocab=vocab_size, dim=hidden_size, heads=num_attention_heads, layers=num_hidden_layers,
                        ffn=intermediate_size, max_pos=max_position_embeddings, eps=layer_norm_eps)
        emb = ParamGroup()
        emb.child("token_embedding").add("weight", vocab_size, hidden_size)
        emb.child("position_embedding").add("weight", max_position_embeddings, hidden_size)
        self.embeddings = emb
        enc = ParamGroup()
        enc.add_module("layers", _encoder_layers(num_hidden_layers, hidden_size, intermediate_size))
        self.encoder = enc
        self.final_layer_norm = ParamGroup()
        self.final_layer_norm.add("weight", hidden_size)
        self.final_layer_norm.add("bias", hidden_size)
        self._finish_init()

    def load_state_dict(self, state_dict, strict=True):
        """Accepts HF CLIPTextModel / CLIPModel checkpoints: an optional ``text_model.`` prefix is stripped,
        ``position_ids`` buffers and non-text entries are dropped."""
        sd = {}
        for k, v in state_dict.items():
            if k.startswith("text_model."):
                k = k[len("text_model."):]
            if k.startswith(("vision_model.", "visual_projection", "text_projection", "logit_scale")) or k.endswith("position_ids"):
                continue
            sd[k] = v
        return super().load_state_dict(sd, strict=strict)

    def _c_cfg(self):
        c = self.cfg
        return _hip.ClipConfig(c["vocab"], c["dim"], c["heads"], c["layers"], c["ffn"], c["max_pos"], c["eps"])

    def forward(self, input_ids, hidden_state=None):
        """input_ids [B, L<=max_pos] integer tensor -> last_hidden_state [B, L, D] fp32 (``hidden_state=k``: the state
        after k layers, HF ``output_hidden_states[k]``)."""
        _hip.require_device(input_ids, "input_ids")
        if input_ids.dim() != 2 or input_ids.shape[1] > self.cfg["max_pos"]:
            raise ValueError(f"input_ids must be [B, L<={self.cfg['max_pos']}], got {tuple(input_ids.shape)}")
        if input_ids.numel() and (int(input_ids.min()) < 0 or int(input_ids.max()) >= self.cfg["vocab"]):
            raise IndexError("token id out of range")            # nn.Embedding raises IndexError as well
        dev = input_ids.device
        if input_ids.shape[0] == 0 or input_ids.shape[1] == 0:
            return torch.empty(input_ids.shape[0], input_ids.shape[1], self.cfg["dim"], dtype=torch.float32, device=dev)
        B, T = input_ids.shape
        L, lead = self._forward_args(B, dev)
        ids = input_ids.to(torch.int32).contiguous()
        out = torch.empty(B, T, self.cfg["dim"], dtype=torch.float32, device=dev)
        _hip.check(L.uspace_clip_text_forward(*lead, _hip.ptr(ids), _hip.ptr(out), B, T,
                                              -1 if hidden_state is None else int(hidden_state), _hip.stream_ptr()),
                   "uspace_clip_text_forward")
        return out


CLIP_L_VISION = dict(hidden_size=1024, intermediate_size=4096, num_hidden_layers=24, num_attention_heads=16, image_size=224,
                     patch_size=14, projection_dim=768, layer_norm_eps=1e-5)                  # openai/clip-vit-large-patch14
CLIP_L_336_VISION = dict(CLIP_L_VISION, image_size=336)       # openai/clip-vit-large-patch14-336: 577 tokens (CMMD's tower)
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)                                               # HF OPENAI_CLIP_MEAN / _STD
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


class CLIPVisionTransformer(_CLIPTower, _ImageTower):
    """HF CLIPVisionModelWithProjection's computation (``image_embeds``) in libuspace_hip.so (``uspace_clipv_forward``), with the
    image preprocessing of ``uspace_clip_preprocess`` in front of it; parameters in the HF state_dict order and naming
    (``vision_model.*``, ``visual_projection.weight``)."""
    _SYMBOLS, _DISPLAY, _WHICH = "uspace_clipv_", "CLIP vision", "the CLIP vision tower of openai/clip-vit-large-patch14"

    def __init__(self, hidden_size=1024, intermediate_size=4096, num_hidden_layers=24, num_attention_heads=16, image_size=224,
                 patch_size=14, projection_dim=768, layer_norm_eps=1e-5, hidden_act="quick_gelu", num_channels=3, **_ignored):
        super().__init__(hidden_act, hidden_size, num_attention_heads, intermediate_size)
        if num_channels != 3 or image_size % patch_size or projection_dim % 4:
            raise NotImplementedError("3 channels, image_size a multiple of patch_size and projection_dim a multiple of 4")
        self.cfg = dict(image=image_size, patch=patch_size, dim=hidden_size, heads=num_attention_heads, layers=num_hidden_layers,
                        ffn=intermediate_size, proj_dim=projection_dim, eps=layer_norm_eps)
        self.tokens = (image_size // patch_size) ** 2 + 1
        vm = ParamGroup()
        emb = vm.child("embeddings")
        emb.add("class_embedding", hidden_size)
        emb.child("patch_embedding").add("weight", hidden_size, 3, patch_size, patch_size)
        emb.child("position_embedding").add("weight", self.tokens, hidden_size)
        _norm(vm, "pre_layrnorm", hidden_size)                 # HF's spelling
        vm.child("encoder").add_module("layers", _encoder_layers(num_hidden_layers, hidden_size, intermediate_size))
        _norm(vm, "post_layernorm", hidden_size)
        self.vision_model = vm
        self.visual_projection = ParamGroup()
        self.visual_projection.add("weight", projection_dim, hidden_size)
        self._finish_init()

    @classmethod
    def from_hf(cls, hf):
        """The vision tower and projection of an HF ``CLIPModel``, built from its config with its weights loaded."""
        vc = hf.config.vision_config
        vision = cls(vc.hidden_size, vc.intermediate_size, vc.num_hidden_layers, vc.num_attention_heads, vc.image_size,
                     vc.patch_size, hf.config.projection_dim, vc.layer_norm_eps, vc.hidden_act)
        vision.load_state_dict(hf.state_dict())
        return vision

    def load_state_dict(self, state_dict, strict=True):
        """Accepts HF CLIPModel / CLIPVisionModel / CLIPVisionModelWithProjection checkpoints, with or without the
        ``vision_model.`` prefix; ``position_ids`` buffers and text entries are dropped."""
        sd = {}
        for k, v in state_dict.items():
            if k.startswith(("text_model.", "text_projection", "logit_scale")) or k.endswith("position_ids"):
                continue
            if not k.startswith(("vision_model.", "visual_projection")):
                k = "vision_model." + k
            sd[k] = v
        return super().load_state_dict(sd, strict=strict)

    def _c_cfg(self):
        c = self.cfg
        return _hip.ClipVisionConfig(c["image"], c["patch"], c["dim"], c["heads"], c["layers"], c["ffn"], c["proj_dim"], c["eps"])

    def preprocess(self, images, quantize=True, mean=CLIP_MEAN, std=CLIP_STD):
        """images [B, 3, H, H] fp32 in [0, 1] on the device -> pixel_values [B, 3, image_size, image_size]: ``save_image``'s
        rounding (``quantize``), antialiased bicubic resize (``uspace_clip_preprocess``), CLIP's mean and std."""
        return self._preprocess(images, quantize, mean, std)

    def forward(self, pixel_values, hidden_state=None, return_pooled=False):
        """pixel_values [B, 3, S, S] -> image_embeds [B, projection_dim] fp32 (``return_pooled``: also HF's ``pooler_output``
        [B, D]).  ``hidden_state=k``: the state [B, tokens, D] after k layers instead (k = 0: after pre_layrnorm, HF
        ``hidden_states[k]``; "embeddings": before pre_layrnorm)."""
        B = self._check_pixel_values(pixel_values)
        D, P = self.cfg["dim"], self.cfg["proj_dim"]
        stop = self._stop(hidden_state)
        tap = self._out(pixel_values, self.tokens, D) if stop != -1 else None
        emb = self._out(pixel_values, P) if stop == -1 else None
        pooled = self._out(pixel_values, D) if (return_pooled and stop == -1) else None
        if B:
            L, lead = self._forward_args(B, pixel_values.device)
            pv = pixel_values.detach().to(torch.float32).contiguous()
            _hip.check(L.uspace_clipv_forward(*lead, _hip.ptr(pv), _hip.ptr(emb), _hip.ptr(pooled), B, stop, _hip.ptr(tap),
                                              _hip.stream_ptr()), "uspace_clipv_forward")
        if stop != -1:
            return tap
        return (emb, pooled) if return_pooled else emb


class CLIPTextProjection(nn.Module):
    """HF CLIPModel's text head: the pooled row of ``last_hidden_state`` through ``text_projection`` (no bias), in fp32
    (``uspace_gather_rows_f32``, ``uspace_linear_f32``)."""

    def __init__(self, hidden_size=768, projection_dim=768):
        super().__init__()
        if hidden_size % 4:
            raise NotImplementedError("hidden_size must be a multiple of 4")
        self.text_projection = ParamGroup()
        self.text_projection.add("weight", projection_dim, hidden_size)
        with torch.no_grad():
            self.text_projection.weight.normal_(0.0, hidden_size ** -0.5)
        self.eval()
        self.requires_grad_(False)

    def load_state_dict(self, state_dict, strict=True):
        """Accepts a CLIPModel / CLIPTextModelWithProjection checkpoint: only ``text_projection.weight`` is taken."""
        return super().load_state_dict({k: v for k, v in state_dict.items() if k == "text_projection.weight"}, strict=strict)

    @staticmethod
    def pooled_index(input_ids, eos_token_id=None):
        """HF's rule: ``eos_token_id`` 2 or None (the legacy config of this checkpoint family) -> ``argmax`` of the ids (the
        end-of-text token has the largest id); otherwise the first position that holds ``eos_token_id``."""
        if eos_token_id is None or eos_token_id == 2:
            return input_ids.argmax(-1)
        return (input_ids == eos_token_id).int().argmax(-1)

    def forward(self, last_hidden_state, input_ids, eos_token_id=None):
        """last_hidden_state [B, L, D] fp32 (device), input_ids [B, L] -> text_embeds [B, projection_dim] fp32."""
        _hip.require_device(last_hidden_state, "last_hidden_state")
        h = last_hidden_state.detach().to(torch.float32).contiguous()
        if h.dim() != 3 or tuple(input_ids.shape) != tuple(h.shape[:2]):
            raise ValueError(f"last_hidden_state [B, L, D] and input_ids [B, L] expected, got {tuple(h.shape)} and {tuple(input_ids.shape)}")
        B, T, D = h.shape
        w = self.text_projection.weight
        _hip.require_device(w, "text_projection.weight")
        if D != w.shape[1]:
            raise ValueError(f"hidden size {D} does not match text_projection {tuple(w.shape)}")
        out = torch.empty(B, w.shape[0], dtype=torch.float32, device=h.device)
        if B == 0:
            return out
        idx = self.pooled_index(input_ids, eos_token_id).to(device=h.device, dtype=torch.int32).contiguous()
        pooled = torch.empty(B, D, dtype=torch.float32, device=h.device)
        L = _hip.lib()
        _hip.check(L.uspace_gather_rows_f32(_hip.ptr(h), _hip.ptr(idx), _hip.ptr(pooled), B, T, D, _hip.stream_ptr()),
                   "uspace_gather_rows_f32")
        wf = w.detach().to(torch.float32).contiguous()
        _hip.check(L.uspace_linear_f32(_hip.ptr(pooled), _hip.ptr(wf), _hip.ptr(out), B, w.shape[0], D, _hip.stream_ptr()),
                   "uspace_linear_f32")
        return out


class AbstractEncoder(nn.Module):
    def encode(self, *args, **kwargs):
        raise NotImplementedError


class FrozenCLIPEmbedder(AbstractEncoder):
    """``FrozenCLIPEmbedder(version, device, max_length)`` as in libs/clip.py:40-91.  ``tokenizer`` / ``transformer`` may
    be passed in (offline use, tests); otherwise they are loaded with ``from_pretrained(version)`` like the reference
    (which needs the HF files on disk)."""

    def __init__(self, version="openai/clip-vit-large-patch14", device="cuda", max_length=77, tokenizer=None,
                 transformer=None):
        super().__init__()
        if tokenizer is None:
            from transformers import CLIPTokenizer
            tokenizer = CLIPTokenizer.from_pretrained(version)
        if transformer is None:
            from transformers import CLIPTextModel
            hf = CLIPTextModel.from_pretrained(version)
            c = hf.config
            transformer = CLIPTextTransformer(c.vocab_size, c.hidden_size, c.intermediate_size, c.num_hidden_layers,
                                              c.num_attention_heads, c.max_position_embeddings, c.layer_norm_eps, c.hidden_act)
            transformer.load_state_dict(hf.state_dict())
        self.tokenizer = tokenizer
        self.transformer = transformer
        self.device = device
        self.max_length = max_length
        self.freeze()

    def freeze(self):
        self.transformer = self.transformer.eval()
        for p in self.parameters():
            p.requires_grad = False

    def get_word_inds(self, text, word_place):
        return get_word_inds(text=text, word_place=word_place, tokenizer=self.tokenizer)

    def forward(self, text):
        enc = self.tokenizer(text, truncation=True, max_length=self.max_length, return_length=True,
                             return_overflowing_tokens=False, padding="max_length", return_tensors="pt")
        tokens = enc["input_ids"].to(self.device)
        return self.transformer(tokens)

    def encode(self, text):
        return self(text)
