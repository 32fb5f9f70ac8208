"""CLIP score on the MI355X: how well an image matches its prompt, ``100 * max(cos(e_image, e_text), 0)`` (Hessel et al. 2021, the
form torchmetrics' ``CLIPScore`` reports), with the embeddings of CLIP's two towers and projections computed in libuspace_hip.so:
``CLIPVisionTransformer`` (preprocessing included) for the images, the resident ``CLIPTextTransformer`` and
``CLIPTextProjection`` for the prompts, ``uspace_cosine_f32`` for the score.  Like ``FIDStatistics`` it takes decoded samples
straight from the sampler (``unpreprocess(vae.decode(z))``), quantised as ``save_image`` would, with no PNG round trip.

``directional_similarity`` is the editing metric (StyleGAN-NADA / InstructPix2Pix): the cosine between the step an edit makes in
image-embedding space and the step between the two prompts in text-embedding space.

Single process: a multi-rank run all-reduces ``score_sum`` and ``count`` itself."""
import torch

from uspace_amd import _hip
from uspace_amd.libs.clip import CLIPTextProjection, CLIPTextTransformer, CLIPVisionTransformer
from uspace_amd.tools._inputs import rocm_device


def _pair(a, b):
    _hip.require_device(a, "a")
    _hip.require_device(b, "b")
    a, b = a.detach().to(torch.float32).contiguous(), b.detach().to(torch.float32).contiguous()
    if a.dim() != 2 or a.shape != b.shape:
        raise ValueError(f"two [B, D] tensors expected, got {tuple(a.shape)} and {tuple(b.shape)}")
    return a, b


def cosine(a, b, scale=1.0, relu=False):
    """Row-wise ``scale * cos(a_b, b_b)`` of two fp32 [B, D] device tensors (``max(., 0)`` with ``relu``) -> [B]."""
    a, b = _pair(a, b)
    out = torch.empty(a.shape[0], dtype=torch.float32, device=a.device)
    if a.shape[0]:
        _hip.check(_hip.lib().uspace_cosine_f32(_hip.ptr(a), _hip.ptr(b), _hip.ptr(out), a.shape[0], a.shape[1], float(scale),
                                                1 if relu else 0, _hip.stream_ptr()), "uspace_cosine_f32")
    return out


def normalized_diff(a, b):
    """Row-wise ``a / |a| - b / |b|`` of two fp32 [B, D] device tensors."""
    a, b = _pair(a, b)
    out = torch.empty_like(a)
    if a.shape[0]:
        _hip.check(_hip.lib().uspace_normalized_diff_f32(_hip.ptr(a), _hip.ptr(b), _hip.ptr(out), a.shape[0], a.shape[1],
                                                         _hip.stream_ptr()), "uspace_normalized_diff_f32")
    return out


class CLIPScore:
    """Running CLIP score.  ``vision``: a CLIPVisionTransformer; ``text``: the CLIPTextTransformer the sampler already holds;
    ``text_projection``: a CLIPTextProjection; ``tokenizer``: the HF CLIPTokenizer (or anything called the same way)."""

    def __init__(self, vision, text, text_projection, tokenizer, device=None, max_length=77, eos_token_id=None):
        self.device = rocm_device(device, "the CLIP score")
        self.vision, self.text, self.text_projection = vision.to(self.device), text.to(self.device), text_projection.to(self.device)
        self.tokenizer = tokenizer
        self.max_length = max_length
        self.eos_token_id = eos_token_id
        self.reset()

    @classmethod
    def from_pretrained(cls, version="openai/clip-vit-large-patch14", device=None):
        """Both towers, the projections and the tokenizer from the HF files of ``version`` on disk (``local_files_only=True``:
        nothing is downloaded; a missing file raises what HF raises)."""
        from transformers import CLIPModel, CLIPTokenizer
        tokenizer = CLIPTokenizer.from_pretrained(version, local_files_only=True)
        hf = CLIPModel.from_pretrained(version, local_files_only=True)
        sd = hf.state_dict()
        tc = hf.config.text_config
        text = CLIPTextTransformer(tc.vocab_size, tc.hidden_size, tc.intermediate_size, tc.num_hidden_layers, tc.num_attention_heads,
                                   tc.max_position_embeddings, tc.layer_norm_eps, tc.hidden_act)
        text.load_state_dict(sd)
        proj = CLIPTextProjection(tc.hidden_size, hf.config.projection_dim)
        proj.load_state_dict(sd)
        return cls(CLIPVisionTransformer.from_hf(hf), text, proj, tokenizer, device, tc.max_position_embeddings, getattr(tc, "eos_token_id", None))

    def reset(self):
        self.score_sum = torch.zeros((), dtype=torch.float64, device=self.device)
        self.count = 0

    @torch.no_grad()
    def image_features(self, images, quantize=True):
        """images [B, 3, H, H] in [0, 1] on the device -> image_embeds [B, P] (not normalised)."""
        _hip.require_device(images, "images")
        return self.vision(self.vision.preprocess(images, quantize=quantize))

    @torch.no_grad()
    def text_features(self, prompts):
        """prompts (list of str) -> text_embeds [B, P] (not normalised); tokenised on the host, padded to ``max_length``."""
        if len(prompts) == 0:
            return torch.empty(0, self.text_projection.text_projection.weight.shape[0], dtype=torch.float32, device=self.device)
        enc = self.tokenizer(list(prompts), truncation=True, max_length=self.max_length, padding="max_length", return_tensors="pt")
        ids = enc["input_ids"].to(self.device)
        return self.text_projection(self.text(ids), ids, self.eos_token_id)

    @staticmethod
    def similarity(a, b):
        """The raw cosine of paired embeddings [B, P] -> [B]."""
        return cosine(a, b)

    @torch.no_grad()
    def update(self, images, prompts, quantize=True):
        """Add B (image, prompt) pairs; returns their scores ``100 * max(cos, 0)`` [B] (fp32, on the device)."""
        _hip.require_device(images, "images")
        if images.shape[0] != len(prompts):
            raise ValueError(f"{images.shape[0]} images for {len(prompts)} prompts")
        scores = cosine(self.image_features(images, quantize), self.text_features(prompts), scale=100.0, relu=True)
        self.score_sum += scores.double().sum()
        self.count += int(scores.numel())
        return scores

    def compute(self):
        """Mean score of everything added so far (a Python float)."""
        if self.count == 0:
            raise ValueError("CLIPScore.compute() before any update")
        return float(self.score_sum) / self.count

    @torch.no_grad()
    def directional_similarity(self, img_src, img_edit, prompt_src, prompt_edit, quantize=True):
        """cos(e_img_edit - e_img_src, e_txt_edit - e_txt_src) on normalised embeddings -> [B]."""
        d_img = normalized_diff(self.image_features(img_edit, quantize), self.image_features(img_src, quantize))
        d_txt = normalized_diff(self.text_features(prompt_edit), self.text_features(prompt_src))
        return cosine(d_img, d_txt)


__all__ = ["CLIPScore", "cosine", "normalized_diff"]
