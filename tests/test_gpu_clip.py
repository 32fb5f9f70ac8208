"""CLIP text encoder on the GPU: FrozenCLIPEmbedder's transformer (libs/clip.py:40-91 = HF
CLIPTextModel(input_ids).last_hidden_state) through the C-ABI, against the HF module's own outputs (tiny random-init
fixture) and the CPU oracle; the causal attention / quick-GELU / table-embedding entry points against the oracle."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import clip_oracle as K
from tests.util import rel_l2, to_dev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from uspace_amd import _hip
    _hip.lib()
    return _hip


def _tiny(golden_dir):
    from uspace_amd.libs.clip import CLIPTextTransformer
    z = np.load(os.path.join(golden_dir, "clip_text_tiny.npz"))
    meta = json.loads(bytes(z["meta_json"]).decode())
    m = CLIPTextTransformer(**{k: meta[k] for k in ("vocab_size", "hidden_size", "intermediate_size", "num_hidden_layers",
                                                    "num_attention_heads", "max_position_embeddings", "layer_norm_eps",
                                                    "hidden_act")})
    m.load_state_dict({"text_model." + k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd/")})
    return z, meta, m.cuda()


def test_tiny_text_transformer_matches_hf_golden(golden_dir):
    z, meta, m = _tiny(golden_dir)
    ids = torch.from_numpy(z["ids"]).cuda()
    out = m(ids)
    assert out.shape == (3, 77, 128) and out.dtype == torch.float32
    assert rel_l2(out.cpu().numpy(), z["out"]) < 6e-3            # bf16 GEMM / attention operands, fp32 residual stream
    for k in range(meta["num_hidden_layers"] + 1):
        h = m(ids, hidden_state=k).cpu().numpy()
        assert rel_l2(h, z[f"hidden/{k}"]) < (1e-6 if k == 0 else 6e-3), k
    assert torch.equal(m(ids), out)                               # deterministic
    # shorter prompts (L < 77) and one row at a time give the same rows (causal: a prefix does not see its suffix)
    # (bit-equal: every GEMM form walks K in the same order and splits none, the row kernels work per row and masked keys get P = 0
    # exactly -- tests/test_gpu_clip_parity.py checks this at the CLIP-L shape)
    assert torch.equal(m(ids[:, :33].contiguous()), out[:, :33])
    assert torch.equal(m(ids[1:2].contiguous()), out[1:2])
    with pytest.raises(IndexError):
        m(torch.full((1, 5), 1000, device="cuda"))
    with pytest.raises(ValueError):
        m(torch.zeros(1, 78, dtype=torch.long, device="cuda"))


@pytest.mark.parametrize("B,L,H", [(2, 77, 2), (3, 33, 12), (1, 129, 1)])
def test_causal_attention_matches_oracle(hip, B, L, H):
    rng = np.random.default_rng(L + H)
    D = 64 * H
    qkv = (rng.standard_normal((B, L, 3 * D)) * 0.8).astype(np.float32)
    qb = torch.from_numpy(qkv).to("cuda", dtype=torch.bfloat16)
    q32 = qb.float().cpu().numpy()
    ref = K.causal_attention(q32[..., :D], q32[..., D:2 * D], q32[..., 2 * D:], H)
    out = torch.empty(B, L, D, dtype=torch.bfloat16, device="cuda")
    rc = hip.lib().uspace_attention_causal_bf16(hip.ptr(qb), hip.ptr(out), B, L, H, hip.stream_ptr())
    assert rc == 0
    got = out.float().cpu().numpy()
    assert rel_l2(got, ref) < 8e-3
    assert torch.equal(out[:, 0], qb[:, 0, 2 * D:])                # the first token attends only to itself: P = 1, out = v_0 exactly
    assert hip.lib().uspace_attention_causal_bf16(hip.ptr(qb), hip.ptr(out), B, 161, H, hip.stream_ptr()) != 0


def test_table_embed_quick_gelu_and_f32_layernorm(hip):
    import ctypes
    from oracle import _cops as C
    rng = np.random.default_rng(3)
    B, L, D, V = 3, 20, 128, 50
    tok, pos = rng.standard_normal((V, D)).astype(np.float32), rng.standard_normal((L, D)).astype(np.float32)
    ids = rng.integers(0, V, (B, L)).astype(np.int32)
    out = torch.empty(B, L, D, device="cuda")
    t_, p_, i_ = to_dev(tok), to_dev(pos), torch.from_numpy(ids).cuda()
    assert hip.lib().uspace_table_embed(hip.ptr(i_), hip.ptr(t_), hip.ptr(p_), hip.ptr(out), B, L, D, V, hip.stream_ptr()) == 0
    assert np.array_equal(out.cpu().numpy(), tok[ids] + pos[None])
    x = (rng.standard_normal(4096) * 3).astype(np.float32)
    xb = torch.from_numpy(x).to("cuda", dtype=torch.bfloat16)
    ref = K.quick_gelu(xb.float().cpu().numpy())
    assert hip.lib().uspace_quick_gelu_bf16(hip.ptr(xb), 4096, hip.stream_ptr()) == 0
    assert np.abs(xb.float().cpu().numpy() - ref).max() <= 2.0 ** -8 * np.abs(ref).max()
    xs = (rng.standard_normal((37, 768)) * 2 + 0.5).astype(np.float32)
    g, b = rng.standard_normal(768).astype(np.float32), rng.standard_normal(768).astype(np.float32)
    y = torch.empty(37, 768, device="cuda")
    xs_, g_, b_ = to_dev(xs), to_dev(g), to_dev(b)
    assert hip.lib().uspace_layernorm_f32(hip.ptr(xs_), hip.ptr(g_), hip.ptr(b_), hip.ptr(y), 37, 768, ctypes.c_float(1e-5),
                                          hip.stream_ptr()) == 0
    np.testing.assert_allclose(y.cpu().numpy(), C.layernorm(xs, g, b, eps=1e-5), rtol=1e-4, atol=2e-5)


class _WordTokenizer:
    """Whitespace tokenizer with the HF call surface the embedder uses (the CLIP BPE files are not in the image)."""
    bos, eos = 998, 999

    def __init__(self):
        self.vocab = {}

    def _id(self, w):
        return self.vocab.setdefault(w, 1 + len(self.vocab))

    def encode(self, text):
        return [self.bos] + [self._id(w) for w in text.split(" ")] + [self.eos]

    def decode(self, ids):
        inv = {v: k for k, v in self.vocab.items()}
        return " ".join(inv.get(i, "") for i in ids)

    def __call__(self, text, truncation=True, max_length=77, return_length=True, return_overflowing_tokens=False,
                 padding="max_length", return_tensors="pt"):
        rows = []
        for t in ([text] if isinstance(text, str) else text):
            ids = self.encode(t)[:max_length]
            rows.append(ids + [self.eos] * (max_length - len(ids)))
        return {"input_ids": torch.tensor(rows, dtype=torch.long)}


def test_frozen_clip_embedder_surface(golden_dir):
    from uspace_amd.libs.clip import FrozenCLIPEmbedder
    z, meta, m = _tiny(golden_dir)
    emb = FrozenCLIPEmbedder(tokenizer=_WordTokenizer(), transformer=m, device="cuda")
    ctx = emb.encode(["a photo of a cat", "two dogs are running on the grass"])
    assert ctx.shape == (2, 77, 128) and bool(torch.isfinite(ctx).all())
    assert torch.equal(emb(["a photo of a cat"]), ctx[:1])
    assert not any(p.requires_grad for p in emb.parameters())
    assert emb.get_word_inds("two dogs are running", "dogs").tolist() == [2]       # 1-based: <bos> is position 0
    assert emb.get_word_inds("two dogs are running", 3).tolist() == [4]
    # the context drives the T2I network's 77 context tokens (tools/utils_t2i.py:25-39 -> libs/uvit_t2i.py:318)
    from uspace_amd.tools.utils_uvit import get_nnet
    net = get_nnet("uvit_t2i", img_size=16, patch_size=2, in_chans=4, embed_dim=64, depth=2, num_heads=1, clip_dim=128,
                   num_clip_token=77).cuda()
    out, _ = net(torch.randn(2, 4, 16, 16, device="cuda"), torch.full((2,), 0.5, device="cuda"), context=ctx)
    assert out.shape == (2, 4, 16, 16) and bool(torch.isfinite(out).all())


def test_clip_large_shape_runs():
    from uspace_amd.libs.clip import CLIPTextTransformer, CLIP_L_TEXT
    torch.manual_seed(5)
    m = CLIPTextTransformer(**CLIP_L_TEXT).cuda()
    ids = torch.randint(0, 49408, (4, 77), device="cuda")
    out = m(ids)
    assert out.shape == (4, 77, 768) and bool(torch.isfinite(out).all()) and 0.5 < float(out.std()) < 2.0
    assert torch.equal(m(ids[2:3].contiguous()), out[2:3])
