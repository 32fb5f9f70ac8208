"""CLIP's image side on the GPU (uspace_amd/csrc/clip_vision.hip) against the float64 restatement of tests/clip_vision_cases.py and
the Hugging Face golden: the preprocessing at five sizes, the tower stage by stage through the tap at six shapes (pad path, one key
tile, no pad, the production token count, the streaming attention kernel, the CLIP-L width), the fp32 projections, the row gather
and the cosine, bit-equality from run to run, the packed blob, empty batches, host tensors, and the text tower left undisturbed.

Bounds: ``C.TOL`` -- 3x what an MI355X measured, written beside each entry."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from tests import clip_vision_cases as C

pytestmark = pytest.mark.gpu


def _module(name):
    from uspace_amd.libs.clip import CLIPVisionTransformer
    cfg = C.TOWER_CASES[name][0]
    m = CLIPVisionTransformer(**cfg)
    m.load_state_dict(C.case_params(name))
    return m.cuda()


@pytest.fixture(scope="module")
def threads():
    n = C.S.cpu_threads()
    yield
    torch.set_num_threads(n)


# ------------------------------------------------------------------------------------------------------------------ preprocessing
@pytest.mark.parametrize("quantize", [True, False])
@pytest.mark.parametrize("H,S", C.PREPROCESS_SIZES)
def test_preprocess_against_float64(threads, H, S, quantize):
    from uspace_amd.libs.clip import CLIPVisionTransformer
    m = CLIPVisionTransformer(**dict(C.TINY_VISION, image_size=S, num_hidden_layers=0))
    img = C.make_images(2, H, seed=1, kind="mixed")
    ref = C.preprocess(img, S, quantize=quantize)
    got = m.preprocess(img.cuda(), quantize=quantize).cpu()
    e = C.maxabs(got, ref)
    edge = max(C.maxabs(got[..., r, :], ref[..., r, :]) for r in (0, -1))
    edge = max(edge, max(C.maxabs(got[..., :, c], ref[..., :, c]) for c in (0, -1)))
    print(f"preprocess {H}->{S} quantize={quantize}: max abs {e:.2e} (first / last rows and columns {edge:.2e})")
    assert e < C.TOL["preprocess"]
    if H == S and quantize:       # the identity resize: exactly the quantised value, normalised
        q = torch.floor(img * 255.0 + 0.5).clamp(0, 255)
        assert C.maxabs(got, (q.double() / 255.0 - ref.new_tensor(C.CLIP_MEAN).view(1, 3, 1, 1)) / ref.new_tensor(C.CLIP_STD).view(1, 3, 1, 1)) < 1e-6


def test_preprocess_refuses_what_it_does_not_do():
    from uspace_amd import _hip
    L = _hip.lib()
    x = torch.rand(1, 3, 32, 48, device="cuda")
    out = torch.empty(1, 3, 16, 16, device="cuda")
    m3, s3 = (ctypes.c_float * 3)(*C.CLIP_MEAN), (ctypes.c_float * 3)(*C.CLIP_STD)
    assert L.uspace_clip_preprocess(_hip.ptr(x), _hip.ptr(out), 1, 32, 48, 16, 1, m3, s3, _hip.stream_ptr()) == -1     # not square
    assert L.uspace_clip_preprocess(_hip.ptr(x), _hip.ptr(out), 1, 8192, 8192, 16, 1, m3, s3, _hip.stream_ptr()) == -1
    from uspace_amd.libs.clip import CLIPVisionTransformer
    with pytest.raises(ValueError):
        CLIPVisionTransformer(**C.TINY_VISION).preprocess(x)


# ------------------------------------------------------------------------------------------------------------------ the tower
@pytest.fixture(scope="module")
def tower_refs(threads):
    """case -> (pixel_values, state dict, float64 loose forward), computed once."""
    cache = {}

    def get(name):
        if name not in cache:
            pv, sd = C.case_pixels(name), C.case_params(name)
            cache[name] = (pv, sd, C.vision_forward(pv, sd, C.TOWER_CASES[name][0]["num_attention_heads"], "loose"))
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(C.TOWER_CASES))
def test_tower_stage_by_stage(tower_refs, name):
    from uspace_amd import _hip
    cfg = C.TOWER_CASES[name][0]
    heads, nl = cfg["num_attention_heads"], cfg["num_hidden_layers"]
    pv, sd, ref = tower_refs(name)
    m = _module(name)
    dev = pv.cuda()
    emb = m(dev, hidden_state="embeddings").cpu()
    _hip.prof_all_begin()
    T = [m(dev, hidden_state=k).cpu() for k in range(nl + 1)]
    recs = [r for r in _hip.prof_all_end() if r["kind"] == 1]
    # which attention kernel ran: the recorder's flag 2 marks the streaming form
    tokens = (cfg["image_size"] // cfg["patch_size"]) ** 2 + 1
    assert recs and all(r["N"] == tokens for r in recs)
    assert all(bool(r["flags"] & 2) == (tokens > 336) for r in recs), recs
    e_loose = C.rel(emb, ref["embeddings"])
    e_tight = C.rel(emb, C.embeddings(pv, sd, "tight"))
    hid = [C.rel(T[k], ref["hidden"][k]) for k in range(nl + 1)]
    upd = []
    for k in range(1, nl + 1):
        R = C.layer(T[k - 1], sd, k - 1, "tight", heads)
        upd.append(float((T[k].double() - R).norm() / (T[k].double() - T[k - 1].double()).norm()))
    img, pool = m(dev, return_pooled=True)
    img, pool = img.cpu(), pool.cpu()
    e_pool = C.rel(pool, C.pooled(T[nl], sd))
    e_lin = C.rel(img, pool.double() @ sd["visual_projection.weight"].double().T)
    e_img = C.rel(img, ref["image_embeds"])
    print(f"tower {name}: embeddings loose {e_loose:.2e} tight {e_tight:.2e}; hidden", ["%.2e" % h for h in hid], "update",
          ["%.2e" % u for u in upd], f"pooler {e_pool:.2e} projection {e_lin:.2e} image_embeds {e_img:.2e}")
    assert e_loose < C.TOL["embeddings"] and e_tight < C.TOL["embeddings_tight"]
    assert max(hid) < C.TOL["hidden"], hid
    assert max(upd) < C.TOL["update"], upd
    assert e_pool < C.TOL["pooler"] and e_lin < C.TOL["linear"] and e_img < C.TOL["image_embeds"]
    if name == "tiny":           # ... and against what HF computed (its own fp32 noise, 4e-7, is far inside the bounds)
        z = C.load_golden()[0]
        assert C.rel(emb, z["embeddings"]) < C.TOL["embeddings"]
        assert max(C.rel(T[k], z["hidden_states"][k]) for k in range(3)) < C.TOL["hidden"]
        assert C.rel(pool, z["pooler_output"]) < C.TOL["image_embeds"] and C.rel(img, z["image_embeds"]) < C.TOL["image_embeds"]
    # run to run: the same bits
    assert torch.equal(m(dev).cpu(), img)
    assert torch.equal(m(dev, hidden_state=nl).cpu(), T[nl])


def test_image_embeds_and_cosine_against_the_golden(threads):
    from uspace_amd.libs.clip import CLIPTextProjection, CLIPTextTransformer
    from uspace_amd.tools.clip_score import cosine
    z, sd = C.load_golden()
    m = _module("tiny")
    text = CLIPTextTransformer(**C.TINY_TEXT)
    text.load_state_dict(sd)
    proj = CLIPTextProjection(128, 64)
    proj.load_state_dict(sd)
    text, proj = text.cuda(), proj.cuda()
    ids = torch.from_numpy(z["input_ids"]).cuda()
    img = m(torch.from_numpy(z["pixel_values"]).cuda())
    te = proj(text(ids), ids)
    e_txt = C.rel(te.cpu(), z["text_embeds"])
    worst = 0.0
    for shift in range(3):           # every (image, prompt) pair of the 3 x 3 matrix, three pairings
        perm = [(i + shift) % 3 for i in range(3)]
        got = cosine(img, te[perm]).cpu()
        worst = max(worst, C.maxabs(got, z["cosine"][np.arange(3), perm]))
    print(f"golden: text_embeds {e_txt:.2e}, cosine max abs {worst:.2e}")
    assert e_txt < C.TOL["text_embeds"] and worst < C.TOL["cosine"]


# ------------------------------------------------------------------------------------------------------------------ the fp32 pieces
@pytest.mark.parametrize("B", [1, 3, 64])
@pytest.mark.parametrize("D", [64, 768, 1024])
def test_linear_gather_cosine_against_float64(B, D):
    from uspace_amd import _hip
    from uspace_amd.tools.clip_score import cosine, normalized_diff
    L = _hip.lib()
    g = torch.Generator().manual_seed(40 + B * 7 + D)
    N = 770 if D == 768 else 768                                  # 770: a last block of two columns
    x, w = torch.randn(B, D, generator=g), torch.randn(N, D, generator=g) / D ** 0.5
    out = torch.empty(B, N, device="cuda")
    dx, dw = x.cuda(), w.cuda()
    _hip.check(L.uspace_linear_f32(_hip.ptr(dx), _hip.ptr(dw), _hip.ptr(out), B, N, D, _hip.stream_ptr()), "linear")
    e_lin = C.rel(out.cpu(), x.double() @ w.double().T)
    # gather: exact
    T = 7
    seq = torch.randn(B, T, D, generator=g)
    idx = torch.randint(0, T, (B,), generator=g, dtype=torch.int32)
    idx[0], idx[-1] = T - 1, 0
    got = torch.empty(B, D, device="cuda")
    ds, di = seq.cuda(), idx.cuda()
    _hip.check(L.uspace_gather_rows_f32(_hip.ptr(ds), _hip.ptr(di), _hip.ptr(got), B, T, D, _hip.stream_ptr()), "gather")
    assert torch.equal(got.cpu(), seq[torch.arange(B), idx.long()])
    # cosine: random pairs, a nearly parallel pair, an opposite pair (relu), a large-norm pair
    a, b = torch.randn(B, D, generator=g), torch.randn(B, D, generator=g)
    b[0] = a[0] * 3.0 + 1e-3 * b[0]
    if B > 1:
        b[1] = -a[1]
        a[-1] *= 1e4
    ref = C.cosine(a, b)
    e_cos = C.maxabs(cosine(a.cuda(), b.cuda()).cpu(), ref)
    e_score = C.maxabs(cosine(a.cuda(), b.cuda(), scale=100.0, relu=True).cpu(), C.clip_score(a, b))
    nd = lambda t: t.double() / t.double().norm(dim=-1, keepdim=True)
    e_diff = C.maxabs(normalized_diff(a.cuda(), b.cuda()).cpu(), nd(a) - nd(b))
    print(f"ops B={B} D={D}: linear {e_lin:.2e} cosine {e_cos:.2e} score {e_score:.2e} normalised difference {e_diff:.2e}")
    assert e_lin < C.TOL["linear"] and e_cos < C.TOL["cosine_op"] and e_score < 100.0 * C.TOL["cosine_op"] and e_diff < C.TOL["cosine_op"]
    assert torch.equal(cosine(a.cuda(), b.cuda()), cosine(a.cuda(), b.cuda()))


# ------------------------------------------------------------------------------------------------------------------ contract
def test_blob_digest_is_stable_and_pad_columns_are_zero():
    from tests import blob_cases
    from uspace_amd import _hip
    m = _module("tiny")
    tensors = list(m.parameters())
    d1 = blob_cases.blob_digest("uspace_clipv_", m._c_cfg(), tensors)
    assert d1 == blob_cases.blob_digest("uspace_clipv_", m._c_cfg(), tensors)
    # the patch weight inside the blob: bf16 [D, 640], columns 588 .. 639 zero, the rest the cast of the parameter
    blob = m._packed_blob(torch.device("cuda"))
    off = 512                                                   # behind the class embedding (128 floats)
    w = blob[off:off + 128 * 640 * 2].view(torch.bfloat16).view(128, 640).cpu()
    want = m.vision_model.embeddings.patch_embedding.weight.detach().reshape(128, 588).to(torch.bfloat16).cpu()
    assert torch.equal(w[:, :588], want) and not bool(w[:, 588:].any())
    assert m._packed_blob(torch.device("cuda")) is blob          # cached
    m.invalidate_packed()
    assert m._packed_blob(torch.device("cuda")) is not blob


def test_empty_batch_and_host_tensors():
    from uspace_amd import _hip
    from uspace_amd.libs.clip import CLIPTextProjection
    m = _module("tiny")
    assert m(torch.empty(0, 3, 56, 56, device="cuda")).shape == (0, 64)
    assert m(torch.empty(0, 3, 56, 56, device="cuda"), hidden_state=1).shape == (0, 17, 128)
    assert m.preprocess(torch.empty(0, 3, 64, 64, device="cuda")).shape == (0, 3, 56, 56)
    p = CLIPTextProjection(128, 64).cuda()
    assert p(torch.empty(0, 77, 128, device="cuda"), torch.empty(0, 77, dtype=torch.long, device="cuda")).shape == (0, 64)
    with pytest.raises(_hip.UspaceHipError):
        m(torch.zeros(1, 3, 56, 56))
    with pytest.raises(_hip.UspaceHipError):
        m.preprocess(torch.zeros(1, 3, 64, 64))
    with pytest.raises(_hip.UspaceHipError):
        p(torch.zeros(1, 77, 128), torch.zeros(1, 77, dtype=torch.long))
    with pytest.raises(ValueError):
        m(torch.zeros(1, 3, 28, 28, device="cuda"))


def test_text_forward_is_bit_equal_after_vision_calls(golden_dir):
    """The two towers share the workspace and cache code: the text forward on clip_text_tiny.npz gives the same bits before and
    after vision forwards (and a preprocessing) ran in between."""
    from uspace_amd.libs.clip import CLIPTextTransformer
    z = np.load(os.path.join(golden_dir, "clip_text_tiny.npz"))
    meta = json.loads(bytes(z["meta_json"]).decode())
    text = CLIPTextTransformer(**{k: meta[k] for k in ("vocab_size", "hidden_size", "intermediate_size", "num_hidden_layers",
                                                       "num_attention_heads", "max_position_embeddings", "layer_norm_eps", "hidden_act")})
    text.load_state_dict({"text_model." + k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd/")})
    text = text.cuda()
    ids = torch.from_numpy(z["ids"]).cuda()
    before = text(ids).clone()
    m = _module("tiny")
    pv = C.case_pixels("tiny").cuda()
    m(pv)
    m.preprocess(C.make_images(2, 64).cuda())
    m(pv, hidden_state=1)
    assert torch.equal(text(ids), before)
