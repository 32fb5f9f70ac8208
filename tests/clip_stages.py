"""float64 restatement of the CLIP text transformer (HF CLIPTextModel(input_ids).last_hidden_state, the encoder behind the
reference's FrozenCLIPEmbedder, libs/clip.py:40-91) for the tests, layer by layer, with torch CPU ops.  Written from the math.

``mode="loose"``: plain float64 from the fp32 parameters.  ``mode="tight"``: rounded to bf16 exactly where clip.hip rounds --
the GEMM weights (pack time), the LN1 output, the qkv output, the attention P (before P.V; the normaliser is the sum of the
ROUNDED P, as the kernel's ones-tile sum is), the attention output, the LN2 output, the fc1 output and the quick-GELU output.
The residual stream, biases, LayerNorm parameters and the tables stay fp32 / float64.

Also here: a seeded CLIP-L parameter generator in HF ``state_dict`` order (a "workflow" set whose branches move the residual
stream by a sizeable fraction of its size, and a "stress" set with a massive first token, a large end-of-text channel, an
attention-sink head and a sharp head) and prompt-shaped token ids (BOS, words, EOS padding to 77)."""
import torch
import torch.nn.functional as F

BOS, EOS = 49406, 49407
CLIP_L = dict(vocab_size=49408, hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12,
              max_position_embeddings=77, layer_norm_eps=1e-5)
SINK_HEAD, SHARP_HEAD = 3, 7          # stress set: the attention-sink head and the 4x sharper head (every layer)
MASSIVE = (11, 200, 451, 700)         # stress set: channels of position row 0 at +-64


def cpu_threads():
    """Cap torch's CPU pool at 16 threads (the GPU machines' share); returns the old count."""
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 16))
    return n


def _bf(x, on):
    return x.to(torch.bfloat16).to(x.dtype) if on else x


def _w(sd, name, tight):
    """A GEMM weight as float64: bf16-rounded from fp32 in tight mode (uspace_clip_pack_weights)."""
    w = sd[name]
    return (w.to(torch.bfloat16) if tight else w).to(torch.float64)


def _v(sd, name):
    return sd[name].to(torch.float64)


def n_layers(sd):
    n = 0
    while f"encoder.layers.{n}.layer_norm1.weight" in sd:
        n += 1
    return n


def quick_gelu(x):
    return x * torch.sigmoid(1.702 * x)


def causal_attention(q, k, v, heads, tight, fault=None):
    """q, k, v [B, L, D] float64 -> [B, L, D]: softmax(q k^T / 8 + causal mask) v per head (head_dim 64).  Tight: P is
    rounded to bf16 and normalised by the sum of the rounded values; the output is rounded to bf16.  ``fault``: one of the
    attention entries of FAULTS planted."""
    B, L, D = q.shape
    sh = lambda t: t.reshape(B, L, heads, D // heads).transpose(1, 2)
    s = sh(q) @ sh(k).transpose(-1, -2) / (65.0 ** 0.5 if fault == "scale_1/sqrt65" else 8.0)
    if fault != "no_mask":
        s = s.masked_fill(~torch.ones(L, L, dtype=torch.bool).tril(1 if fault == "mask_allows_next_token" else 0), float("-inf"))
    p = _bf(torch.exp(s - s.amax(-1, keepdim=True)), tight)
    o = (p @ sh(v)) / p.sum(-1, keepdim=True)
    return _bf(o.transpose(1, 2).reshape(B, L, D), tight)


def _ln(x, w, b, eps, fault=None):
    """LayerNorm in float64; ``unbiased_var``: the variance over D - 1, ``eps_1e-6``: eps 1e-6 whatever the argument."""
    D = x.shape[-1]
    if fault == "eps_1e-6":
        eps = 1e-6
    if fault == "unbiased_var":
        return (x - x.mean(-1, keepdim=True)) / torch.sqrt(x.var(-1, unbiased=True, keepdim=True) + eps) * w + b
    return F.layer_norm(x, (D,), w, b, eps)


def layer(x, sd, i, mode, heads=12, eps=1e-5, fault=None):
    """One pre-LN block (layer i of ``sd``): x [B, L, D] -> x + attn(LN1 x) then + MLP(LN2 .), float64.  ``fault``: one of the
    layer entries of FAULTS planted."""
    t = mode == "tight"
    pre = f"encoder.layers.{i}."
    x = x.to(torch.float64)
    lin = lambda a, n: a @ _w(sd, pre + n + ".weight", t).T + _v(sd, pre + n + ".bias")
    h = _bf(_ln(x, _v(sd, pre + "layer_norm1.weight"), _v(sd, pre + "layer_norm1.bias"), eps, fault), t)
    q, k, v = (_bf(lin(h, f"self_attn.{n}_proj"), t) for n in "qkv")
    x = x + lin(causal_attention(q, k, v, heads, t, fault), "self_attn.out_proj")
    h = _bf(_ln(x, _v(sd, pre + "layer_norm2.weight"), _v(sd, pre + "layer_norm2.bias"), eps, fault), t)
    f1 = _bf(lin(h, "mlp.fc1"), t)
    h = _bf(F.gelu(f1) if fault == "erf_gelu" else quick_gelu(f1), t)
    return x + lin(h, "mlp.fc2")


def embed(ids, sd):
    """tok[ids] + pos[:L], added in fp32 as the table kernel adds (exact), returned as float64."""
    ids = torch.as_tensor(ids, dtype=torch.long)
    return (sd["embeddings.token_embedding.weight"][ids] + sd["embeddings.position_embedding.weight"][:ids.shape[1]]).to(torch.float64)


def final_norm(x, sd, eps=1e-5, fault=None):
    x = x.to(torch.float64)
    if fault == "no_final_ln":
        return x
    fault = {"final_eps_1e-6": "eps_1e-6", "final_unbiased_var": "unbiased_var"}.get(fault, fault)
    return _ln(x, _v(sd, "final_layer_norm.weight"), _v(sd, "final_layer_norm.bias"), eps, fault)


def forward(ids, sd, mode, heads=12, eps=1e-5, taps=True, stop_after=None, fault=None):
    """ids [B, L] -> (last_hidden_state, [hidden state after k layers for k = 0 ..]) in float64; ``stop_after=k``: return the state
    after k layers (HF hidden_states[k]) instead of the final-LN output.  ``fault``: one entry of FAULTS planted wherever it acts."""
    x = embed(ids, sd)
    hidden = [x] if taps else None
    n = n_layers(sd) if stop_after is None else stop_after
    for i in range(n):
        x = layer(x, sd, i, mode, heads, eps, fault)
        if taps:
            hidden.append(x)
    out = x if stop_after is not None else final_norm(x, sd, eps, fault)
    return out, hidden


# ------------------------------------------------------------------------------------------------------------------ faults
# name -> (metric that excludes the fault, what it does), in the convention of tests/dino_cases.py and tests/uvit_stages.py:
#   "update_tight", "final_ln": TOL entries of tests/test_gpu_clip_parity.py -- the faulty float64 model lies FAULT_MARGIN bounds from
#       the true one, layers measured one by one from the true previous state;
#   "projection": the layer's residual projected onto the fault's direction (tests/util.py::fault_projection), bound PROJECTION_GPU
#       on the GPU, within PROJECTION_HOST of 0 / of 1 without / with the fault on the CPU (workflow parameters: on the stress set
#       the massive token's rounding correlates with the LayerNorm directions, c_f reaches 0.33 without a fault);
#   UNIT_TESTS: besides, excluded by the GPU unit test named there, by FAULT_MARGIN of its bound.  The eps fault is a plain fault
#       only on the "tiny" parameter set, in layer 0, whose rows have a variance of the order of eps
#       (tests/test_gpu_clip_parity.py::test_layer_0_normalises_rows_at_eps): that pins the eps clip.hip hands on, the unit test the kernels.
# tests/test_clip_faults_host.py proves every entry.  Beside the projection faults: the largest |c_f| an MI355X measured
# (tests/test_gpu_clip_parity.py::test_no_planted_fault_explains_the_gpu_error, 12 layers, 4 prompts).
# The text transformer does not pool: the pooled row is taken by the text head, whose suite has that fault
# (tests/clip_vision_cases.py::pooled_index, tests/test_clip_vision_host.py::test_pooled_index_follows_hf), so none is planted here.
FAULT_MARGIN = 10.0
PROJECTION_HOST = 0.25
PROJECTION_GPU = 0.5
FAULTS = {
    "mask_allows_next_token": ("update_tight", "causal mask one diagonal too wide"),
    "no_mask": ("update_tight", "no causal mask"),
    "erf_gelu": ("projection", "erf-GELU instead of quick-GELU"),                            # measured |c_f| 0.001
    "scale_1/sqrt65": ("projection", "logits scaled by 1 / sqrt(65) instead of 1 / 8"),     # measured |c_f| 0.013
    "unbiased_var": ("projection", "LayerNorm variance over D - 1 (layers and final norm)"),  # measured |c_f| 0.016
    "eps_1e-6": ("update_tight", "LayerNorm eps 1e-6 instead of 1e-5 in the layers"),       # layer 0 of the tiny set (the eps clip.hip passes), and UNIT_TESTS
    "final_eps_1e-6": ("final_ln", "final LayerNorm with eps 1e-6"),
    "final_unbiased_var": ("final_ln", "final LayerNorm with the variance over D - 1"),
    "no_final_ln": ("final_ln", "final LayerNorm omitted"),
}
UNIT_TESTS = {"eps_1e-6": ("tests/test_gpu_clip_parity.py::test_layernorm_kernels_at_d768",)}
FAULT_IDS = (8, 201, (0, 1, 4, 7))        # prompt_ids(n, seed) and the sampled prompts: the empty one, the full one and two ragged ones


# ------------------------------------------------------------------------------------------------------------------ parameters
def clip_params(kind="workflow", seed=0, vocab_size=49408, hidden_size=768, intermediate_size=3072, num_hidden_layers=12,
                num_attention_heads=12, max_position_embeddings=77, **_ignored):
    """Seeded fp32 parameters in HF state_dict order (no ``text_model.`` prefix).  ``kind="workflow"``: every branch moves the
    residual stream by roughly 0.1-1x its size; LN gamma / beta and every bias are non-trivial.  ``kind="stress"``: the same plus
    a massive first token (channels MASSIVE of position row 0 at +-64), an end-of-text table row with one channel at 40, head
    SINK_HEAD whose logits for key 0 (the massive token) exceed the others by about 20-40 in every layer, and head SHARP_HEAD with
    4x sharper logits.  ``kind="tiny"``: the workflow set with the two tables at 0.003x (the eps of layer 0's norms shows)."""
    g = torch.Generator().manual_seed(seed)
    D, Fd, H = hidden_size, intermediate_size, num_attention_heads
    rn = lambda *s: torch.randn(*s, generator=g)
    sd = {"embeddings.token_embedding.weight": rn(vocab_size, D) * 0.5,
          "embeddings.position_embedding.weight": rn(max_position_embeddings, D) * 0.2}
    for i in range(num_hidden_layers):
        pre = f"encoder.layers.{i}."
        gain = 1.0 + 0.1 * i        # later layers write larger updates (the residual stream grows)
        for n, s in (("k", 1.4), ("v", 1.0), ("q", 1.4), ("out", 0.45 * gain)):
            sd[pre + f"self_attn.{n}_proj.weight"] = rn(D, D) * (s / D ** 0.5)
            sd[pre + f"self_attn.{n}_proj.bias"] = rn(D) * 0.1
        sd[pre + "layer_norm1.weight"] = 1.0 + 0.2 * rn(D)
        sd[pre + "layer_norm1.bias"] = 0.1 * rn(D)
        sd[pre + "mlp.fc1.weight"] = rn(Fd, D) * (1.0 / D ** 0.5)
        sd[pre + "mlp.fc1.bias"] = rn(Fd) * 0.3
        sd[pre + "mlp.fc2.weight"] = rn(D, Fd) * (0.6 * gain / Fd ** 0.5)
        sd[pre + "mlp.fc2.bias"] = rn(D) * 0.1
        sd[pre + "layer_norm2.weight"] = 1.0 + 0.2 * rn(D)
        sd[pre + "layer_norm2.bias"] = 0.1 * rn(D)
    sd["final_layer_norm.weight"] = 1.0 + 0.2 * rn(D)
    sd["final_layer_norm.bias"] = 0.1 * rn(D)
    if kind == "tiny":          # workflow with both tables at 0.003x: layer 0 normalises rows with a variance of 2.6e-6, of the order of eps
        sd["embeddings.token_embedding.weight"] *= 0.003
        sd["embeddings.position_embedding.weight"] *= 0.003
    if kind == "stress":
        pos, tok = sd["embeddings.position_embedding.weight"], sd["embeddings.token_embedding.weight"]
        sign = torch.tensor([1.0, -1.0, 1.0, -1.0])[:len(MASSIVE)]
        pos[0, list(MASSIVE)] = 64.0 * sign
        tok[EOS, 5] = 40.0
        dh = 64
        e = rn(dh)
        e = e / e.norm()
        for i in range(num_hidden_layers):
            pre = f"encoder.layers.{i}."
            # sink: the LN1 output of the massive token is about +-13.9 on MASSIVE (sqrt(D / 4)), a few tenths elsewhere; the head's
            # key picks that up along e, and its query bias points along e for every token: q . k0 / 8 ~ 4 * 1.3 * 13.9 * 4 / 8 ~ 36
            # above the key noise, of which the LN gamma / residual drift leaves about 20-40 over the other keys
            rows = slice(SINK_HEAD * dh, (SINK_HEAD + 1) * dh)
            wk = sd[pre + "self_attn.k_proj.weight"]
            wk[rows] *= 0.25
            wk[rows][:, list(MASSIVE)] += 1.3 * e[:, None] * sign[None, :]
            sd[pre + "self_attn.q_proj.bias"][rows] = 4.0 * e
            sd[pre + "self_attn.q_proj.weight"][rows] *= 0.25
            # sharp: 4x the logits of one head
            rows = slice(SHARP_HEAD * dh, (SHARP_HEAD + 1) * dh)
            sd[pre + "self_attn.q_proj.weight"][rows] *= 4.0
            sd[pre + "self_attn.q_proj.bias"][rows] *= 4.0
    return sd


def prompt_ids(n, seed=0, lengths=None, vocab_size=49408, max_len=77):
    """n prompt-shaped rows [n, max_len] (torch.long): BOS at 0, then 0-75 word ids, then EOS padding to max_len -- the HF
    tokenizer's output with padding="max_length".  Row 0 is the empty prompt (BOS then only padding); word ids 0 and
    vocab_size - 3 (the largest below BOS) occur, so with EOS both edges of the table are read."""
    g = torch.Generator().manual_seed(seed)
    if lengths is None:
        lengths = [0] + torch.randint(1, max_len - 1, (n - 1,), generator=g).tolist()
        if n > 2:
            lengths[1] = max_len - 2          # a prompt that fills the context
    ids = torch.full((n, max_len), EOS, dtype=torch.long)
    ids[:, 0] = BOS
    for r, w in enumerate(lengths):
        ids[r, 1:1 + w] = torch.randint(0, BOS, (w,), generator=g)
    if n > 1 and lengths[1] >= 2:
        ids[1, 1], ids[1, 2] = 0, BOS - 1
    return ids
