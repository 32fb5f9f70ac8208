"""float64 restatement of the U-ViT velocity network (libs/uvit.py:306-351, libs/uvit_t2i.py:308-342) for the tests, block by
block, with torch CPU ops.  Written from the math; citations are relative to the reference's root, as in oracle/uvit_oracle.py.

Pieces: ``embed`` (tokens as block 0 reads them), ``block`` (one pre-LN block, with the long skip for out-blocks and the per-block
attention-map column factors), ``mid_hook`` (the u-space write after the mid block) and ``head`` (final LayerNorm, decoder_pred,
unpatchify, conv3x3).  ``forward`` chains them.

Modes:
``loose``      plain float64 from the fp32 parameters.
``tight_sep``  rounded to bf16 exactly where the separate-launch path of uvit.hip (``uspace_uvit_set_ln_fold(0)``) rounds: the
               LayerNorm outputs, every GEMM weight, the qkv output, the attention P before P.V (normalised by the sum of the
               ROUNDED, UNSCALED P; under key_scale the P.V operand is bf16(P * ks)), the attention output, the GELU output and the bf16
               copies of x that feed the skips and skip_linear.
``tight_fold`` rounded where the LayerNorm-folded path rounds: the centred copy bf16(x - c) with c the row mean at
               the previous norm of the same row (the block's ``c_in``, returned by the previous block as its norm-2 mean; the
               embed's row mean for block 0), the folded weights bf16(W * gamma) with their column sums and the fp32 W beta bias
               terms, the skip slab stored centred by the in-block's norm-2 mean plus the rank-1 term cskip * rowsum(bf16(W2)); the
               attention and GELU roundings are those of tight_sep.
``rounding=False`` keeps a tight mode's data flow (centring, folding, rank-1 term) with every rounding switched off: it must
collapse to ``loose``.  The residual stream, biases, LayerNorm statistics, the embed and the head stay float64 in every mode (the
GPU keeps them in fp32; the context GEMM of text-to-image models has bf16 operands, which ``embed(tight=True)`` rounds).

Also here: seeded parameter sets at any width (``make_net``): ``workflow`` = the module's own seeded init (what the reference
produces: LayerNorms (1, 0), zero Linear biases), ``stress`` = non-trivial gamma / beta on every norm, non-zero biases, pos_embed
row offsets that dwarf the row std, massive channels, outlier tokens, a sink head and a sharp head."""
import math

import torch
import torch.nn.functional as F

MODES = ("loose", "tight_sep", "tight_fold")
EPS = 1e-5
SINK_HEAD, SHARP_HEAD = 1, 3              # stress set: heads (of every block) with a key-0 sink and with 4x sharper logits


def cpu_threads():
    """Cap torch's CPU pool at 16 threads (the GPU machines' share); returns the old count."""
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 16))
    return n


def _bf(x, on):
    return x.to(torch.bfloat16).to(torch.float64) if on else x


def _d(t):
    return torch.as_tensor(t).to(torch.float64)


class Spec:
    """Shapes of one U-ViT (libs/uvit.py:183-232, libs/uvit_t2i.py:193-236): ``n_extra`` 0 (uncond), 1 (label token, placed
    before the time token: ``time_first = 0``) or the CLIP token count (``t2i``: after the time token)."""

    def __init__(self, img_size=32, patch_size=2, in_chans=4, embed_dim=1024, depth=20, num_heads=16, mlp_ratio=4,
                 num_classes=-1, t2i=False, clip_dim=768, num_clip_token=77):
        self.img_size, self.patch_size, self.in_chans = img_size, patch_size, in_chans
        self.D, self.depth, self.H = embed_dim, depth, num_heads
        self.hidden = int(embed_dim * mlp_ratio)
        self.t2i, self.clip_dim = t2i, clip_dim
        self.n_extra = num_clip_token if t2i else (1 if num_classes > 0 else 0)
        self.num_classes = num_classes
        self.time_first = 0 if (not t2i and num_classes > 0) else 1
        self.extras = 1 + self.n_extra
        self.n_patch = (img_size // patch_size) ** 2
        self.L = self.extras + self.n_patch
        self.half = depth // 2
        self.nblocks = depth + 1

    def prefix(self, i):
        """State-dict prefix of block i in execution order (libs/uvit.py:331-340)."""
        if i < self.half:
            return f"in_blocks.{i}."
        if i == self.half:
            return "mid_block."
        return f"out_blocks.{i - self.half - 1}."


# ------------------------------------------------------------------------------------------------------------------ embed
def timestep_embedding(t, D, fault=None):
    """libs/uvit.py:26-46: [cos(t f), sin(t f)], f = exp(-log(10000) k / (D/2)); float64."""
    half = D // 2
    f = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float64) / half)
    a = _d(t)[:, None] * f[None]
    e = torch.cat([torch.sin(a), torch.cos(a)] if fault == "sin_cos_swapped" else [torch.cos(a), torch.sin(a)], -1)
    return torch.cat([e, torch.zeros_like(e[:, :1])], -1) if D % 2 else e


def embed(spec, sd, x, t, y=None, context=None, tight=False, fault=None):
    """Tokens as block 0 reads them: PatchEmbed (libs/uvit.py:171-179), the time token (time_embed = Identity), the label token
    first (libs/uvit.py:322-326) or the context tokens after the time token through context_embed (libs/uvit_t2i.py:318-323),
    + pos_embed.  ``tight``: the context GEMM's operands in bf16 (uvit.hip casts the context and packs the weight to bf16).
    ``fault``: one of the embed entries of FAULTS planted."""
    x = _d(x)
    B = x.shape[0]
    tok = F.conv2d(x, _d(sd["patch_embed.proj.weight"]), _d(sd["patch_embed.proj.bias"]), stride=spec.patch_size)
    tok = tok.flatten(2).transpose(1, 2)
    tt = _d(t).reshape(-1).expand(B) if _d(t).numel() == 1 else _d(t).reshape(-1)
    time_tok = timestep_embedding(tt, spec.D, fault)[:, None, :]
    if spec.t2i:
        ctx = _bf(_d(context), tight) @ _bf(_d(sd["context_embed.weight"]), tight).T + _d(sd["context_embed.bias"])
        h = torch.cat([time_tok, ctx, tok], 1)                         # libs/uvit_t2i.py:323
    elif spec.n_extra:
        lab = _d(sd["label_emb.weight"])[torch.as_tensor(y, dtype=torch.long)][:, None, :]
        h = torch.cat([time_tok, lab, tok] if fault == "label_after_time" else [lab, time_tok, tok], 1)   # libs/uvit.py:322-326
    else:
        h = torch.cat([time_tok, tok], 1)                              # libs/uvit.py:322
    pos = _d(sd["pos_embed"])
    if fault == "no_pos_embed_on_extras":
        pos = torch.cat([torch.zeros_like(pos[:, :spec.extras]), pos[:, spec.extras:]], 1)
    return h + pos


# ------------------------------------------------------------------------------------------------------------------ block
def _ln_stats(x, fault=None):
    mu = x.mean(-1, keepdim=True)
    var = x.var(-1, unbiased=fault == "unbiased_var", keepdim=True)
    return mu, 1.0 / torch.sqrt(var + (1e-6 if fault in ("eps_1e-6", "final_eps_1e-6") else EPS))


def attention(qkv, H, rnd, key_scale=None, fault=None):
    """libs/uvit.py:89-96 (and the post-softmax column factor of tools/utils_t2i.py:196-224 at libs/uvit_t2i.py:101-105):
    qkv [B, L, 3D] "(K H D)" -> [B, L, D], head_dim 64.  ``rnd``: P rounded to bf16, normalised by the sum of the rounded unscaled P,
    the P.V operand bf16(P * ks) under key_scale, the output rounded to bf16 (attention.hip).  ``fault``: one of the attention /
    key_scale entries of FAULTS planted."""
    B, L, _ = qkv.shape
    q, k, v = qkv.reshape(B, L, 3, H, 64).permute(2, 0, 3, 1, 4)
    ks = None if key_scale is None else _d(key_scale)[:, None, None, :]
    if fault == "last_key_dropped":
        k, v, ks = k[..., :-1, :], v[..., :-1, :], None if ks is None else ks[..., :-1]
    elif fault == "first_key_dropped":
        k, v, ks = k[..., 1:, :], v[..., 1:, :], None if ks is None else ks[..., 1:]
    s = q @ k.transpose(-1, -2) / (math.sqrt(65.0) if fault == "scale_1/sqrt65" else 8.0)
    if fault == "key_scale_pre_softmax" and ks is not None:
        s, ks = s + torch.log(ks), None
    p = torch.exp(s - s.amax(-1, keepdim=True))
    pu = _bf(p, rnd)
    pv = pu if ks is None else _bf(p * ks, rnd)
    o = (pv @ v) / (pv if fault == "key_scale_renormalised" else pu).sum(-1, keepdim=True)
    return _bf(o.transpose(1, 2).reshape(B, L, H * 64), rnd)


def gelu(x, fault=None):
    if fault == "tanh_gelu":
        return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))
    if fault == "quick_gelu":
        return x * torch.sigmoid(1.702 * x)
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def block(x, sd, spec, i, mode, skip=None, key_scale=None, c_in=None, c_skip=None, rounding=True, taps=None, fault=None):
    """Block i (libs/uvit.py:157-162): x [B, L, D] -> (x', mu2), float64; mu2 [B, L, 1] is the row mean at norm2, the centring
    constant the folded path hands on (to the next block's ``c_in``; for an in-block also its skip's ``c_skip``).
    Out-blocks take ``skip`` (the in-block output popped LIFO).  ``key_scale`` [B, L]: this block's column factors.
    tight_fold: ``c_in`` [B, L, 1] is the constant x (for out-blocks: skip_linear's output) is centred by, ``c_skip`` that of the
    skip slab; None = the row mean (exact).  ``taps`` (dict) receives the intermediates the reference goldens hold (the LN1
    output and the GELU input as the loose / separate data flow has them).  ``fault``: one of the block entries of FAULTS planted (those of the
    chaining -- which skip, which key_scale slice, where the hook goes -- are planted by ``step``)."""
    assert mode in MODES
    pre = spec.prefix(i)
    rnd = rounding and mode != "loose"
    fold = mode == "tight_fold"
    W = lambda n: _bf(_d(sd[pre + n + ".weight"]), rnd)
    dropped = {"no_proj_bias": "attn.proj.bias", "no_fc1_bias": "mlp.fc1.bias", "no_skip_bias": "skip_linear.bias"}.get(fault)
    v = lambda n: torch.zeros_like(_d(sd[pre + n])) if n == dropped else _d(sd[pre + n])
    x = _d(x)
    D = x.shape[-1]
    if skip is not None:                                               # skip_linear(cat([x, skip])), libs/uvit.py:158-159
        Wsk = _d(sd[pre + "skip_linear.weight"])
        W1, W2 = _bf(Wsk[:, :D], rnd), _bf(Wsk[:, D:], rnd)
        skip = _d(skip)
        if fault == "skip_swapped":                                    # cat([skip, x])
            x, skip = skip, x
        if fold:
            cs = skip.mean(-1, keepdim=True) if c_skip is None else _d(c_skip)
            y = _bf(x, rnd) @ W1.T + _bf(skip - cs, rnd) @ W2.T + cs * W2.sum(1) + v("skip_linear.bias")
        else:
            y = _bf(x, rnd) @ W1.T + _bf(skip, rnd) @ W2.T + v("skip_linear.bias")
        x = y
        if taps is not None:
            taps["skip"] = x
    if fold and c_in is None:
        c_in = x.mean(-1, keepdim=True)

    def norm_linear(x, c, ln, lin, bias):
        """LN(x) W^T + b, as the mode computes it; returns (value, row mean)."""
        mu, rstd = _ln_stats(x, fault)
        Wr = _d(sd[pre + lin + ".weight"])
        g, be = v(ln + ".weight"), v(ln + ".bias")
        b = v(bias) if bias else 0.0
        if not fold:
            h = _bf((x - mu) * rstd * g + be, rnd)
            return h @ _bf(Wr, rnd).T + b, mu
        Wf = _bf(Wr * g, rnd)                                          # bf16(W o gamma), its column sums, b + W beta (pack time)
        return rstd * (_bf(x - c, rnd) @ Wf.T - (mu - c) * Wf.sum(1)) + (b + Wr @ be), mu

    qkv, mu1 = norm_linear(x, c_in, "norm1", "attn.qkv", None)        # qkv_bias=False
    a = attention(_bf(qkv, rnd), spec.H, rnd, key_scale, fault) @ W("attn.proj").T + v("attn.proj.bias")
    if taps is not None:
        mu, rstd = _ln_stats(x)
        taps.update(norm1=(x - mu) * rstd * v("norm1.weight") + v("norm1.bias"), qkv=qkv, attn=a)
    x = x + a
    f, mu2 = norm_linear(x, mu1, "norm2", "mlp.fc1", "mlp.fc1.bias")
    if taps is not None:
        taps["fc1"] = f
    m = _bf(gelu(f, fault), rnd) @ W("mlp.fc2").T + v("mlp.fc2.bias")
    if taps is not None:
        taps["mlp"] = m
    return x + m, mu2


def mid_hook(x, delta, scale, row_scale=None):
    """The u-space write after the mid block (libs/uvit.py:336, libs/dissection.py:157): x + scale * row_scale[b] * delta."""
    s = torch.full((x.shape[0],), float(scale), dtype=torch.float64) if row_scale is None else float(scale) * _d(row_scale)
    return _d(x) + s[:, None, None] * _d(delta).reshape(1, *x.shape[1:])


# ------------------------------------------------------------------------------------------------------------------ head
def head(spec, sd, x, taps=None, fault=None):
    """norm -> decoder_pred on all L tokens -> drop the extras -> unpatchify -> final_layer conv3x3 (libs/uvit.py:342-347,
    56-63, 284-288); float64.  ``taps`` (dict) receives the LayerNorm and decoder_pred outputs.  ``fault``: one of the head entries of FAULTS."""
    x = _d(x)
    mu, rstd = _ln_stats(x, fault if fault == "final_eps_1e-6" else None)
    h = (x - mu) * rstd * _d(sd["norm.weight"]) + _d(sd["norm.bias"])
    if taps is not None:
        taps["norm"] = h
    h = h @ _d(sd["decoder_pred.weight"]).T + _d(sd["decoder_pred.bias"])
    if taps is not None:
        taps["dec"] = h
    h = h[:, 1:1 + spec.n_patch, :] if fault == "extras_not_dropped" else h[:, spec.extras:, :]
    B, p, C = h.shape[0], spec.patch_size, spec.in_chans
    g = spec.img_size // p
    h = h.reshape(B, g, g, p, p, C)                                    # "B (h w) (p1 p2 C) -> B C (h p1) (w p2)"
    if fault == "unpatchify_transposed":
        h = h.transpose(3, 4)
    img = h.permute(0, 5, 1, 3, 2, 4).reshape(B, C, g * p, g * p)
    return F.conv2d(img, _d(sd["final_layer.weight"]), _d(sd["final_layer.bias"]), padding=1)


def skip_source(spec, i, fault=None):
    """The in-block whose output out-block i takes: popped LIFO (libs/uvit.py:340); ``skip_fifo``: first in, first out."""
    return i - spec.half - 1 if fault == "skip_fifo" else spec.nblocks - 1 - i


def step(spec, sd, T, i, mode, key_scale=None, mid=None, c=None, cskip=None, rounding=True, mid_out=None, fault=None):
    """Stage i + 1 from the stages T[0 .. i] (a list: T[k + 1] is block k's output, the mid block's after the hook): (x', mu2) as
    ``block`` returns them.  Everything the chaining decides is decided here: which in-block output an out-block takes, which
    ``key_scale`` [depth + 1, B, L] slice the block reads and where the mid hook goes.  ``cskip[k]``: in-block k's norm-2 mean
    (tight_fold), or None."""
    prev = T[i]
    skip = cs = None
    if i > spec.half:
        si = skip_source(spec, i, fault)
        skip, cs = T[si + 1], None if cskip is None else cskip[si]
    ks = None if key_scale is None else key_scale[(i + 1) % spec.nblocks if fault == "key_scale_next_block" else i]
    hook = mid is not None and i == spec.half
    if hook and fault == "mid_hook_before_mid_block":
        prev = mid_hook(prev, *mid)
    h, c = block(prev, sd, spec, i, mode, skip=skip, key_scale=ks, c_in=c, c_skip=cs, rounding=rounding, fault=fault)
    if i == spec.half and mid_out is not None:
        mid_out.append(h)
    if hook and fault != "mid_hook_before_mid_block":
        h = mid_hook(h, *mid)
    return h, c


def forward(spec, sd, x, t, mode, y=None, context=None, key_scale=None, mid=None, rounding=True, mid_out=None, fault=None):
    """The whole network from the latents: (output [B, C, S, S], [x after stage k for k = 0 .. depth + 1]) in float64, stage k as
    uspace_uvit_forward_tap numbers it (the mid block's stage after the hook).  ``key_scale`` [depth + 1, B, L]; ``mid`` =
    (delta [L, D], scale, row_scale [B] or None); ``mid_out`` (list) receives the mid block's output before the hook.
    ``fault``: one entry of FAULTS planted wherever it acts."""
    stages = [embed(spec, sd, x, t, y=y, context=context, tight=mode != "loose" and rounding, fault=fault)]
    cskip = [None] * spec.half
    c = None
    for i in range(spec.nblocks):
        h, c = step(spec, sd, stages, i, mode, key_scale=key_scale, mid=mid, c=c, cskip=cskip, rounding=rounding, mid_out=mid_out,
                    fault=fault)
        if i < spec.half:
            cskip[i] = c
        stages.append(h)
    return head(spec, sd, stages[-1], fault=fault), stages


# ------------------------------------------------------------------------------------------------------------------ faults
# name -> (metric that excludes the fault, what it does), in the convention of tests/dino_cases.py.  The metric is
#   a TOL entry of tests/test_gpu_uvit_parity.py ("update_tight", "embed", "head"): the faulty float64 model lies at least FAULT_MARGIN
#       times that bound from the true one, measured as the GPU test measures it (blocks: from the true previous state);
#   "projection": the fault moves a block's update by less than that, so the GPU test projects its residual onto the fault's
#       direction (tests/util.py::fault_projection): 0 for a correct kernel, 1 for one with the fault; bound PROJECTION_GPU, and on
#       the CPU (tight model standing in for the GPU) within PROJECTION_HOST of 0 without and of 1 with the fault;
#   "projection_head": the same on the output against the float64 head of the last tap;
#   "unit": neither resolves it at the block level; the GPU unit tests UNIT_TESTS names do, by FAULT_MARGIN times their own bounds.
# tests/test_uvit_faults_host.py proves every entry on the CPU.  Beside each projection fault: the largest |c_f| an MI355X measured
# (tests/test_gpu_uvit_parity.py::test_no_planted_fault_explains_the_gpu_error, worst over nets, blocks and both LayerNorm modes).
FAULT_MARGIN = 10.0
PROJECTION_HOST = 0.25
PROJECTION_GPU = 0.5
FAULTS = {
    # LayerNorm of the blocks
    "unbiased_var": ("projection", "variance over D - 1"),                                   # measured |c_f| 0.008
    "eps_1e-6": ("update_tight", "eps 1e-6 instead of 1e-5"),        # block 0 of the tiny net (the eps uvit.hip passes), and UNIT_TESTS
    # attention
    "last_key_dropped": ("projection", "key L - 1 invisible (tail off by one)"),             # measured |c_f| 0.004
    "first_key_dropped": ("projection", "key 0 invisible"),                                  # measured |c_f| 0.002
    "scale_1/sqrt65": ("unit", "logits scaled by 1 / sqrt(65) instead of 1 / 8"),
    # GELU
    "tanh_gelu": ("unit", "the tanh form instead of the erf form"),
    "quick_gelu": ("projection", "x sigmoid(1.702 x)"),                                      # measured |c_f| 0.001
    # key_scale
    "key_scale_renormalised": ("projection", "P ks also in the normalising sum"),            # measured |c_f| < 0.0005
    "key_scale_next_block": ("projection", "block i reads the slice of block i + 1"),        # measured |c_f| < 0.0005
    "key_scale_pre_softmax": ("projection", "log ks added to the logits, then normalised"),  # measured |c_f| < 0.0005
    # skips
    "skip_swapped": ("update_tight", "skip_linear(cat([skip, x]))"),
    "skip_fifo": ("update_tight", "in-block outputs popped first in, first out"),
    # biases (all zero in the workflow set: the stress set)
    "no_proj_bias": ("projection", "attn.proj bias omitted"),                                # measured |c_f| < 0.0005
    "no_fc1_bias": ("projection", "mlp.fc1 bias omitted"),                                   # measured |c_f| < 0.0005
    "no_skip_bias": ("projection", "skip_linear bias omitted"),                              # measured |c_f| < 0.0005
    # mid hook
    "mid_hook_before_mid_block": ("update_tight", "the u-space write ahead of the mid block instead of behind it"),
    # embed
    "sin_cos_swapped": ("embed", "time token [sin, cos] instead of [cos, sin]"),
    "label_after_time": ("embed", "label token behind the time token"),
    "no_pos_embed_on_extras": ("embed", "pos_embed on the patch tokens alone"),
    # head
    "final_eps_1e-6": ("projection_head", "final LayerNorm with eps 1e-6"),                  # measured |c_f| 0.059
    "extras_not_dropped": ("head", "tokens 1 .. n_patch unpatchified, whatever the number of extras"),
    "unpatchify_transposed": ("head", "p1 and p2 exchanged"),
}
# unit faults -> the GPU unit tests that exclude them (tests/unit_fault_cases.py and tests/attention_cases.py hold their inputs)
UNIT_TESTS = {
    "eps_1e-6": ("tests/test_gpu_ops.py::test_layernorm", "tests/test_gpu_ops.py::test_layernorm_folded_through_gemms_rows_at_eps"),
    "tanh_gelu": ("tests/test_gpu_ops.py::test_gemm_epilogues",),
    "scale_1/sqrt65": ("tests/test_gpu_attention_parity.py::test_every_head_against_float64",),
}
# The nets of the fault tests, depth 4 (the smallest at which FIFO differs from LIFO) but the wide one: name -> (module keywords
# beside the common ones, t2i, parameter set, hooks of the inputs, batch size of the GPU test).  B = 64 at D = 1024 takes the 256x256
# plan with strips that the product runs, B = 4 the small-launch forms.
FAULT_NETS = {
    "u512": (dict(embed_dim=512, depth=4, num_heads=8, num_classes=-1), False, "workflow", "mid", 4),
    "t2i512": (dict(embed_dim=512, depth=4, num_heads=8, clip_dim=768, num_clip_token=77), True, "workflow", "ks", 4),
    "u1024": (dict(embed_dim=1024, depth=2, num_heads=16, num_classes=-1), False, "workflow", None, 64),
    "stress512": (dict(embed_dim=512, depth=4, num_heads=8, num_classes=-1), False, "stress", None, 4),
    "cond512": (dict(embed_dim=512, depth=4, num_heads=8, num_classes=1001), False, "workflow", None, 4),
    "tiny512": (dict(embed_dim=512, depth=4, num_heads=8, num_classes=-1), False, "tiny", None, 4),
}
# fault -> the nets it is measured on (it must stand clear on each); the others: the three workflow nets of the issue
_GENERAL = ("u512", "t2i512", "u1024")
FAULT_ON = {
    "key_scale_renormalised": ("t2i512",), "key_scale_next_block": ("t2i512",), "key_scale_pre_softmax": ("t2i512",),
    "skip_fifo": ("u512", "t2i512"), "mid_hook_before_mid_block": ("u512",),
    "no_proj_bias": ("stress512",), "no_fc1_bias": ("stress512",), "no_skip_bias": ("stress512",),
    "label_after_time": ("cond512",), "extras_not_dropped": ("t2i512", "cond512"), "eps_1e-6": ("tiny512",),
}


def inputs(spec, B, hooks, seed):
    """Seeded CPU inputs of a test forward: (latents [B, 4, 32, 32], per-sample times, dict of ``forward`` keywords).  hooks "ks": a
    different attention-map edit per block (a third of the columns scaled by 0.1 ... 10, the rest by 1); "mid": a u-space write with
    per-sample factors."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 4, 32, 32, generator=g)
    t = 0.05 + 0.9 * torch.rand(B, generator=g)
    kw = dict()
    if spec.t2i:
        kw["context"] = torch.randn(B, spec.n_extra, spec.clip_dim, generator=g)
    elif spec.n_extra:
        kw["y"] = torch.randint(0, spec.num_classes, (B,), generator=g)
    if hooks == "ks":
        ks = torch.ones(spec.nblocks, B, spec.L)
        for i in range(spec.nblocks):
            cols = torch.randperm(spec.L, generator=g)[:spec.L // 3]
            ks[i][:, cols] = torch.exp(2.3 * (2 * torch.rand(B, cols.numel(), generator=g) - 1))
        kw["key_scale"] = ks
    if hooks == "mid":
        kw["mid"] = (torch.randn(spec.L, spec.D, generator=g) * 0.5, 0.7, torch.linspace(-1.5, 2.0, B))
    return x, t, kw


def select_rows(kw, rows):
    """The ``forward`` keywords of ``inputs`` restricted to the samples ``rows``."""
    out = dict(kw)
    for k in ("context", "y"):
        if k in out:
            out[k] = out[k][rows]
    if "key_scale" in out:
        out["key_scale"] = out["key_scale"][:, rows]
    if "mid" in out:
        d, s, r = out["mid"]
        out["mid"] = (d, s, r[rows])
    return out


def fault_net(name):
    """(CPU module, state dict, Spec, hooks, GPU batch size) of one of FAULT_NETS."""
    kw, t2i, kind, hooks, B = FAULT_NETS[name]
    common = dict(img_size=32, patch_size=2, in_chans=4, mlp_ratio=4, qkv_bias=False, mlp_time_embed=False)
    net = make_net(dict(common, **kw), kind, seed=1234 if kind == "workflow" else 77, t2i=t2i).eval()
    spec = Spec(img_size=32, embed_dim=kw["embed_dim"], depth=kw["depth"], num_heads=kw["num_heads"],
                num_classes=kw.get("num_classes", -1), t2i=t2i)
    return net, state_dict(net), spec, hooks, B


def fault_case(name):
    """(seed of ``inputs``, the sampled samples) of one of FAULT_NETS: the GPU test and the host test take the same sample."""
    B = FAULT_NETS[name][4]
    return 900 + list(FAULT_NETS).index(name), ([B - 1] if B < 8 else [B // 3])


def fault_nets(name):
    return FAULT_ON.get(name, _GENERAL)


def fault_blocks(spec, name):
    """The blocks a block-level fault can act in."""
    if name in ("skip_swapped", "skip_fifo", "no_skip_bias"):
        return list(range(spec.half + 1, spec.nblocks))
    if name == "mid_hook_before_mid_block":
        return [spec.half]
    if name == "eps_1e-6":            # visible where the rows are tiny: behind the embed of the tiny net; block 0 grows them
        return [0]
    return list(range(spec.nblocks))


# ------------------------------------------------------------------------------------------------------------------ parameters
def make_net(spec_kwargs, kind="workflow", seed=0, t2i=False):
    """A CPU U-ViT module (uspace_amd.libs.uvit / uvit_t2i) with seeded parameters.  ``workflow``: the module's own init under
    torch.manual_seed(seed) -- the reference's init bit for bit (LayerNorms (1, 0), zero Linear biases, trunc-normal 0.02
    weights).  ``stress``: that, plus
      - gamma = 1 + 0.3 N, beta = 0.2 N on every norm; biases 0.1 N + a per-block constant on proj / fc2 / skip_linear, 0.1 N on
        fc1, decoder_pred and context_embed;
      - pos_embed: outlier tokens (rows 3, L // 3, L - 5 at 12x), then every row offset by 20 + 10 N (row means dwarf the row std:
        the centring constants and the rank-1 skip term carry most of the value), then four massive channels at +-60 whose proj /
        fc2 / skip_linear output rows are 8x / 8x / 4x;
      - head SINK_HEAD of every block: token 0 carries four sink channels at +-40, the head's keys read them and its queries read the
        massive channels, so every query's logit for key 0 leads the others by tens; head SHARP_HEAD: 4x sharper logits.
    ``tiny``: workflow with the patch embedding and pos_embed at 0.003x (the eps of block 0's norms shows)."""
    from uspace_amd.tools.utils_uvit import get_nnet
    torch.manual_seed(seed)
    net = get_nnet("uvit_t2i" if t2i else "uvit", **spec_kwargs)
    if kind == "workflow":
        return net
    if kind == "tiny":           # workflow with the patch embedding and pos_embed at 0.003x: the rows block 0 normalises have a
        with torch.no_grad():    # variance of 3e-6, of the order of the LayerNorm's eps (but the time token's row)
            for p in (net.patch_embed.proj.weight, net.patch_embed.proj.bias, net.pos_embed):
                p.mul_(0.003)
        return net
    assert kind == "stress", kind
    g = torch.Generator().manual_seed(seed + 1)
    rn = lambda *s: torch.randn(*s, generator=g)
    D, L = net.embed_dim, net.seq_len
    big = [7, 130 % D, 301 % D, D - 57]
    sink = [11, 200 % D, 333 % D, D - 21]
    sign = torch.tensor([1.0, -1.0, 1.0, -1.0])
    e = rn(64)
    e = e / e.norm()
    with torch.no_grad():
        pos = net.pos_embed
        pos[:, [3, L // 3, L - 5], :] *= 12.0
        pos.add_(20.0 + 10.0 * rn(1, L, 1))
        pos[:, :, big] += 60.0 * sign
        pos[:, 0, sink] += 40.0 * sign
        for i, blk in enumerate(net._blocks()):
            for n in (blk.norm1, blk.norm2):
                n.weight.copy_(1.0 + 0.3 * rn(D))
                n.bias.copy_(0.2 * rn(D))
            blk.attn.proj.bias.copy_(0.1 * rn(D) + 0.5 * (1 + i % 3))
            blk.mlp.fc1.bias.copy_(0.1 * rn(blk.mlp.fc1.bias.numel()))
            blk.mlp.fc2.bias.copy_(0.1 * rn(D) - 0.5 * (1 + i % 2))
            blk.attn.proj.weight[big] *= 8.0
            blk.mlp.fc2.weight[big] *= 8.0
            if hasattr(blk, "skip_linear"):
                blk.skip_linear.bias.copy_(0.1 * rn(D) + 1.25)
                blk.skip_linear.weight[big] *= 4.0
            wq = blk.attn.qkv.weight                                   # rows [0, D): q, [D, 2D): k  ("(K H D)")
            r = slice(SINK_HEAD * 64, SINK_HEAD * 64 + 64)
            wq[r] *= 0.25
            wq[r][:, big] += 0.1 * e[:, None] * sign[None, :]
            rk = slice(D + SINK_HEAD * 64, D + SINK_HEAD * 64 + 64)
            wq[rk] *= 0.25
            wq[rk][:, sink] += 1.3 * e[:, None] * sign[None, :]
            wq[SHARP_HEAD * 64:SHARP_HEAD * 64 + 64] *= 4.0
        net.norm.weight.copy_(1.0 + 0.3 * rn(D))
        net.norm.bias.copy_(0.2 * rn(D))
        net.decoder_pred.bias.copy_(0.1 * rn(net.decoder_pred.bias.numel()))
        if t2i:
            net.context_embed.bias.copy_(0.1 * rn(D))
    return net


def state_dict(net):
    """The module's parameters as fp32 CPU tensors under the reference's keys."""
    return {k: v.detach().to("cpu", torch.float32) for k, v in net.state_dict().items()}
