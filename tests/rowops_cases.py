"""The calls whose raw output bytes pin the row and elementwise kernels of uspace_amd/csrc/rowops.hip bit for bit (a helper, not a
test): every exported entry point of that file on shapes that reach every kernel form and every rung of the per-row register ladder,
the per-token fallbacks of the embed and the head and the general 3x3 conv among them.  Shared by tests/golden/make_rowops_digests.py
(which records the sha256 of every output buffer) and tests/test_gpu_rowops_bits.py (which compares).  None of these kernels uses
atomics: every call is run-to-run bit-equal, and a change of rowops.hip that keeps the order of every sum leaves every digest as it is.
Inputs are numpy-seeded per call; nothing is read from outside the repository."""
import ctypes
import itertools
import os
import zlib

import numpy as np
import torch

from tests.util import bf16_round, to_dev
from tests.vit_tower_cases import digest

HERE = os.path.dirname(os.path.abspath(__file__))
DIGESTS = os.path.join(HERE, "golden", "rowops_digests.json")

# rows: one full block of four and one partial block; widths: one per NV rung (1, 2, 4, 8, 16 float4 per lane), the middle three with
# a masked last chunk; row 2 holds one value (variance 0)
ROW_M = 5
ROW_D = (64, 320, 768, 1536, 4096)

# uspace_embed_tokens: (B, D, n_extra, time_first, S, p, C, bf16 copy).  The four sets of test_embed_tokens_matches_oracle, then
# B = 33 (embed_patch16_kernel<16>; the smaller batches take <4>), 9 patches (per-token kernel, 16-byte weight loads), 12 pixels,
# 3 pixels (scalar weight loop), each with n_extra 0 and 2, both token orders, with and without the bf16 copy.
EMBED_OLD = ((3, 128, 0, 1), (2, 512, 1, 0), (2, 1024, 77, 1), (2, 64, 0, 1))
EMBED_NEW_SHAPES = ((33, 64, 32, 2, 4), (3, 136, 6, 2, 4), (2, 64, 8, 2, 3), (2, 1028, 4, 1, 3))       # (B, D, S, p, C)
EMBED_CALLS = tuple(c + (32, 2, 4, True) for c in EMBED_OLD) + tuple(
    (B, D, ne, tf, S, p, C, bf) for (B, D, S, p, C) in EMBED_NEW_SHAPES for ne, tf, bf in itertools.product((0, 2), (1, 0), (True, False)))

# uspace_output_head: (B, D, extras, S, p, C).  The five sets of test_output_head_matches_oracle (the matrix-core kernel), the per-token
# kernel at NV 1, 2 and 8 (D % 32 != 0; 27 tokens: a partial last block), and 3 channels (PD = 12: the general conv).
HEAD_CALLS = tuple(c + (32, 2, 4) for c in ((3, 128, 1), (2, 512, 78), (5, 1024, 1), (2, 64, 2), (1, 1536, 1))) + (
    (3, 72, 1, 6, 2, 4), (3, 264, 2, 6, 2, 4), (3, 1028, 1, 6, 2, 4), (2, 128, 2, 8, 2, 3))


def rng_for(call):
    return np.random.default_rng(zlib.crc32(call.encode()))


def rand(rng, *shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(np.float32)


def _ok(rc, what):
    assert rc == 0, (what, rc)


def _api():
    from uspace_amd import _hip
    return _hip, _hip.lib(), _hip.ptr, _hip.stream_ptr()


def row_inputs(D):
    rng = rng_for(f"rows-{D}")
    x = rand(rng, ROW_M, D, scale=3.0) + 0.7
    x[2] = 1.25
    return x, rand(rng, D) + 1.0, rand(rng, D)


def row_outputs():
    _hip, L, P, s = _api()
    for D in ROW_D:
        x, g, b = (to_dev(a) for a in row_inputs(D))
        y = torch.empty(ROW_M, D, dtype=torch.bfloat16, device="cuda")
        _ok(L.uspace_layernorm_f32_bf16(P(x), P(g), P(b), P(y), ROW_M, D, 1e-5, s), "layernorm_f32_bf16")
        yield f"layernorm_f32_bf16-D{D}/y", y
        yf = torch.empty(ROW_M, D, device="cuda")
        _ok(L.uspace_layernorm_f32(P(x), P(g), P(b), P(yf), ROW_M, D, 1e-5, s), "layernorm_f32")
        yield f"layernorm_f32-D{D}/y", yf
        xc = torch.empty(ROW_M, D, dtype=torch.bfloat16, device="cuda")
        c, part = torch.empty(ROW_M, device="cuda"), torch.empty(ROW_M, 2, device="cuda")
        _ok(L.uspace_center_rows(P(x), P(xc), P(c), P(part), ROW_M, D, s), "center_rows")
        yield f"center_rows-D{D}/xc", xc
        yield f"center_rows-D{D}/c", c
        yield f"center_rows-D{D}/part", part


def embed_inputs(B, D, n_extra, S, p, C):
    rng = rng_for(f"embed-{B}-{D}-{n_extra}-{S}-{p}-{C}")
    L_ = 1 + n_extra + (S // p) ** 2
    return dict(img=rand(rng, B, C, S, S), t=rng.uniform(0.05, 0.95, B).astype(np.float32), pw=rand(rng, D, C, p, p, scale=0.2),
                pb=rand(rng, D, scale=0.1), pos=rand(rng, L_, D, scale=0.02), extra=rand(rng, B, max(n_extra, 1), D))


def run_embed(a, B, D, n_extra, time_first, S, p, C, want_bf16=True):
    """uspace_embed_tokens on the host arrays of embed_inputs -> (tok fp32 [B, L, D], its bf16 copy or None)."""
    _hip, L, P, s = _api()
    L_ = 1 + n_extra + (S // p) ** 2
    d = {k: to_dev(v) for k, v in a.items()}
    tok = torch.empty(B, L_, D, device="cuda")
    tokb = torch.empty(B, L_, D, device="cuda", dtype=torch.bfloat16) if want_bf16 else None
    _ok(L.uspace_embed_tokens(P(d["img"]), P(d["t"]), 1, P(d["extra"]) if n_extra else None, n_extra, time_first, P(d["pw"]), P(d["pb"]),
                              P(d["pos"]), P(tok), P(tokb), B, C, S, p, D, s), "embed_tokens")
    return tok, tokb


def embed_outputs():
    for B, D, ne, tf, S, p, C, bf in EMBED_CALLS:
        tok, tokb = run_embed(embed_inputs(B, D, ne, S, p, C), B, D, ne, tf, S, p, C, bf)
        call = f"embed-B{B}-D{D}-e{ne}-tf{tf}-S{S}-p{p}-C{C}-{'bf' if bf else 'nobf'}"
        yield call + "/tok", tok
        if bf:
            yield call + "/tok_bf16", tokb


def head_inputs(B, D, extras, S, p, C):
    rng = rng_for(f"head-{B}-{D}-{extras}-{S}-{p}-{C}")
    L_ = extras + (S // p) ** 2
    return dict(x=(rand(rng, B, L_, D, scale=1.5) + 0.3).astype(np.float32), ng=rand(rng, D) * 0.2 + 1.0, nb=rand(rng, D, scale=0.1),
                dw=rand(rng, p * p * C, D, scale=0.05), db=rand(rng, p * p * C, scale=0.1), cw=rand(rng, C, C, 3, 3, scale=0.2),
                cb=rand(rng, C, scale=0.1))


def run_head(a, B, D, extras, S, p, C):
    """uspace_output_head on the host arrays of head_inputs -> (out [B, C, S, S], the unpatchified map before the conv)."""
    _hip, L, P, s = _api()
    d = {k: to_dev(v) for k, v in a.items()}
    scratch = torch.empty(B, C, S, S, device="cuda")
    out = torch.empty(B, C, S, S, device="cuda")
    _ok(L.uspace_output_head(P(d["x"]), extras + (S // p) ** 2, extras, P(d["ng"]), P(d["nb"]), P(d["dw"]), P(d["db"]), P(d["cw"]), P(d["cb"]),
                             P(scratch), P(out), B, C, S, p, D, 1e-5, s), "output_head")
    return out, scratch


def head_outputs():
    for B, D, extras, S, p, C in HEAD_CALLS:
        out, scratch = run_head(head_inputs(B, D, extras, S, p, C), B, D, extras, S, p, C)
        call = f"head-B{B}-D{D}-x{extras}-S{S}-p{p}-C{C}"
        yield call + "/out", out
        yield call + "/scratch", scratch


def elementwise_outputs():
    _hip, L, P, s = _api()
    # x[b] += scale * row_scale[b] * delta: the 4-wide and the scalar form, with and without row scales and the bf16 copy
    for per, rows, copy in itertools.product((256, 255), (False, True), (False, True)):
        rng = rng_for(f"add-{per}")
        x, d = to_dev(rand(rng, 3, per)), to_dev(rand(rng, per))
        rs = to_dev(np.array([0.5, -2.0, 0.0], np.float32)) if rows else None
        xb = torch.empty(3, per, dtype=torch.bfloat16, device="cuda") if copy else None
        _ok(L.uspace_add_broadcast_rows(P(x), P(xb), P(d), -1.5, P(rs), 3, per, s), "add_broadcast_rows")
        call = f"add_broadcast_rows-{per}-{'rows' if rows else 'norows'}"
        yield f"{call}-{'bf' if copy else 'nobf'}/x", x
        if copy:
            yield f"{call}-bf/x_bf16", xb
    v = to_dev(rand(rng_for("cast"), 1003))
    yield "cast_f32_bf16-1003/dst", _hip.cast_bf16(v)
    # c + s_b (c - u): 4-wide, scalar (per_sample % 4 != 0), scalar because `out` is not 16-byte aligned; row scales with a zero
    for per, shift, rows in ((256, 0, False), (256, 0, True), (255, 0, True), (256, 1, True)):
        pair = to_dev(rand(rng_for(f"cfg-{per}"), 6, per))
        rs = to_dev(np.array([1.5, 0.0, -0.25], np.float32)) if rows else None
        buf = torch.zeros(3 * per + 4, device="cuda")
        out = buf[shift:shift + 3 * per]
        assert out.data_ptr() % 16 == 4 * shift
        _ok(L.uspace_cfg_combine(P(pair), P(rs), 2.0, P(out), 3, per, s), "cfg_combine")
        yield f"cfg_combine-{per}-shift{shift}-{'rows' if rows else 'norows'}/out", out
    n = 4 * 4 * 8 * 8 + 3
    rng = rng_for("ode")
    y, y1 = to_dev(rand(rng, n)), to_dev(rand(rng, n))
    ks = [to_dev(rand(rng, n)) for _ in range(8)]
    cs = [0.3, -1.2, 0.0, 2.5, 1e-3, -0.7, 0.11, 0.9]
    for n_k in (0, 1, 8):
        yield f"ode_combine-k{n_k}/out", _hip.ode_combine(torch.empty(n, device="cuda"), y, ks[:n_k], cs[:n_k])
    scratch, res = torch.zeros(1024, device="cuda"), torch.empty(2, device="cuda")
    _hip.ode_error_norm(y, y1, ks[:7], cs[:7], 1e-3, 1e-4, scratch, res)
    yield "ode_error_norm-k7/result", res
    yield "ode_error_norm-k7/partials", scratch[:(n + 255) // 256]
    g = torch.from_numpy(bf16_round(rand(rng_for("gelu"), 1028, scale=2.0))).to("cuda", torch.bfloat16)
    _ok(L.uspace_quick_gelu_bf16(P(g), 1028, s), "quick_gelu_bf16")
    yield "quick_gelu_bf16-1028/x", g
    rng = rng_for("table")
    ids = torch.from_numpy(rng.integers(0, 11, (2, 5)).astype(np.int32)).cuda()
    tt, pt = to_dev(rand(rng, 11, 136)), to_dev(rand(rng, 5, 136))
    out = torch.empty(2, 5, 136, device="cuda")
    _ok(L.uspace_table_embed(P(ids), P(tt), P(pt), P(out), 2, 5, 136, 11, s), "table_embed")
    yield "table_embed-2x5x136/out", out
    rng = rng_for("direction")                                   # B = 17: two chunks of 16 samples
    feat = to_dev(rand(rng, 17, 260))
    attr = torch.from_numpy(rng.integers(-1, 2, (17, 3)).astype(np.int32)).cuda()
    pos, neg = to_dev(rand(rng, 3, 260)), to_dev(rand(rng, 3, 260))
    _ok(L.uspace_direction_accumulate(P(feat), P(attr), P(pos), P(neg), 17, 260, 3, s), "direction_accumulate")
    yield "direction_accumulate-17x260x3/pos", pos
    yield "direction_accumulate-17x260x3/neg", neg
    rng = rng_for("fold")
    W, gam, bet, bias = (to_dev(a) for a in (rand(rng, 5, 300, scale=0.1), rand(rng, 300) + 1.0, rand(rng, 300), rand(rng, 5)))
    for with_bias in (True, False):
        Wf = torch.empty(5, 300, dtype=torch.bfloat16, device="cuda")
        bo, cs_ = torch.empty(5, device="cuda"), torch.empty(5, device="cuda")
        _ok(L.uspace_fold_layernorm(P(W), P(gam), P(bet), P(bias) if with_bias else None, P(Wf), P(bo), P(cs_), 5, 300, s), "fold_layernorm")
        call = f"fold_layernorm-5x300-{'bias' if with_bias else 'nobias'}"
        yield call + "/Wf", Wf
        yield call + "/bias_out", bo
        yield call + "/colsum", cs_


# group -> generator of (call/buffer, output tensor)
CASES = {"rows": row_outputs, "embed": embed_outputs, "head": head_outputs, "elementwise": elementwise_outputs}


def case_digests(case):
    """{call/buffer: sha256} of one group's calls, computed on the GPU."""
    out = {call: digest(t) for call, t in CASES[case]()}
    torch.cuda.synchronize()
    return out
