"""Cases, data sets, the float64 model of the streamed arithmetic, the plan mirror and the bounds for the wide single-head attention
kernel (uspace_amd/csrc/attention_wide.hip); a helper of tests/test_attention_wide_cases.py (CPU) and tests/test_gpu_attention_wide.py
(GPU), not a test.  Follows tests/attention_long_cases.py."""
import math

import torch

KT = 32                          # keys per key tile
WIDTHS = (64, 128, 256, 512)     # every width uspace_groupnorm_map_bf16 accepts
CUS = 256


# ------------------------------------------------------------------------------------------------------------------ plan mirror
def plan(B, N, C):
    """Mirrors wide_plan of attention_wide.hip: (KT, QB, NW, grid, block, LDS bytes).  A wave owns 16 queries; a workgroup is the most
    waves (4, 2, 1) that still gives each of the 256 CUs a workgroup."""
    NW = 4 if B * -(-N // 64) >= CUS else 2 if B * -(-N // 32) >= CUS else 1
    QB = 16 * NW
    return KT, QB, NW, B * -(-N // QB), 64 * NW, 4 * KT * C * 2


def branch_batches(N):
    """The smallest B that takes NW = 1, 2 and 4 at N tokens (None where B = 1 already takes more waves)."""
    b2, b4 = -(-CUS // -(-N // 32)), -(-CUS // -(-N // 64))
    return {1: 1 if b2 > 1 else None, 2: b2 if b2 < b4 else None, 4: b4}


# ------------------------------------------------------------------------------------------------------------------ cases
# (B, N, C, data set, sampled query rows or None).  N: 1, KT - 1, KT, KT + 1, 2 KT - 1, 2 KT + 1 (one past the 64 queries of a 4-wave
# workgroup), 129 at every width with B = 3; 33 x 33, 40 x 40 and 1 025 tokens; one image of 64 x 64 tokens at the VAE's width, where
# the reference is computed on 256 sampled query rows.
SMALL_N = (1, 31, 32, 33, 63, 65, 129)
DATA_SETS = ("first", "last", "rand")
CASES = [(3, N, C, DATA_SETS[(i + j) % 3], None) for j, C in enumerate(WIDTHS) for i, N in enumerate(SMALL_N)]
CASES += [(2, 1089, 128, "last", None), (3, 1600, 256, "first", None), (2, 1025, 512, "last", None), (1, 4096, 512, "rand", 256)]


def case_id(case):
    B, N, C, data, rows = case
    return f"{B}x{N}x{C}-{data}" + (f"-{rows}rows" if rows else "")


def _bf(x):
    """Round to bf16 (RNE), back in the input's dtype."""
    return x.to(torch.float32).to(torch.bfloat16).to(x.dtype)


def _seed(B, N, C, data):
    return 1000003 * N + 7919 * C + 31 * B + DATA_SETS.index(data) if data in DATA_SETS else 17 * N + C + B


def make_qkv(B, N, C, data):
    """q, k, v as bf16 [B * N, C] and the scale C^-1/2.  k, v ~ N(0, 1) (v + 0.5: a wrong normaliser moves every channel one way);
    query i points at one key t(i): q = a k_t + 0.2 noise with a = (ln N + 1.5) / sqrt C, so the target's logit stands ln N + 1.5 above
    the others' N(0, a^2) and the peak probability is ~0.6 rather than the near-uniform 1 / N.
      'first'  t(i) in the first key tile: the running maximum never rises after it -- the no-rescale path
      'last'   t(i) in the last key tile (even rows: the LAST key, N - 1): the maximum rises at the end -- the rescale path
      'rand'   anywhere
      'constv' a set with an exact answer, for the row sum: every key but one per image has the same K row, so a query's P has two levels
               (the odd key's 1 and one common value that a bf16 rounding moves by up to 2^-8), and every V row of an image is the same
               vector u.  The answer is u, bit for bit, iff P.V and the row sum see the SAME rounded P."""
    g = torch.Generator().manual_seed(_seed(B, N, C, data))
    scale = C ** -0.5
    if data == "constv":
        kappa = torch.randn(B, 1, C, generator=g, dtype=torch.float64)
        kappa = _bf(kappa)
        t = torch.randint(0, N, (B,), generator=g)
        k = kappa.expand(B, N, C).clone()
        k[torch.arange(B), t] = 0.0
        d0 = math.log(max(N - 1, 1) / 2.3) if N > 3 else 0.5
        d = d0 + 0.7 * torch.rand(B, N, 1, generator=g, dtype=torch.float64)              # common logit = -d: peak > 0.3
        q = -d * kappa * (math.sqrt(C) / (kappa * kappa).sum(-1, keepdim=True))
        v = _bf(torch.randn(B, 1, C, generator=g, dtype=torch.float64) + 0.5).expand(B, N, C)
    else:
        k = torch.randn(B, N, C, generator=g, dtype=torch.float64)
        v = torch.randn(B, N, C, generator=g, dtype=torch.float64) + 0.5
        last0 = KT * ((N - 1) // KT)
        if data == "first":
            t = torch.randint(0, min(N, KT), (B, N), generator=g)
        elif data == "last":
            t = torch.randint(last0, N, (B, N), generator=g)
            t[:, 0::2] = N - 1
        else:
            t = torch.randint(0, N, (B, N), generator=g)
        a = (math.log(N) + 1.5) / math.sqrt(C)
        q = a * torch.gather(k, 1, t[..., None].expand(B, N, C)) + 0.2 * torch.randn(B, N, C, generator=g, dtype=torch.float64)
    to = lambda x: x.reshape(B * N, C).to(torch.float32).to(torch.bfloat16).contiguous()
    return to(q), to(k), to(v), scale


PAD = 16                 # ld = C + PAD elements, the padding filled with NaN
CANARY_ROWS = 4
CANARY = 0x4b4b          # bf16 13 303 808: never a result


def _padded(x, ld):
    """bf16 [rows, C] -> device buffer [rows, ld] with NaN behind column C."""
    buf = torch.full((x.shape[0], ld), float("nan"), dtype=torch.bfloat16)
    buf[:, : x.shape[1]] = x
    return buf.cuda()


def run(q, k, v, B, N, C, scale, pad=PAD):
    """The kernel on host operands -> out bf16 [B * N, C] on the host (needs the GPU).  Operands with leading dimension C + pad and NaN
    padding; ``out`` with the same padding and CANARY_ROWS more rows, all pre-filled with CANARY: whatever the kernel does not own must
    still hold it."""
    from uspace_amd import _hip
    ld = C + pad
    dq, dk, dv = (_padded(x, ld) for x in (q, k, v))
    out = torch.full((B * N + CANARY_ROWS, ld), CANARY, dtype=torch.int16).cuda()
    _hip.attention_wide(dq, dk, dv, B, N, C, scale, ld=ld, out=out, ld_out=ld)
    torch.cuda.synchronize()
    o = out.cpu()
    assert bool((o[B * N:] == CANARY).all()), "rows behind out were written"
    assert bool((o[:, C:] == CANARY).all()), "columns behind C were written"
    return o[: B * N, :C].contiguous().view(torch.bfloat16)


def sample_rows(N, n, seed=5):
    """n distinct query rows of N, the first and the last among them, sorted."""
    g = torch.Generator().manual_seed(seed)
    idx = torch.randperm(N, generator=g)[:n]
    idx[0], idx[1] = 0, N - 1
    return torch.unique(idx)


def _d(x, B, N, C):
    return x.to(torch.float64).reshape(B, N, C)


# ------------------------------------------------------------------------------------------------------------------ references
def reference(q, k, v, B, N, C, scale, rows=None):
    """Plain float64 softmax(q k^T scale) v on the bf16 operands, unrounded: [B, n_rows, C]; also the largest probability per row."""
    q, k, v = _d(q, B, N, C), _d(k, B, N, C), _d(v, B, N, C)
    if rows is not None:
        q = q[:, rows]
    p = torch.softmax(q @ k.transpose(1, 2) * scale, dim=-1)
    return p @ v, p.amax(-1)


FAULTS = ("mask_late", "rescale_dropped", "unrounded_sum", "v_neighbour")


def streamed(q, k, v, B, N, C, scale, rows=None, fault=None, kt=KT, rnd=True):
    """The kernel's algorithm in float64, written from its description: keys in tiles of ``kt``; per tile the running row maximum m
    rises to m', the accumulated O and row sum l are multiplied by exp(m - m'), P = exp(s - m') is rounded to bf16 ONCE and that rounded
    P feeds both P.V and l; O / l at the end, rounded to bf16.  [B, n_rows, C].  ``fault`` plants one of FAULTS:
      mask_late        the mask starts one key late: key N (the LDS row behind the last key, a copy of row N - 1) takes part
      rescale_dropped  O is not rescaled when the maximum rises (l is)
      unrounded_sum    l sums the un-rounded P
      v_neighbour      V is read from the next image"""
    assert fault is None or fault in FAULTS
    q, k, v = _d(q, B, N, C), _d(k, B, N, C), _d(v, B, N, C)
    if rows is not None:
        q = q[:, rows]
    if fault == "v_neighbour":
        v = torch.roll(v, -1, 0)
    if fault == "mask_late" and N % kt:
        k, v = torch.cat([k, k[:, -1:]], 1), torch.cat([v, v[:, -1:]], 1)
    r = (lambda x: _bf(x)) if rnd else (lambda x: x)
    n = q.shape[1]
    m = torch.full((B, n, 1), -float("inf"), dtype=torch.float64)
    o = torch.zeros(B, n, C, dtype=torch.float64)
    l = torch.zeros(B, n, 1, dtype=torch.float64)
    for k0 in range(0, N, kt):
        k1 = min(k0 + kt, k.shape[1])
        sj = q @ k[:, k0:k1].transpose(1, 2) * scale
        m_new = torch.maximum(m, sj.amax(-1, keepdim=True))
        alpha = torch.exp(m - m_new)
        p = torch.exp(sj - m_new)
        pu = r(p)
        o = (o if fault == "rescale_dropped" else o * alpha) + pu @ v[:, k0:k1]
        l = l * alpha + (p if fault == "unrounded_sum" else pu).sum(-1, keepdim=True)
        m = m_new
    return r(o / l)


# ------------------------------------------------------------------------------------------------------------------ metrics
def rel_l2(got, ref):
    return float((got - ref).norm() / ref.norm())


def max_abs(got, ref, v, B, N, C):
    """max over elements of |got - ref| / max_j |v[b, j, c]|: the unit of the analytic ceiling."""
    vmax = _d(v, B, N, C).abs().amax(1, keepdim=True)
    return float(((got - ref).abs() / vmax).max())


# ------------------------------------------------------------------------------------------------------------------ bounds
# Against the PLAIN float64 softmax on the same bf16 operands, per width C, over every case of that width:
#   rel     rel-L2 over the whole output
#   maxabs  max |err| / max_j |v_j| per (image, channel)
# Each is 3 x what an MI355X measured (GPU_MEASURED, the project's convention), and maxabs never above the analytic ceiling
# CEILING = 2^-8, the ceiling the kernel was specified with: one bf16 rounding of P, then one of the output, counted as 2^-9 of
# max|v| each.  The measured worst case uses 0.90 of it.  A measurement that needs more is a bug, not a reason to widen.
# The 'constv' set has an exact answer and its own bound, 0: O = u sum(P~) and l = sum(P~) hold the same fp32 sum up to (N + tiles)
# roundings of 2^-24, 65 + 3 of them at the test's N = 65, four orders below the half-ulp (>= 2^-9 relative) that would move the bf16
# result off u.
CEILING = 2.0 ** -8
MARGIN = 3.0
GPU_MEASURED = {
    # C: (rel-L2, maxabs / max|v|) -- worst case of that width on an MI355X (tests/test_gpu_attention_wide.py prints them).  They are
    # the float64 model's own figures to the digits shown (tests/test_attention_wide_cases.py prints those): the kernel's fp32 logits
    # moved no rounding that matters.  rel-L2 is the bf16 rounding of the output, 2^-9 / sqrt 3 on average plus a little from P.
    64: (1.692e-3, 3.334e-3),       # 3x32x64 rand / 3x31x64 last        -> bounds 5.08e-3, 2^-8 (3 x 3.334e-3 = 1.0e-2 is above the ceiling)
    128: (1.725e-3, 3.380e-3),      # 3x129x128 last / 3x32x128 first    -> bounds 5.18e-3, 2^-8
    256: (1.675e-3, 3.473e-3),      # 3x33x256 rand (both)               -> bounds 5.03e-3, 2^-8
    512: (1.664e-3, 3.500e-3),      # 3x32x512 rand / 3x65x512 rand      -> bounds 4.99e-3, 2^-8
}


def bounds(C):
    rel, ma = GPU_MEASURED[C]
    return MARGIN * rel, min(MARGIN * ma, CEILING)
