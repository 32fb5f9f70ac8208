"""Cases, the float64 model of the streamed arithmetic, the plan mirror and the bounds for the long-sequence attention kernel
(uspace_amd/csrc/attention_long.hip); a helper of tests/test_attention_long_cases.py (CPU) and tests/test_gpu_attention_long.py (GPU),
not a test.  Data sets, metrics, the envelope and the faulty references are those of tests/attention_cases.py."""
import torch

from tests import attention_cases as AC
from tests.uvit_stages import _bf, _d

KT = 64                     # keys per key tile
NW = 4                      # waves per workgroup
RESIDENT_MAX_L = 336        # uspace_attention_bf16 stops here


# ------------------------------------------------------------------------------------------------------------------ plan mirror
def plan(B, L, H, scaled):
    """Mirrors long_plan of attention_long.hip: (KT, QB, NW, grid, block, LDS bytes).  QB = 128 queries per workgroup once that still
    gives each of the 256 CUs two workgroups, 64 below."""
    BH = B * H
    QB = 128 if BH * -(-L // 128) >= 512 else 64
    return KT, QB, NW, BH * -(-L // QB), 64 * NW, 4 * KT * 128 + (2 * KT * 4 if scaled else 0)


def switch_bh(L):
    """The smallest B * H that takes QB = 128 at length L."""
    return -(-512 // -(-L // 128))


# ------------------------------------------------------------------------------------------------------------------ cases
# (B, L, H, scaled, data set).  L: 1, 17, 334, 336 (shared with the resident kernel), 337 (the first length only this kernel takes),
# 6 KT - 1 / 6 KT / 6 KT + 1, QB + 1 for both QB (65, 129), 1 025 / 1 102 (64 x 64 latents, unconditional / T2I) and 2 049; B * H on
# both sides of the plan's one switch at L = 17 (511 / 512), 129 (255 / 256) and 337 (170 / 171), and beyond it at 385 (8 x 16).
# The lengths above 385 keep B <= 2 and H <= 2.  Every key_scale case has B >= 2: its last sample's scales are all 0.
CASES = [
    (1, 1, 1, False, "workflow"), (2, 1, 2, True, "flat"),
    (3, 17, 2, False, "sharp"), (2, 17, 2, True, "workflow"), (511, 17, 1, False, "flat"), (512, 17, 1, True, "flat"),
    (2, 65, 2, False, "edges"), (3, 129, 1, True, "edges"), (255, 129, 1, False, "flat"), (256, 129, 1, False, "voff"),
    (2, 334, 2, False, "edges"), (2, 334, 3, True, "workflow"), (2, 336, 2, False, "flat"), (3, 336, 1, True, "edges"),
    (2, 337, 2, False, "edges"), (3, 337, 1, True, "flat"), (170, 337, 1, False, "flat"), (171, 337, 1, True, "sharp"),
    (171, 337, 1, False, "edges"),
    (2, 383, 2, False, "flat"), (2, 384, 2, True, "edges"), (2, 385, 2, False, "sharp"), (8, 385, 16, False, "edges"),
    (8, 385, 16, True, "voff"),
    (2, 1025, 2, False, "edges"), (2, 1025, 1, True, "flat"), (1, 1025, 2, False, "workflow"),
    (2, 1102, 2, True, "edges"), (1, 1102, 2, False, "sharp"), (2, 1102, 1, False, "voff"),
    (1, 2049, 2, False, "edges"), (2, 2049, 1, True, "workflow"), (1, 2049, 1, False, "flat"),
]
REQUIRED_L = (1, 17, 334, 336, 337, 6 * KT - 1, 6 * KT, 6 * KT + 1, 64 + 1, 128 + 1, 1025, 1102, 2049)
SHARED_L = (17, 334, 336)           # both kernels run these cases and meet the same bounds


# ------------------------------------------------------------------------------------------------------------------ streamed model
def streamed_attention(qkv, H, rnd=True, key_scale=None, kt=KT, rescale_dropped=False):
    """The kernel's algorithm in float64, written from its description: keys in tiles of ``kt``; per tile the running row maximum m
    rises to m', the accumulated O and row sum l are multiplied by exp(m - m'), P = exp(s - m') is rounded to bf16 (``rnd``) ONCE and
    that rounded P feeds both P.V and l (under key_scale: bf16(P ks) feeds P.V, bf16(P) feeds l); O / l at the end, rounded to bf16.
    Same signature as uvit_stages.attention.  ``rescale_dropped``: the fault of an O that is not rescaled when the maximum rises."""
    B, L, _ = qkv.shape
    q, k, v = _d(qkv).reshape(B, L, 3, H, 64).permute(2, 0, 3, 1, 4)
    s = q @ k.transpose(-1, -2) / 8.0
    ks = None if key_scale is None else _d(key_scale)[:, None, None, :]
    m = torch.full((B, H, L, 1), -float("inf"), dtype=torch.float64)
    o = torch.zeros(B, H, L, 64, dtype=torch.float64)
    l = torch.zeros(B, H, L, 1, dtype=torch.float64)
    for k0 in range(0, L, kt):
        sj = s[..., k0:k0 + kt]
        m_new = torch.maximum(m, sj.amax(-1, keepdim=True))
        alpha = torch.exp(m - m_new)
        p = torch.exp(sj - m_new)
        pu = _bf(p, rnd)
        pv = pu if ks is None else _bf(p * ks[..., k0:k0 + kt], rnd)
        o = (o if rescale_dropped else o * alpha) + pv @ v[:, :, k0:k0 + kt]
        l = l * alpha + pu.sum(-1, keepdim=True)
        m = m_new
    return _bf((o / l).transpose(1, 2).reshape(B, L, H * 64), rnd)


def rescale_dropped(qkv, H, rnd, key_scale=None):
    return streamed_attention(qkv, H, rnd, key_scale, rescale_dropped=True)


# fault -> (function, needs key_scale, data sets for the rel-L2 bounds, for the envelope, for every bound under key_scale): those of
# attention_cases.PERTURBED, and the one fault only a streaming kernel can have.  'edges' rows whose dominant key is L - 1 meet their
# maximum in the last key tile, 'sharp' / 'workflow' rows wherever it falls.
PERTURBED = dict(AC.PERTURBED, rescale_dropped=(rescale_dropped, False, ("edges", "sharp", "workflow"), ("edges", "sharp"), ("edges", "sharp")))


# ------------------------------------------------------------------------------------------------------------------ bounds
# The GPU test compares with the PLAIN float64 softmax (uvit_stages.attention, no rounding), per head and per query row:
#   head   attention_cases.TOL["att_loose"] / ["att_loose_ks"]: the project's bound of the resident kernel against the same reference
#   env    |got - ref| <= env_k 2^-8 |ref| + env_a envelope_a: analytic (attention_cases.envelope_a: every P a whole bf16 ulp off, whatever
#          it is relative to -- a tile's maximum or the row's), so it holds against the unrounded reference as well
#   row    3 x ROW_MODEL: the worst query row of the streamed MODEL above against plain float64, measured on the CPU over CASES by
#          tests/test_attention_long_cases.py (which fails if a case exceeds the entry); 3 x is the margin of attention_cases.TOL
ROW_MODEL = dict(
    plain=3.21e-3,      # measured 3.200e-3 (2x1025x2 edges)
    ks=5.06e-3,         # measured 5.054e-3 (2x1102x2 edges; 5.02e-3 at 171x337x1 sharp)
)
ROW_MARGIN = 3.0
# what an MI355X measured over CASES (worst case beside each): head / row rel-L2 against plain float64, share of the envelope used
GPU_MEASURED = dict(
    head=2.43e-3,       # bound att_loose 7.4e-3: measured 2.429e-3 (170x337x1 flat)
    head_ks=3.06e-3,    # bound att_loose_ks 1.3e-2: measured 3.052e-3 (512x17x1 flat)
    row=3.20e-3,        # bound 3 x ROW_MODEL = 9.63e-3: measured 3.200e-3 (2x1025x2 edges) -- the model's own figure: the kernel's fp32
                        # logits move no rounding of P on that case
    row_ks=5.06e-3,     # bound 1.52e-2: measured 5.054e-3 (2x1102x2 edges)
    env=0.221,          # bound 1: measured 0.220 of the envelope used (1x1102x2 sharp)
    env_ks=0.325,       # bound 1: measured 0.325 (171x337x1 sharp)
)


def row_bound(scaled):
    return ROW_MARGIN * ROW_MODEL["ks" if scaled else "plain"]
