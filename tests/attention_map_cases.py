"""Cases, float64 reference, metrics and perturbed references for the head-mean attention-map kernel
(uspace_amd/csrc/attention_map.hip); a helper of tests/test_attention_map_host.py (CPU) and tests/test_gpu_attention_map.py (GPU),
not a test.

``reference`` is the map from the packed bf16 qkv in float64, ``CASES`` the (B, L, H, window, data set) list of the GPU test (data sets:
``tests.attention_cases.make_qkv``), ``PERTURBED`` holds ``reference`` with one fault each -- what a subtly wrong kernel or call would
compute -- and ``TOL`` the bounds.  The CPU test shows that every bound separates each fault from the true reference."""
import numpy as np
import torch

from tests.attention_cases import DH, make_key_scale, make_qkv  # noqa: F401  (re-exported: the tests build their data with them)

N_CTX = 77          # T2I token order: time (1), context (77), image


# ------------------------------------------------------------------------------------------------------------------ windows
def window(name, L):
    """(q0, nq, k0, nk) of a named window at sequence length L.
      full  the whole L x L map (every row sums to 1)
      ic    image x context of the T2I layout (what vis_attention_map draws); needs L > 78
      ii    image x image (the input of tools/attention_vis.py show_self_attention_comp)
      odd   nq and nk no multiples of 16, neither edge on a tile boundary
      k1    one key column, the last one (nk = 1)
      q1    one query row in the middle (nq = 1)"""
    if name == "full":
        return 0, L, 0, L
    if name == "ic":
        return 1 + N_CTX, L - 1 - N_CTX, 1, N_CTX
    if name == "ii":
        return 1 + N_CTX, L - 1 - N_CTX, 1 + N_CTX, L - 1 - N_CTX
    if name == "odd":
        return 3, min(L - 3, 37), 5, min(L - 5, 21)
    if name == "k1":
        return 0, L, L - 1, 1
    if name == "q1":
        return L // 2, 1, 0, L
    raise ValueError(name)


# (B, L, H, window, data set).  L in {1, 17, 142, 257, 300, 334, 336} (one tile, one key into the second tile, the tiny T2I length, the
# two production lengths, a ragged one and the largest), H in {1, 8, 16}, every window at the T2I lengths, and B on both sides of one
# wave of workgroups: the L = 334 kernel keeps one wave per SIMD (1024 workgroups on 256 CUs), the full window has 21 query tiles per
# sample: 48 x 21 = 1008, 50 x 21 = 1050.
CASES = [
    (1, 1, 1, "full", "workflow"), (2, 1, 8, "full", "flat"),
    (3, 17, 1, "full", "flat"), (2, 17, 8, "odd", "workflow"), (2, 17, 16, "k1", "edges"),
    (3, 142, 1, "ic", "workflow"), (2, 142, 8, "ii", "flat"), (2, 142, 16, "full", "sharp"), (3, 142, 8, "ic", "edges"),
    (2, 142, 8, "ic", "flat"),
    (2, 257, 16, "full", "flat"), (2, 257, 8, "odd", "sharp"), (1, 257, 1, "k1", "workflow"),
    (2, 300, 8, "full", "edges"), (2, 300, 16, "odd", "flat"),
    (10, 334, 16, "ic", "workflow"), (2, 334, 8, "ii", "flat"), (2, 334, 16, "full", "sharp"), (48, 334, 1, "full", "flat"),
    (50, 334, 2, "full", "workflow"), (2, 334, 8, "k1", "edges"), (2, 334, 8, "q1", "flat"), (3, 334, 16, "ic", "flat"),
    (2, 336, 16, "full", "flat"), (2, 336, 1, "odd", "edges"), (3, 336, 8, "ic", "sharp"),
]
REQUIRED_L = (1, 17, 142, 257, 300, 334, 336)
REQUIRED_H = (1, 8, 16)
REQUIRED_WINDOWS = ("full", "ic", "ii", "odd", "k1")


def case_id(case):
    B, L, H, win, data = case
    return f"{B}x{L}x{H}-{win}-{data}"


# ------------------------------------------------------------------------------------------------------------------ reference
def _probs(qkv, H, dtype=torch.float64, keys=None, extra_last=0):
    """softmax(q k^T / 8) per head, [B, H, L, L'] in ``dtype``; ``keys`` = (first, count) restricts the softmax to those keys,
    ``extra_last`` appends that many copies of key L - 1."""
    B, L, _ = qkv.shape
    x = qkv.to(dtype).reshape(B, L, 3, H, DH)
    q, k = x[:, :, 0].permute(0, 2, 1, 3), x[:, :, 1].permute(0, 2, 1, 3)
    if extra_last:
        k = torch.cat([k] + [k[:, :, L - 1:]] * extra_last, 2)
    if keys is not None:
        k = k[:, :, keys[0]:keys[0] + keys[1]]
    s = q @ k.transpose(-1, -2) / 8.0
    p = torch.exp(s - s.amax(-1, keepdim=True))
    return p / p.sum(-1, keepdim=True)


def reference(qkv, H, win, key_scale=None, dtype=torch.float64):
    """out[b, i, j] = mean_h softmax_k(q[b, h, q0 + i] . k[b, h, k] / 8)[k0 + j] from the packed bf16 qkv [B, L, 3 H 64], the softmax
    over all L keys; [B, nq, nk] in float64.  ``key_scale`` is accepted and ignored: the map is the one before the edit."""
    q0, nq, k0, nk = win
    return _probs(qkv, H, dtype).mean(1)[:, q0:q0 + nq, k0:k0 + nk].to(torch.float64)


# ------------------------------------------------------------------------------------------------------------------ metrics
def _worst(num, den):
    r = num / np.maximum(den, 1e-300)
    r = np.where(np.isnan(r), np.inf, r)          # a NaN output is as wrong as an output gets
    return float(r.max()) if r.size else 0.0


def row_err(got, ref):
    """Worst rel-L2 over (sample, query row); got, ref [B, nq, nk]."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return _worst(np.sqrt(((got - ref) ** 2).sum(2)), np.sqrt((ref ** 2).sum(2)))


ELEM_FLOOR = 1e-20      # entries below it (fp32 flushes the smallest to 0) are held absolutely


def elem_err(got, ref):
    """max |got - ref| / (|ref| + ELEM_FLOOR): the element-wise relative error."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return _worst(np.abs(got - ref), np.abs(ref) + ELEM_FLOOR)


def block_err(got, ref):
    """rel-L2 per sample of one block's map, worst sample; got, ref [B, nq, nk]."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return _worst(np.sqrt(((got - ref) ** 2).sum((1, 2))), np.sqrt((ref ** 2).sum((1, 2))))


# ------------------------------------------------------------------------------------------------------------------ faults
def head_sum(qkv, H, win, key_scale=None):
    """The heads summed, the 1 / H forgotten."""
    return reference(qkv, H, win) * H


def window_shifted(qkv, H, win, key_scale=None):
    """The key window one column early: with the image x context window the time token leaks in."""
    q0, nq, k0, nk = win
    return reference(qkv, H, (q0, nq, k0 - 1, nk))


def window_softmax(qkv, H, win, key_scale=None):
    """The softmax normalised over the window's keys instead of all L."""
    q0, nq, k0, nk = win
    return _probs(qkv, H, keys=(k0, nk)).mean(1)[:, q0:q0 + nq]


def last_key_masked(qkv, H, win, key_scale=None):
    """Key L - 1 invisible (a mask off by one): its column is 0, the others share its weight."""
    q0, nq, k0, nk = win
    L = qkv.shape[1]
    p = _probs(qkv, H, keys=(0, L - 1)).mean(1)
    p = torch.cat([p, torch.zeros_like(p[:, :, :1])], 2)
    return p[:, q0:q0 + nq, k0:k0 + nk]


def pad_key_visible(qkv, H, win, key_scale=None):
    """One padding key visible: the kernel reads row L - 1 again behind L, so a leak counts that key twice in the row sum."""
    q0, nq, k0, nk = win
    return _probs(qkv, H, extra_last=1).mean(1)[:, q0:q0 + nq, k0:k0 + nk]


def key_scale_applied(qkv, H, win, key_scale=None):
    """The p2p column factors applied to the map (the reference shows the map BEFORE the edit)."""
    q0, nq, k0, nk = win
    return reference(qkv, H, win) * key_scale.to(torch.float64)[:, None, k0:k0 + nk]


def next_sample_heads(qkv, H, win, key_scale=None):
    """Every sample shows the heads of the next one (a wrong batch stride)."""
    return torch.roll(reference(qkv, H, win), -1, dims=0)


# fault -> (function, data sets meant to expose it, what a case must offer).  'flat' (P near-uniform, every key 1 / L of every row) is
# the set that sees a wrong normalisation or mask; 'workflow' / 'sharp' rows differ from sample to sample and column to column.
PERTURBED = dict(
    head_sum=(head_sum, ("flat", "workflow", "sharp", "edges"), lambda B, L, H, w: H > 1),
    window_shifted=(window_shifted, ("workflow", "sharp", "flat"), lambda B, L, H, w: w[2] >= 1),
    window_softmax=(window_softmax, ("flat", "workflow", "sharp", "edges"), lambda B, L, H, w: w[3] < L),
    last_key_masked=(last_key_masked, ("flat", "edges"), lambda B, L, H, w: L >= 2),
    pad_key_visible=(pad_key_visible, ("flat", "edges"), lambda B, L, H, w: True),
    key_scale_applied=(key_scale_applied, ("flat", "workflow", "sharp", "edges"), lambda B, L, H, w: True),
    next_sample_heads=(next_sample_heads, ("workflow", "sharp"), lambda B, L, H, w: B >= 2),
)


def fault_key_scale(B, L, win):
    """Column factors for key_scale_applied: the p2p multiplier 3 on two columns of the window (its first and last), 1 elsewhere."""
    ks = torch.ones(B, L)
    ks[:, win[2]] = 3.0
    ks[:, win[2] + win[3] - 1] = 3.0
    return ks


# ------------------------------------------------------------------------------------------------------------------ GPU test bounds
# Each bound is 3x the worst value an MI355X measured (beside it, with the case), the convention of tests/attention_cases.py:TOL.
# Kernel bounds: against ``reference`` over CASES.  What the kernel adds to float64 is the fp32 accumulation of the logits, the fp32
# exponent argument s c - max c (half an ulp at a magnitude of tens) and the fp32 sums: parts in 1e6, far from the smallest fault
# (one key's share of a flat row, 1 / 336 = 3e-3).
TOL = dict(
    map_row=8.2e-6,      # measured 2.73e-6 (2x336x1-odd-edges; 2.0e-6 at 3x336x8-ic-sharp, <= 1.3e-7 on 'flat'): worst (sample, query row) rel-L2
    map_elem=2.1e-5,     # measured 6.90e-6 (2x334x16-full-sharp; 5.2e-6 at 2x142x16-full-sharp): worst element, relative (elem_err)
    # Model bounds: rel-L2 per (block, sample).  What they hold is the distance between two bf16 qkv tensors that agree up to rounding
    # flips (GPU fp32 accumulation against float64), resp. between bf16 operands and the reference's fp32: parts in 1e4, growing
    # with depth.
    model_qkv=3.1e-4,    # measured 1.04e-4 (stress D=128 block 4, folded; 6.7e-5 separate; 3.4e-5 tiny block 2): forward_maps against the
                         # map kernel on the float64 stage model's qkv
    ref_tiny=4.6e-4,     # measured 1.55e-4 (tiny_edit block 2; 1.22e-4 block 0): against the reference's own attn tensor, tiny T2I
    ref_S=1.5e-3,        # measured 5.02e-4 (S_edit block 16; 3.5e-4 block 0): ... U-ViT-S T2I
    # Arg-max image token per text token.  Two maps that agree to within e can only pick different tokens where the reference's top-1
    # leads its top-2 by less than 2 e, so exact equality is demanded where the lead is clear and a near-tie rule elsewhere: where
    # the reference's relative lead is at least argmax_lead the pick must be the reference's; elsewhere it must be a token the
    # reference holds within argmax_lead of its top.  The threshold follows the 3x convention: the worst share of the top a differing
    # pick gave up measured 5.18e-4 (tiny_edit block 2; 1-3 of the 231 (sample, token) pairs per block differ, every one a near-tie).
    argmax_lead=1.6e-3,
)
