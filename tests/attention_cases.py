"""Cases, data sets, metrics and perturbed references for the non-causal attention kernel (uspace_amd/csrc/attention.hip); a helper
of tests/test_attention_cases.py (CPU) and tests/test_gpu_attention_parity.py (GPU), not a test.

``launch_form`` / ``launch_branch`` mirror the host dispatch, ``CASES`` reaches every launch form it can take, the ``make_*``
functions produce seeded bf16-rounded inputs and ``key_scale`` sets, ``head_err`` / ``row_err`` / ``envelope_excess`` are the
metrics of the GPU test, and ``PERTURBED`` holds ``tests.uvit_stages.attention`` with one fault each: what a subtly wrong kernel
would compute.  The CPU test shows that every bound of the GPU test separates each of them from the true reference."""
import numpy as np
import torch

from tests.uvit_stages import attention

DH = 64
# (NT, LC) the kernel is instantiated for: NT 16-key tiles, LC the compile-time length (0 = any length up to 16 NT)
INSTANTIATIONS = ((6, 0), (10, 0), (17, 0), (21, 0), (17, 257), (21, 334))
BRANCHES = ("small", "two", "hpw2", "hpw4", "one")
DATA_SETS = ("workflow", "flat", "sharp", "voff", "edges")


# ------------------------------------------------------------------------------------------------------------------ dispatch
# Mirrors att_plan of attention.hip: L -> NT, LC; NT -> NW; key_scale -> SCALED; B * H -> QS, HPW and the grid.
# tests/test_attention_cases.py ties it to the built library: to its kernels and to uspace_attention_plan.
def _instantiation(L):
    nt = (L + 15) // 16
    if L == 257:
        return 17, 257
    if L == 334:
        return 21, 334
    for n in (6, 10, 17, 21):
        if nt <= n:
            return n, 0
    raise ValueError(f"L = {L}: longer than 336 tokens")


def launch_branch(B, L, H, scaled):
    """Which of the five launches of att_plan a call takes: 'small' (QS = ceil(NT / NW) workgroups per head), 'two' (QS = 2),
    'hpw2' / 'hpw4' (two / four heads per workgroup) or 'one' (one workgroup per head)."""
    NT, LC = _instantiation(L)
    NW = 8 if NT > 17 else 4
    BH = B * H
    if BH <= 64:
        return "small"
    if BH <= 128:
        return "two"
    if not scaled and NW == 8 and LC > 0:
        rounds = -(-BH // 256)
        if rounds == 2:
            return "hpw2"
        if rounds in (3, 4):
            return "hpw4"
    return "one"


def launch_form(B, L, H, scaled):
    """(NT, LC, NW, SCALED, QS, HPW): the template arguments of the attention_kernel instantiation a call launches."""
    NT, LC = _instantiation(L)
    NW = 8 if NT > 17 else 4
    br = launch_branch(B, L, H, scaled)
    QS = {"small": -(-NT // NW), "two": 2}.get(br, 1)
    HPW = {"hpw2": 2, "hpw4": 4}.get(br, 1)
    return NT, LC, NW, bool(scaled), QS, HPW


def launch_grid(B, L, H, scaled):
    """Workgroups of the launch; a workgroup of the several-heads forms owns heads g, g + grid, g + 2 grid, ... (< B * H)."""
    BH = B * H
    br = launch_branch(B, L, H, scaled)
    if br in ("small", "two"):
        return BH * launch_form(B, L, H, scaled)[4]
    if br == "hpw2":
        return -(-BH // 2)
    if br == "hpw4":
        return -(-BH // -(-BH // 256))
    return BH


def all_launches():
    """Every (NT, LC, scaled, branch) att_plan can take: 38.  They are 36 distinct kernels: with NT = 6 on four waves
    ceil(NT / NW) is 2, so 'small' and 'two' launch the same instantiation."""
    out = []
    for NT, LC in INSTANTIATIONS:
        for scaled in (False, True):
            for br in BRANCHES:
                if br in ("hpw2", "hpw4") and (scaled or (NT, LC) != (21, 334)):
                    continue
                out.append((NT, LC, scaled, br))
    return out


def all_forms():
    """The set of launch_form values over every launch: the kernels the library must hold."""
    forms = set()
    for NT, LC, scaled, br in all_launches():
        NW = 8 if NT > 17 else 4
        forms.add((NT, LC, NW, scaled, {"small": -(-NT // NW), "two": 2}.get(br, 1), {"hpw2": 2, "hpw4": 4}.get(br, 1)))
    return forms


def case_launch(case):
    B, L, H, scaled, _ = case
    NT, LC = _instantiation(L)
    return NT, LC, bool(scaled), launch_branch(B, L, H, scaled)


# (B, L, H, scaled, data set).  Every launch of all_launches(); B * H on both sides of every switch of att_plan at L = 334 (64 / 65,
# 128 / 129, 256 / 257, 512 / 513, 768 / 769, 1024 / 1040; H = 1 gives any product); several-heads launches whose last workgroups own
# fewer heads than the others ((257, 334, 1), (513, 334, 1), (37, 334, 16)); L on both sides of every tile count the dispatch switches
# at and at exact tile multiples.  'flat' is the most frequent set: it is the one that sees a wrong mask or row sum.
CASES = [
    # (6, 0): L <= 96
    (1, 1, 1, False, "workflow"), (2, 2, 1, False, "flat"), (3, 15, 2, False, "flat"), (2, 16, 3, False, "edges"),
    (1, 17, 1, False, "sharp"), (4, 96, 16, False, "flat"), (2, 17, 2, True, "workflow"), (3, 16, 1, True, "flat"),
    (5, 96, 16, False, "voff"), (65, 15, 1, True, "flat"), (9, 96, 16, False, "flat"), (129, 17, 1, True, "edges"),
    # (10, 0): 97 <= L <= 160
    (2, 97, 2, False, "flat"), (2, 160, 4, True, "flat"), (65, 160, 1, False, "edges"), (8, 97, 16, True, "voff"),
    (9, 160, 16, False, "flat"), (17, 97, 8, True, "sharp"),
    # (17, 0): 161 <= L <= 272 but 257
    (2, 161, 2, False, "flat"), (1, 272, 4, False, "flat"), (2, 258, 1, True, "flat"), (4, 256, 16, True, "workflow"),
    (5, 256, 16, False, "edges"), (65, 272, 1, True, "flat"), (9, 258, 16, False, "flat"), (129, 272, 1, False, "sharp"),
    (10, 161, 16, True, "voff"),
    # (21, 0): 273 <= L <= 336 but 334
    (1, 273, 2, False, "flat"), (2, 336, 2, False, "flat"), (3, 333, 1, False, "edges"), (2, 335, 2, True, "flat"),
    (5, 300, 16, False, "flat"), (65, 336, 1, True, "edges"), (23, 300, 16, False, "voff"), (129, 335, 1, False, "flat"),
    (9, 300, 16, True, "flat"), (20, 333, 8, True, "sharp"),
    # (17, 257)
    (3, 257, 2, False, "flat"), (4, 257, 16, True, "edges"), (5, 257, 16, False, "voff"), (65, 257, 1, True, "flat"),
    (64, 257, 16, False, "flat"), (9, 257, 16, False, "sharp"), (9, 257, 16, True, "flat"), (33, 257, 16, True, "workflow"),
    # (21, 334), plain
    (4, 334, 16, False, "flat"), (65, 334, 1, False, "edges"), (8, 334, 16, False, "voff"), (129, 334, 1, False, "flat"),
    (16, 334, 16, False, "sharp"), (257, 334, 1, False, "flat"), (32, 334, 16, False, "workflow"), (33, 334, 8, False, "sharp"),
    (513, 334, 1, False, "flat"), (37, 334, 16, False, "flat"), (48, 334, 16, False, "edges"), (769, 334, 1, False, "flat"),
    (64, 334, 16, False, "voff"), (65, 334, 16, False, "flat"),
    # (21, 334), key_scale
    (1, 334, 16, True, "flat"), (2, 334, 3, True, "workflow"), (8, 334, 16, True, "flat"), (65, 334, 1, True, "voff"),
    (129, 334, 1, True, "edges"), (257, 334, 1, True, "sharp"), (65, 334, 16, True, "flat"),
]
REQUIRED_L = (1, 2, 15, 16, 17, 96, 97, 160, 161, 256, 257, 258, 272, 273, 300, 333, 334, 335, 336)
REQUIRED_BH_334 = (64, 65, 128, 129, 256, 257, 512, 513, 768, 769, 1024, 1040)


def case_id(case):
    B, L, H, scaled, data = case
    return f"{B}x{L}x{H}-{'ks' if scaled else 'plain'}-{data}"


# ------------------------------------------------------------------------------------------------------------------ data
def _seed(B, L, H, data, salt=0):
    return 1000003 * B + 1009 * L + 17 * H + 7 * DATA_SETS.index(data) + salt


def make_qkv(B, L, H, data, salt=0):
    """Seeded qkv [B, L, 3 H 64] ("(K H D)": q, k, v thirds, head-major inside each) as a bf16 tensor.
      workflow  randn x 1.5 (the scale of the operator tests)
      flat      q and k x 0.05: P is near-uniform, so every key carries 1 / L of every row -- a dropped, doubled or leaked key
                and a wrong row sum move the whole output
      sharp     q and k randn x 3: a few keys carry each row
      voff      workflow with V + 4: the outputs sit at 4, errors of the row sum show undiluted
      edges     workflow with a key-0 sink in the even heads (b H + h even; queries q % 3 != 0 look at key 0 with a logit lead of
                about 24) and, in every head, queries q % 6 == 0 whose dominant key is L - 1 (a lead of about 9) and queries q % 6 == 3 that
                give key L - 1 about half of the row (a lead of log L: a doubled last key moves them most)"""
    g = torch.Generator().manual_seed(_seed(B, L, H, data, salt))
    x = torch.randn(B, L, 3, H, DH, generator=g)
    if data == "flat":
        x[:, :, :2] *= 0.05
        x[:, :, 2] *= 1.5
    elif data == "sharp":
        x[:, :, :2] *= 3.0
        x[:, :, 2] *= 1.5
    else:
        x *= 1.5
    if data == "voff":
        x[:, :, 2] += 4.0
    if data == "edges":
        e = torch.randn(DH, generator=g)
        e = e / e.norm()
        even = ((torch.arange(B)[:, None] * H + torch.arange(H)[None, :]) % 2 == 0).to(x.dtype)      # [B, H]
        sinkq = (torch.arange(L) % 3 != 0).to(x.dtype)
        x[:, 0, 1] += 24.0 * e * even[:, :, None]                                                    # key 0 of the sink heads
        x[:, :, 0] += 8.0 * e * even[:, None, :, None] * sinkq[None, :, None, None]
        last = x[:, L - 1, 1].clone()                                                                # [B, H, 64], |k| about 12
        x[:, torch.arange(0, L, 6), 0] = 0.5 * last[:, None]
        half = 8.0 * (np.log(L) + 0.3) / (last * last).sum(-1, keepdim=True)
        x[:, torch.arange(3, L, 6), 0] = (half * last)[:, None]
    return x.reshape(B, L, 3 * H * DH).to(torch.bfloat16)


def make_key_scale(B, L, salt=0):
    """Seeded key_scale [B, L] fp32 (the attention-map edit: column factors on the normalised P): a third of the columns at
    exp(U(-2.3, 2.3)), the rest 1; two columns at 0 and two at 40 (the reference's p2p_multiplier range) where L allows; with B >= 2
    the whole row of the last sample is 0 (its output must be exactly 0)."""
    g = torch.Generator().manual_seed(_seed(B, L, 1, "workflow", 991 + salt))
    ks = torch.ones(B, L)
    pick = torch.rand(B, L, generator=g) < 1.0 / 3.0
    val = torch.exp((torch.rand(B, L, generator=g) * 2.0 - 1.0) * 2.3)
    ks = torch.where(pick, val, ks)
    for b in range(B):
        cols = torch.randperm(L, generator=g)[:4].tolist()
        for j, c in enumerate(cols if L >= 8 else cols[:2]):
            ks[b, c] = 0.0 if j % 2 == 0 else 40.0
    if B >= 2:
        ks[B - 1] = 0.0
    return ks.float()


# ------------------------------------------------------------------------------------------------------------------ references
def head_qkv(qkv, H, heads):
    """The (b, h) pairs of ``heads`` (b H + h indices) as a batch of one-head samples [n, L, 192] float64."""
    B, L, _ = qkv.shape
    x = qkv.reshape(B, L, 3, H, DH).permute(0, 3, 1, 2, 4).reshape(B * H, L, 3 * DH)
    return x[torch.as_tensor(heads, dtype=torch.long)].to(torch.float64)


def head_out(out, H, heads):
    """The same heads of an attention output [B, L, H 64] as [n, L, 64] float64."""
    B, L, _ = out.shape
    x = out.reshape(B, L, H, DH).permute(0, 2, 1, 3).reshape(B * H, L, DH)
    return x[torch.as_tensor(heads, dtype=torch.long)].to(torch.float64)


def reference(qkv, H, heads, rnd, key_scale=None, fn=attention):
    """``fn`` (uvit_stages.attention or one of PERTURBED) on the heads ``heads`` of qkv, each as a one-head sample: [n, L, 64]."""
    x = head_qkv(qkv, H, heads)
    ks = None if key_scale is None else key_scale.to(torch.float64)[torch.as_tensor(heads, dtype=torch.long) // H]
    return fn(x, 1, rnd, ks)


# ------------------------------------------------------------------------------------------------------------------ metrics
def _worst(num, den):
    r = num / np.maximum(den, 1e-30)
    r = np.where(np.isnan(r), np.inf, r)          # a NaN output is as wrong as an output gets
    return float(r.max()) if r.size else 0.0


def head_err(got, ref):
    """Worst rel-L2 over heads; got, ref [n, L, 64]."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return _worst(np.sqrt(((got - ref) ** 2).sum((1, 2))), np.sqrt((ref ** 2).sum((1, 2))))


def row_err(got, ref):
    """Worst rel-L2 over (head, query) rows of 64."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return _worst(np.sqrt(((got - ref) ** 2).sum(2)), np.sqrt((ref ** 2).sum(2)))


def envelope_excess(got, ref, k, a):
    """max |got - ref| / (k 2^-8 |ref| + a): at most 1 inside the element-wise envelope.  ``a`` an array like ref or a number.  Where
    both sides of the envelope are 0 (a sample whose key_scale row is 0) the excess is 0."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    num, den = np.abs(got - ref), k * 2.0 ** -8 * np.abs(ref) + np.asarray(a, np.float64)
    return _worst(num, np.where((num == 0) & (den == 0), 1.0, den))


def envelope_a(x, key_scale=None):
    """The absolute term of the envelope for one-head samples x [n, L, 192], per element [n, L, 64]: 2^-6 A with
    A = sum_k P_k ks_k |v_k| / sum_k P_k (the attention of |V|).  A bf16(P ks) that rounds the other way than in the reference is off
    by one ulp, at most 2^-7 of itself: if EVERY one did, the numerator would move by at most 2^-7 A and the row sum by 2^-7 of itself,
    which moves the output by 2^-7 |o| <= 2^-7 A.  The relative term k = 2 is one bf16 ulp of the stored output, between 2^-8 and 2^-7
    of the value."""
    y = x.clone()
    y[:, :, 2 * DH:] = y[:, :, 2 * DH:].abs()
    ks = None if key_scale is None else key_scale.to(torch.float64)
    return (2.0 ** -6 * attention(y, 1, False, ks)).numpy()


# ------------------------------------------------------------------------------------------------------------------ faults
# uvit_stages.attention with one fault each, same signature.  They work on whatever batch they are given; reference() hands them
# one-head samples, so "the next head" is the next sample of that batch.
def _with_query(x, H, row):
    """x with the query part of its row 0 replaced by that of ``row`` (an [B, 1, 3 H 64] slice)."""
    y = x.clone()
    y[:, 0, :H * DH] = row[:, 0, :H * DH]
    return y


def last_key_masked(qkv, H, rnd, key_scale=None):
    """Key L - 1 invisible to every query (a mask off by one)."""
    L = qkv.shape[1]
    if L < 2:
        raise ValueError("needs two keys")
    ks = None if key_scale is None else key_scale[:, :L - 1]
    head = qkv[:, :L - 1]
    out = attention(head, H, rnd, ks)                                                  # queries 0 .. L-2 over keys 0 .. L-2
    tail = attention(_with_query(head, H, qkv[:, L - 1:]), H, rnd, ks)[:, :1]          # query L-1 over the same keys
    return torch.cat([out, tail], 1)


def pad_key_visible(qkv, H, rnd, key_scale=None):
    """One padding key visible: the kernel stages row L - 1 again in the rows behind L, so a leak counts that key twice."""
    L = qkv.shape[1]
    ks = None if key_scale is None else torch.cat([key_scale, key_scale[:, L - 1:]], 1)
    return attention(torch.cat([qkv, qkv[:, L - 1:]], 1), H, rnd, ks)[:, :L]


def key_scale_shifted(qkv, H, rnd, key_scale=None):
    """key_scale applied one column late."""
    return attention(qkv, H, rnd, torch.roll(key_scale, 1, dims=1))


def scaled_sum_norm(qkv, H, rnd, key_scale=None):
    """Rows normalised by the sum of the SCALED P.  The ratio of the two sums comes from a plain float64 run with V = 1 (so it
    misses the bf16 rounding of P in the sums: 2^-8 of a fault that is of order one); 0 / 0 is NaN, as on the GPU."""
    B, L, _ = qkv.shape
    ones = qkv.clone().reshape(B, L, 3, H, DH)
    ones[:, :, 2] = 1.0
    ratio = attention(ones.reshape(B, L, -1), H, False, key_scale)                    # sum(P ks) / sum(P) in every element
    out = attention(qkv, H, rnd, key_scale) / ratio
    return out.to(torch.bfloat16).to(torch.float64) if rnd else out


def tile_from_next_head(qkv, H, rnd, key_scale=None, tile=1, head=0):
    """Queries 16 tile .. 16 tile + 15 of head ``head`` (a b H + h index) computed against the KEYS of the next head."""
    B, L, _ = qkv.shape
    if B * H < 2:
        raise ValueError("needs two heads")
    x = qkv.reshape(B, L, 3, H, DH)
    k = x[:, :, 1].permute(0, 2, 1, 3).reshape(B * H, L, DH)
    y = x.clone()
    y[:, :, 1] = torch.roll(k, -1, dims=0).reshape(B, H, L, DH).permute(0, 2, 1, 3)
    good = attention(qkv, H, rnd, key_scale).reshape(B, L, H, DH).clone()
    bad = attention(y.reshape(B, L, -1), H, rnd, key_scale).reshape(B, L, H, DH)
    b, h = divmod(head, H)
    q0 = min(16 * tile, max(L - 16, 0))
    good[b, q0:q0 + 16, h] = bad[b, q0:q0 + 16, h]
    return good.reshape(B, L, H * DH)


# fault -> (function, needs key_scale, data sets meant to expose it to the rel-L2 bounds, ... to the element-wise envelope, ... to every
# bound when a fault that does not need key_scale is run with it).  The envelope allows for every rounding of P falling the wrong way,
# which on 'flat' data is more than one key's share of a row: it sees a fault only where single keys carry a row, so it gets the
# 'edges' / 'sharp' / 'workflow' sets.  Under key_scale the 40x columns of make_key_scale outweigh the one key that a wrong mask drops
# or doubles on 'flat' data (row_tight separates it by 1.2x only): there the two mask faults are exposed by 'edges' alone, whose rows
# hang on key L - 1 -- on the GPU by the key_scale cases on 'edges' (129x17x1, 65x336x1, 4x257x16, 129x334x1).
PERTURBED = dict(
    last_key_masked=(last_key_masked, False, ("flat", "edges"), ("edges",), ("edges",)),
    pad_key_visible=(pad_key_visible, False, ("flat",), ("edges",), ("edges",)),
    key_scale_shifted=(key_scale_shifted, True, ("flat", "workflow"), ("sharp",), ()),
    scaled_sum_norm=(scaled_sum_norm, True, ("flat", "voff"), ("sharp",), ()),
    tile_from_next_head=(tile_from_next_head, False, ("workflow", "sharp"), ("workflow",), ("workflow", "sharp")),
)


# ------------------------------------------------------------------------------------------------------------------ GPU test tables
# Bounds of tests/test_gpu_attention_parity.py: 3x the worst value an MI355X measured over CASES, every head of every case, against the
# float64 reference (beside each), or analytic.  Without key_scale one rounded P feeds both P.V and the row sum, so a rounding of P that
# falls the other way than in float64 (fp32 logits: about one in a thousand does) largely cancels; with it bf16(P ks) and bf16(P) round
# apart, and a factor of 0 on a row's leading key leaves the row to a few small P, each flip 2^-8 .. 2^-7 of it: separate bounds.
TOL = dict(
    att_tight=9.8e-4,       # measured 3.2e-4 (5x256x16 edges; 0 at L <= 17): worst head vs float64 with the kernel's roundings, no key_scale
    att_tight_ks=3.9e-3,    # measured 1.3e-3 (17x97x8 sharp; 7.7e-4 at 20x333x8 sharp): ... with key_scale
    att_loose=7.4e-3,       # measured 2.5e-3 (64x257x16 flat): worst head vs plain float64 softmax, no key_scale
    att_loose_ks=1.3e-2,    # measured 4.3e-3 (129x334x1 edges): ... with key_scale
    row_tight=1.3e-2,       # measured 4.2e-3 (33x334x8 sharp): worst query row vs the tight reference, no key_scale
    row_tight_ks=2.0e-2,    # measured 6.6e-3 (257x334x1 sharp): ... with key_scale
    env_k=2.0,              # analytic: one bf16 ulp of the stored output is at most 2^-7 of its value
    env_a=1.0,              # analytic: x envelope_a (every rounding of P a whole ulp the other way); measured: 0.43 of the envelope
                            # used (257x334x1 key_scale sharp; 0.33 without key_scale)
)


def tol(name, scaled):
    return TOL[name + "_ks" if scaled else name]


# part C: (B, H) per launch form and L; one L per (NT, LC) instantiation
FORM_BATCHES = {
    334: [(3, 1), (1, 16), (70, 1), (8, 16), (200, 1), (300, 1), (32, 16), (600, 1), (37, 16), (64, 16), (1030, 1)],
    257: [(3, 1), (1, 16), (70, 1), (8, 16), (200, 1), (33, 16), (1030, 1)],
    300: [(3, 1), (1, 16), (70, 1), (8, 16), (200, 1), (33, 16)],
    258: [(3, 1), (1, 16), (70, 1), (8, 16), (200, 1), (33, 16)],
    160: [(3, 1), (1, 16), (70, 1), (8, 16), (200, 1)],
    81: [(3, 1), (1, 16), (70, 1), (8, 16), (200, 1)],
}
# part D: a ragged L per instantiation, (B, H) per launch
RAGGED_L = {(6, 0): 81, (10, 0): 150, (17, 0): 258, (21, 0): 300, (17, 257): 257, (21, 334): 334}
BRANCH_BH = dict(small=[(3, 2)], two=[(5, 16)], one=[(9, 16)], hpw2=[(257, 1), (20, 16)], hpw4=[(37, 16), (769, 1)])


def launch_table():
    """[(launch, kernel, first case that reaches it)] for the 38 launches."""
    return [(l, launch_form(*c[:4]), c) for l in all_launches() for c in [next(c for c in CASES if case_launch(c) == l)]]
