"""Cases, layouts, data sets, float64 references, guarded buffers, checks and perturbed stand-ins for the bf16 GEMM
(uspace_amd/csrc/gemm.hip: uspace_gemm_bf16 / _ext / _slabs_bf16); a helper of tests/test_gemm_cases.py (CPU) and
tests/test_gpu_gemm_parity.py (GPU), not a test.

``CASES`` lists one launch per form the dispatcher can take and role (plain, producer or consumer of a folded LayerNorm, two K slabs,
nine row-shifted slabs); ``launches`` pairs each of a case's epilogues with operand layouts; ``Win`` is a window inside a larger,
canary-filled allocation; ``make_data`` / ``reference`` give the seeded operands and their float64 result with a per-element error
bound; ``check`` compares what a launch (or a stand-in) left in the windows; ``standin`` is a float32 NumPy GEMM that stores through
the same windows and takes one ``fault`` of ``PERTURBED``: what a subtly wrong kernel would compute.

Bounds.  u = 2^-24.  fp32 accumulation of K products and a few epilogue terms in ANY order is within (K + 8) u S_abs of the exact
value, S_abs = |A| |W|^T + |resid| + |row_add col_add| + |bias|.  On 'lattice' data (small integers) every partial sum is an integer
below 2^24, so the bound is 0 and outputs are compared bit for bit.  A bf16 store adds 2^-8 of the value (half an ulp, RNE).

GELU: gelu_erf of common.h is documented within min(4.1e-7, 1.0e-6 |v|) of the exact erf form; with |gelu'| <= 1.13 an error e of the
pre-activation becomes 1.13 e, and the fp32 result carries one more rounding u |gelu|.

LayerNorm consumer (LN_IN).  The kernel computes, all in fp32, s1 = sum_q part[q][0], s2 = sum_q part[q][1] (np terms each),
d = s1 inv_d, q = s2 inv_d - d d + eps, r = rsqrt(q), y = acc r + (colsum (-d r) + bias).  First-order propagation, with D = norm_dim:
    E_d = (np + 2) u sum_q |part[q][0]| / D                     np - 1 adds, the rounding of inv_d, the multiply
    E_q = (np + 2) u s2 / D + 2 |d| E_d + 2 u (d^2 + q)         the same for s2; d d; the subtraction and the + eps
    rho = E_q / (2 q) + 4 u                                     d r / r = - d q / (2 q); the hardware rsqrt is good to 2 ulp
    E_y = r E_acc + (|acc| + |d colsum|) r (rho + 3 u) + |colsum| r E_d + 3 u (|y| + |bias|)
    E_c = E_d + u (|d| + |c_out|)                               c_out = row_c + d
E_q / q stays small only while q is no cancellation: ``reference`` asserts d^2 <= var on the float64 values."""
import ctypes
import functools
from collections import namedtuple

import numpy as np
import torch

B_, G_, R_, F_, H_, C_, L_, K_ = 1, 2, 4, 8, 16, 32, 64, 128      # USPACE_EPI_* of include/uspace_hip.h
U = 2.0 ** -24
BF16_EPS = 2.0 ** -8
GUARD = 272                      # BM + 16 rows around every 2-D window: a stray tile row lands in the guards
CANARY_F32 = 0x7FC5A3E1          # NaNs with a fixed payload: a read poisons the output, a write changes the pattern
CANARY_BF16 = 0x7FA5
LN_EPS = 1e-5

PLAIN_FLAGS = (H_, B_ | H_, B_ | G_ | H_, B_ | R_ | F_, B_ | R_ | F_ | H_, B_ | F_, B_ | F_ | H_, F_)
PRODUCER_FLAGS = (C_ | B_ | R_ | F_, C_ | B_ | R_ | F_ | H_, C_ | B_ | F_, K_ | C_ | B_ | F_)
CONSUMER_FLAGS = (L_ | B_ | H_, L_ | B_ | G_ | H_)
SK_PLAIN_FLAGS = (B_ | R_ | F_, B_ | R_ | F_ | H_)      # the plain epilogues the in-launch K-split tail is instantiated for (sk_flags)
ROLES = ("plain", "producer", "consumer", "two-slab", "two-slab-producer", "slabs")
LAYOUTS = ("a", "b", "c", "d", "e")
DATA_SETS = ("lattice", "workflow")
SLAB_SHIFTS = (-9, -8, -7, -1, 0, 1, 7, 8, 9)           # the taps of a 3x3 convolution over a map 8 pixels wide (6 + border)


def flag_name(f):
    return "".join(n for b, n in ((K_, "K"), (L_, "L"), (C_, "C"), (B_, "B"), (G_, "G"), (R_, "R"), (F_, "F"), (H_, "H")) if f & b)


# ------------------------------------------------------------------------------------------------------------------ cases
# what: the entry of the issue's coverage list a case stands for; expect: what uspace_gemm_plan_k must answer for it
Case = namedtuple("Case", "M N K role form what expect")


def _c(M, N, K, role, form, what, **expect):
    return Case(M, N, K, role, form, what, tuple(sorted(expect.items())))      # (hashable: make_data caches by case)


# K of a 'slabs' case is K1 of one slab (the launch has K = 9 K1)
CASES = [
    _c(17701, 640, 64, "plain", 0, "0", strip=False),
    _c(21761, 516, 64, "plain", 0, "0-strip", strip=True),
    _c(23141, 260, 64, "plain", 1, "1", strip=False),
    _c(24577, 320, 64, "plain", 1, "1-strip", strip=True),
    _c(2725, 3072, 64, "plain", 2, "2", strip=True, tiles=161),
    _c(10241, 132, 64, "plain", 2, "2", strip=False, tiles=161),
    _c(17537, 1024, 64, "plain", 3, "3", split_rows=16384),
    _c(16385, 132, 64, "plain", 4, "4", strip=False),
    _c(21761, 320, 64, "plain", 4, "4-strip", strip=True),
    _c(70, 64, 64, "plain", 5, "5-two", per_round=1024),
    _c(1030, 260, 192, "plain", 5, "5-two", per_round=1024),
    _c(641, 3072, 1024, "plain", 5, "5-ring", per_round=512, strip=True),
    _c(1, 64, 256, "plain", 5, "5-ring", per_round=512),
    _c(2177, 3072, 4096, "plain", 6, "6-S2", S=2, n_dp=0),
    _c(8961, 768, 4096, "plain", 6, "6-strip", S=2, strip=True, n_dp=0),
    _c(3265, 1280, 4096, "plain", 6, "6-S3", S=3, n_dp=0),
    _c(769, 3072, 4096, "plain", 6, "6-S4", S=4, strip=True, n_dp=0),
    _c(4353, 4096, 4096, "plain", 6, "6-round", S=4, n_dp=256),
    _c(1030, 260, 128, "two-slab", 5, "5-two", per_round=1024),
    _c(769, 3072, 4096, "two-slab", 6, "6-S4", S=4, strip=True, n_dp=0),
    _c(1281, 3072, 64, "producer", 0, "p0", strip=False),
    _c(21761, 516, 64, "producer", 0, "p0", strip=True),
    _c(23141, 260, 64, "producer", 1, "p1"),
    _c(1, 640, 64, "producer", 2, "p2"),
    _c(16385, 132, 64, "producer", 4, "p4"),
    _c(1030, 260, 192, "producer", 5, "p5", per_round=1024),
    _c(1, 64, 256, "producer", 5, "p5", per_round=512),
    _c(2049, 1024, 4096, "producer", 6, "p6", S=4, strip=True),
    _c(1028, 1024, 2048, "producer", 2, "ksplit", ksplit=2),
    _c(1028, 1024, 2048, "two-slab-producer", 2, "ksplit", ksplit=2),
    _c(1028, 1024, 4096, "producer", 2, "ksplit", ksplit=2),
    _c(17701, 640, 64, "consumer", 0, "c0"),
    _c(23141, 260, 64, "consumer", 1, "c1"),
    _c(10241, 132, 64, "consumer", 2, "c2"),
    _c(17537, 1024, 64, "consumer", 3, "c3", split_rows=16384),
    _c(16385, 132, 64, "consumer", 4, "c4"),
    _c(70, 64, 64, "consumer", 5, "c5-two", per_round=1024),
    _c(641, 3072, 1024, "consumer", 5, "c5-ring", per_round=512, strip=True),
    _c(300, 64, 64, "slabs", 5, "slabs", per_round=512),
    _c(10241, 132, 64, "slabs", 2, "slabs"),
]
REQUIRED = ("0", "0-strip", "1", "1-strip", "2", "3", "4", "4-strip", "5-two", "5-ring", "6-S2", "6-S3", "6-S4", "6-strip", "6-round",
            "ksplit", "slabs", "p0", "p1", "p2", "p4", "p5", "p6", "c0", "c1", "c2", "c3", "c4", "c5-two", "c5-ring")


def case_id(c):
    return f"{c.role}-{c.M}x{c.N}x{c.K}-form{c.form}"


def is_producer(c):
    return c.role in ("producer", "two-slab-producer")


def full_k(c):
    return c.K * len(SLAB_SHIFTS) if c.role == "slabs" else c.K


def case_flags(c):
    """The epilogues run on a case: every one dispatch_flags accepts for the role (the tail forms: every one that takes the tail)."""
    if is_producer(c):
        return PRODUCER_FLAGS
    if c.role == "consumer":
        return CONSUMER_FLAGS
    return SK_PLAIN_FLAGS if c.form == 6 else PLAIN_FLAGS


def layout_applies(layout, flags):
    """(c), (d) are about the bf16 outputs and (e) is about the residual: they say nothing on an epilogue without them."""
    if layout in ("c", "d"):
        return bool(flags & (H_ | C_))
    if layout == "e":
        return bool(flags & R_)
    return True


SMALL_CASE = 1 << 19        # M N up to here: every epilogue on every layout
# beyond: a plain case runs each of its eight epilogues on one layout, all five between them ...
PLAIN_LAYOUT = {H_: "d", B_ | H_: "c", B_ | G_ | H_: "b", B_ | R_ | F_: "e", B_ | R_ | F_ | H_: "a", B_ | F_: "b", B_ | F_ | H_: "d", F_: "a"}


def launches(c):
    """[(flags, layout)] of a case."""
    out = []
    j = CASES.index(c) if c in CASES else 0
    for i, f in enumerate(case_flags(c)):
        lay = [l for l in LAYOUTS if layout_applies(l, f)]
        if c.M * c.N <= SMALL_CASE:
            out += [(f, l) for l in lay]
        elif case_flags(c) is PLAIN_FLAGS:
            out.append((f, PLAIN_LAYOUT[f]))
        elif case_flags(c) is SK_PLAIN_FLAGS:           # ... the tail's two epilogues one layout each, rotating with the case
            out.append((f, lay[j % len(lay)]))
        else:                                           # ... producers and consumers two layouts per epilogue, rotating
            out += [(f, lay[(i + j) % len(lay)]), (f, lay[(i + j + 2) % len(lay)])]
    return out


def plan_of(lib, c):
    """out[8] of uspace_gemm_plan_k for the launch of a case (nine-slab launches never take the K-split tail: asked with it off)."""
    out = (ctypes.c_int * 8)()
    if c.role == "slabs":
        assert lib.uspace_gemm_set_sk(0) == 0
    try:
        assert lib.uspace_gemm_plan_k(c.M, c.N, full_k(c), int(is_producer(c)), out) == 0
    finally:
        lib.uspace_gemm_set_sk(-1)
    return list(out)


def geometry(c, plan, split_bytes=0):
    """The facts of a launch the reference and the stand-in need, from out[8] of uspace_gemm_plan_k: tile rows BM and partial-sum
    columns BN, partial-sum slots per row, K parts S, the first strip row m_main, the row the split form cuts at, and whether the
    partial sums follow the finish kernel's convention (everything in slot 0)."""
    form, x, BM, BN, tiles_m, tiles_n, n_strip = plan[:7]
    ksplit = is_producer(c) and form == 2 and split_bytes > 0
    return dict(BM=BM, BN=BN, slots=tiles_n, S=x if form == 6 else (split_bytes // (4 * c.M * c.N) if ksplit else 1),
                m_main=tiles_m * BM if n_strip > 0 else c.M, split_rows=x if form == 3 else 0, finish=ksplit)


def sample_rows(c, geom, n_dp=0):
    """All rows -- or, for the one case with a whole round of tiles in front of the shared ones (n_dp > 0) when it is beyond 2^34
    multiply-adds, a sample: every row of the first and the last tile row, every strip row and, in EVERY tile row (the shared tiles are
    spread over them), the rows on both sides of each 16-row sub-tile edge (the K parts of a shared tile own whole sub-tiles: own_lo /
    own_hi are such edges)."""
    M = c.M
    if n_dp == 0 or M * c.N * full_k(c) <= 1 << 34:
        return None
    BM = geom["BM"]
    last = (min(geom["m_main"], M) - 1) // BM * BM
    parts = [np.arange(min(BM, M)), np.arange(last, M)]
    for t0 in range(0, M, BM):
        e = t0 + 16 * np.arange(BM // 16 + 1)
        parts += [e - 1, e]
    r = np.unique(np.concatenate(parts))
    return r[(r >= 0) & (r < M)]


# ------------------------------------------------------------------------------------------------------------------ bf16
def bf16_bits(x):
    """fp32 -> bf16 bit patterns, round to nearest even (finite inputs)."""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return ((b + (((b >> 16) & 1) + 0x7FFF)) >> 16).astype(np.uint16)


def bf16_trunc_bits(x):
    return (np.ascontiguousarray(x, np.float32).view(np.uint32) >> 16).astype(np.uint16)


def bf16_value(h):
    return (np.ascontiguousarray(h).astype(np.uint32) << 16).view(np.float32)


def bf16_round(x):
    return bf16_value(bf16_bits(x))


# ------------------------------------------------------------------------------------------------------------------ windows
class Win:
    """rows x cols values inside a (guard + rows + guard) x (col0 + cols + pad) allocation that is canary everywhere else.  The
    allocation is kept as unsigned integers (the bit patterns): kind 'f32' or 'bf16'."""

    def __init__(self, kind, rows, cols, pad=0, col0=0, guard=GUARD):
        self.kind, self.rows, self.cols, self.col0, self.guard = kind, rows, cols, col0, guard
        self.ld = col0 + cols + pad
        self.dtype, self.canary = (np.uint32, CANARY_F32) if kind == "f32" else (np.uint16, CANARY_BF16)
        self.buf = np.full((2 * guard + rows, self.ld), self.canary, self.dtype)

    @property
    def off(self):                       # of the window's first element, in elements
        return self.guard * self.ld + self.col0

    @property
    def itemsize(self):
        return self.buf.itemsize

    def view(self):
        return self.buf[self.guard:self.guard + self.rows, self.col0:self.col0 + self.cols]

    def flat(self):
        return self.buf.reshape(-1)

    def put(self, x):
        x = np.asarray(x, np.float32).reshape(self.rows, self.cols)
        self.view()[...] = x.view(np.uint32) if self.kind == "f32" else bf16_bits(x)
        return self

    def bits(self):
        return np.ascontiguousarray(self.view())

    def get(self):
        return self.bits().view(np.float32) if self.kind == "f32" else bf16_value(self.bits())

    def strays(self):
        """Elements outside the window that no longer hold the canary."""
        b = self.buf.copy()
        b[self.guard:self.guard + self.rows, self.col0:self.col0 + self.cols] = self.canary
        return int((b != self.canary).sum())

    def untouched(self):
        return bool((self.view() == self.canary).all())


def vec(n, x=None, guard=GUARD):
    """A vector of n fp32 values as a one-row window with ``guard`` canaries on either side."""
    w = Win("f32", 1, n, pad=guard, col0=guard, guard=0)
    return w if x is None else w.put(x)


def bf16_layout(layout, N):
    """(pad, col0) of a bf16 output window of N columns."""
    if layout in ("a", "e"):
        return 0, 0
    if layout == "b":                    # row stride % 8 == 0, 16-byte aligned: keeps the 16-byte stores
        return 8 - N % 8, 0
    if layout == "c":                    # row stride % 8 == 4
        return (4 - N % 8) % 8 or 8, 0
    return (-(4 + N)) % 8 or 8, 4        # (d) row stride % 8 == 0, the window 8 bytes into a 16-byte line


class Ops:
    """The operands of one launch: windows by name, how the launch addresses them, the launch's sizes."""


def build_ops(c, flags, layout, d, geom):
    M, N, K = c.M, c.N, full_k(c)
    o = Ops()
    o.case, o.flags, o.layout, o.geom = c, flags, layout, geom
    o.M, o.N, o.K = M, N, K
    o.K1 = K // 2 if c.role.startswith("two-slab") else c.K
    o.norm_dim, o.eps = K, LN_EPS
    pad_in = 0 if layout == "a" else 8
    w = o.w = {}
    A = d["A"]
    o.a_row0 = (A.shape[0] - M) // 2                                   # slabs: the shifted rows above row 0 are data, not guards
    if c.role.startswith("two-slab") and layout == "a":                                     # two contiguous slabs
        w["A"], w["A2"] = Win("bf16", M, o.K1).put(A[:, :o.K1]), Win("bf16", M, o.K1).put(A[:, o.K1:])
        o.a2 = ("A2", 0)
    else:                                                              # [A | A2] as column windows of one buffer: lda2 == lda
        w["A"] = Win("bf16", A.shape[0], A.shape[1], pad=pad_in).put(A)
        o.a2 = ("A", o.K1) if c.role.startswith("two-slab") else None
    w["W"] = Win("bf16", N, K, pad=pad_in).put(d["W"])
    if flags & B_:
        w["bias"] = vec(N, d["bias"])
    f32_pad = 4 if layout in ("b", "d") else 0
    if flags & F_:
        w["out_f32"] = Win("f32", M, N, pad=f32_pad)
    o.resid = None
    if flags & R_:
        if layout in ("a", "c"):                                       # in place
            o.resid = "out_f32"
            w["out_f32"].put(d["resid"])
        else:
            o.resid = "resid"
            w["resid"] = Win("f32", M, N, pad=f32_pad + 4).put(d["resid"])
            o.resid_bits = w["resid"].bits()
    bpad, bcol = bf16_layout(layout, N)
    if flags & H_:
        w["out_bf16"] = Win("bf16", M, N, pad=bpad, col0=bcol)
    if flags & C_:
        w["out_cen"] = Win("bf16", M, N, pad=bpad, col0=bcol)
        w["part_out"] = Win("f32", M, 2 * geom["slots"])
        w["row_c"] = vec(M, d["row_c"])
    if flags & K_:
        w["row_add"], w["col_add"] = vec(M, d["row_add"]), vec(N, d["col_add"])
    if flags & L_:
        o.np_in = d["part_in"].shape[1]
        w["part_in"] = Win("f32", M, 2 * o.np_in).put(d["part_in"].reshape(M, -1))
        w["colsum"], w["row_c"], w["c_out"] = vec(N, d["colsum"]), vec(M, d["row_c"]), vec(M)
    return o


# ------------------------------------------------------------------------------------------------------------------ data
def _seed(c, dataset):
    return 1000003 * c.M + 1009 * c.N + 17 * c.K + 7 * ROLES.index(c.role) + DATA_SETS.index(dataset)


def _ints(g, lo, hi, *shape):
    return g.integers(lo, hi + 1, shape).astype(np.float32)


@functools.lru_cache(maxsize=2)
def make_data(c, dataset):
    """Seeded operands of a case as fp32 arrays (A, W hold bf16 values).
      lattice   small integers: {-3 .. 3}, or {-1, 0, 1} in A and W of a producer with K >= 1024 (its sums of squares stay below 2^24);
                the bias of every other role is {-3 .. 3} + 1000 {-1, 0, 1}, of a producer on 64x64 tiles {-3 .. 3}, + 300 {-1, 0, 1} in every eighth column
      workflow  bf16-rounded Gaussians at the scale of the operator tests; producers get rows with large, differing means"""
    g = np.random.default_rng(_seed(c, dataset))
    M, N, K = c.M, c.N, full_k(c)
    sh = max(np.abs(SLAB_SHIFTS)) if c.role == "slabs" else 0
    d = {}
    if dataset == "lattice":
        a = 1 if is_producer(c) and K >= 1024 else 3
        d["A"], d["W"] = _ints(g, -a, a, M + 2 * sh, c.K if sh else K), _ints(g, -a, a, N, K)
        d["bias"], d["resid"] = _ints(g, -3, 3, N), _ints(g, -3, 3, M, N)
        # integers beyond 256 are not all bf16 values: the rounding of the bf16 outputs (a producer's out_cen among them) has something to
        # do.  Producers get it in every eighth column, and only on few columns (the 64x64 form, the stand-ins): N / 8 x 350^2 stays below 2^24
        if not is_producer(c):
            d["bias"] += np.float32(1000.0) * _ints(g, -1, 1, N)
        elif c.form in (5, -1) and K < 1024:
            d["bias"] += np.float32(300.0) * _ints(g, -1, 1, N) * (np.arange(N) % 8 == 0)
        d["row_c"], d["row_add"], d["col_add"] = _ints(g, -2, 2, M), _ints(g, -3, 3, M), _ints(g, -1, 1, N)
    else:
        d["A"] = bf16_round(g.standard_normal((M + 2 * sh, c.K if sh else K), np.float32))
        d["W"] = bf16_round(g.standard_normal((N, K), np.float32) * np.float32(0.1))
        d["bias"] = g.standard_normal(N, np.float32)
        mean = g.standard_normal((M, 1), np.float32) * np.float32(2.0 if is_producer(c) else 0.0)
        d["resid"] = g.standard_normal((M, N), np.float32) * np.float32(1.5) + mean
        d["row_c"] = (mean[:, 0] + np.float32(0.05) * g.standard_normal(M, np.float32)).astype(np.float32)
        d["row_add"], d["col_add"] = g.standard_normal(M, np.float32) * np.float32(3.0), d["W"][:, K // 2:].sum(1).astype(np.float32)
    if c.role == "consumer":
        # the statistics a producer would have published for rows of variance 0.5 .. 2.5 whose centring constants are off by
        # d = -0.3 .. 0.3 standard deviations (d^2 <= var: no cancellation), cut into np slots of random positive weight
        npi = 1 + M % 8
        wq = g.random((M, npi)) + 0.1
        wq /= wq.sum(1, keepdims=True)
        var = 0.5 + 2.0 * g.random(M)
        dm = (g.random(M) * 0.6 - 0.3) * np.sqrt(var)
        part = np.stack([(K * dm)[:, None] * wq, (K * (var + dm * dm))[:, None] * wq], 2)
        d["part_in"] = part.astype(np.float32)
        d["colsum"] = d["W"].sum(1).astype(np.float32)
        if dataset == "workflow":
            d["row_c"] = g.standard_normal(M, np.float32)
    d["dataset"] = dataset
    return d


def gelu64(v):
    t = torch.from_numpy(np.ascontiguousarray(v, np.float64))
    return (0.5 * t * (1.0 + torch.erf(t / np.sqrt(2.0)))).numpy()


def reference(c, d, flags, geom, rows=None, cache=None):
    """The float64 result of a launch on the rows ``rows`` (all: None) and its error bounds, as a dict:
      v, e         the value the epilogue stores [r, N] and the bound of its fp32 form (0 where it is exact)
      vc, ec       producers: v - row_c and its bound;  part, epart [r, slots, 2]: the partial sums of each BN-column tile (the finish
                   kernel's convention: the row's sums in slot 0, zeros behind) and their bounds
      c_out, e_c   consumers: row_c + d
      exact        lattice data through an epilogue without GELU / LayerNorm: compare bit for bit
    On lattice data it asserts the preconditions of exactness.  ``cache`` (a dict) keeps the matrix products between epilogues."""
    M, N, K = c.M, c.N, full_k(c)
    lattice = d["dataset"] == "lattice"
    rows = np.arange(M) if rows is None else rows
    cache = {} if cache is None else cache
    if "acc" not in cache:
        A, W = d["A"].astype(np.float64), d["W"].astype(np.float64)
        if c.role == "slabs":
            sh = (A.shape[0] - M) // 2
            cache["acc"] = sum(A[rows + sh + s] @ W[:, t * c.K:(t + 1) * c.K].T for t, s in enumerate(SLAB_SHIFTS))
            cache["sabs"] = 0.0 if lattice else sum(np.abs(A[rows + sh + s]) @ np.abs(W[:, t * c.K:(t + 1) * c.K]).T for t, s in enumerate(SLAB_SHIFTS))
        else:
            cache["acc"] = A[rows] @ W.T
            cache["sabs"] = 0.0 if lattice else np.abs(A[rows]) @ np.abs(W).T
        if lattice:     # sum_k |a| |w| < 2^24: every partial sum of the products, in any order, is an exact fp32 integer
            assert (np.abs(A).sum(1).max() * (len(SLAB_SHIFTS) if c.role == "slabs" else 1)) * np.abs(W).max() < 2 ** 24
    acc, sabs = cache["acc"], cache["sabs"]
    R = dict(exact=lattice and not flags & (G_ | L_), rows=rows)
    v, s = acc.copy(), sabs + np.zeros_like(acc)
    if flags & R_:
        v += d["resid"][rows]
        s += np.abs(d["resid"][rows])
    if flags & K_:
        t = d["row_add"][rows].astype(np.float64)[:, None] * d["col_add"].astype(np.float64)[None, :]
        v += t
        s += np.abs(t)
    if flags & B_ and not flags & L_:
        v += d["bias"].astype(np.float64)
        s += np.abs(d["bias"])
    e = np.zeros_like(v) if lattice else (K + 8) * U * s
    if flags & L_:
        p = d["part_in"][rows].astype(np.float64)
        npi, D = p.shape[1], float(K)
        dm, s2 = p[:, :, 0].sum(1) / D, p[:, :, 1].sum(1) / D
        var = s2 - dm * dm
        assert (dm * dm <= var).all()
        q = var + LN_EPS
        r = 1.0 / np.sqrt(q)
        cs, b = d["colsum"].astype(np.float64)[None, :], d["bias"].astype(np.float64)[None, :]
        y = r[:, None] * (acc - dm[:, None] * cs) + b
        E_d = (npi + 2) * U * np.abs(p[:, :, 0]).sum(1) / D
        E_q = (npi + 2) * U * s2 + 2 * np.abs(dm) * E_d + 2 * U * (dm * dm + q)
        rho = (E_q / (2 * q) + 4 * U)[:, None]
        e = r[:, None] * e + (np.abs(acc) + np.abs(dm[:, None] * cs)) * r[:, None] * (rho + 3 * U) + np.abs(cs) * (r * E_d)[:, None] \
            + 3 * U * (np.abs(y) + np.abs(b))
        v = y
        R["c_out"] = d["row_c"][rows].astype(np.float64) + dm
        R["e_c"] = E_d + U * (np.abs(dm) + np.abs(R["c_out"]))
    if flags & G_:
        pre = v
        v = gelu64(pre)
        e = 1.13 * e + np.minimum(4.1e-7, 1.0e-6 * np.abs(pre)) + U * np.abs(v)
    if lattice:
        assert np.abs(v).max() < 2 ** 24
    R["v"], R["e"] = v, e
    if flags & C_:
        vc = v - d["row_c"][rows].astype(np.float64)[:, None]
        ec = e if lattice else e + U * np.abs(vc)
        BN, slots = geom["BN"], geom["slots"]
        if lattice:
            assert np.abs(vc).sum(1).max() < 2 ** 24 and (vc * vc).sum(1).max() < 2 ** 24
        part, epart = np.zeros((len(rows), slots, 2)), np.zeros((len(rows), slots, 2))
        for t in range(1 if geom["finish"] else slots):
            x, ex = (vc, ec) if geom["finish"] else (vc[:, t * BN:(t + 1) * BN], ec[:, t * BN:(t + 1) * BN])
            part[:, t, 0], part[:, t, 1] = x.sum(1), (x * x).sum(1)
            if not lattice:
                n = x.shape[1] + 8
                epart[:, t, 0] = ex.sum(1) + n * U * np.abs(x).sum(1)
                epart[:, t, 1] = (2 * np.abs(x) * ex + ex * ex).sum(1) + n * U * (x * x).sum(1)
        R.update(vc=vc, ec=ec, part=part, epart=epart)
    return R


# ------------------------------------------------------------------------------------------------------------------ checks
def _excess(got, ref, bound):
    """max |got - ref| / bound over the elements (inf for a NaN or an error where the bound is 0; 0 where both are 0)."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    err = np.where(np.isnan(err), np.inf, err)
    with np.errstate(divide="ignore", invalid="ignore"):
        x = np.where(err == 0, 0.0, err / bound)
    return float(x.max()) if x.size else 0.0


def check(o, R):
    """Compare what a launch left in the windows of ``o`` with the reference ``R``.  Returns (failures, worst): a list of strings, empty
    when everything holds, and the largest error-over-bound of each toleranced comparison by output name."""
    fails, worst = [], {}
    w, flags, rows, exact = o.w, o.flags, R["rows"], R["exact"]
    for name, win in w.items():
        n = win.strays()
        if n:
            fails.append(f"{name}: {n} canaries changed")

    def cmp(name, got_win, ref, bound, is_bf16):
        if exact:
            want = bf16_bits(ref.astype(np.float32)) if is_bf16 else ref.astype(np.float32).view(np.uint32)
            got = got_win.bits()[rows]
            got = np.where(got == (0x8000 if is_bf16 else 0x80000000), 0, got)       # -0 is 0
            bad = int((got != want).sum())
            if bad:
                fails.append(f"{name}: {bad} elements differ from the exact result")
            return
        b = bound + BF16_EPS * (np.abs(ref) + bound) if is_bf16 else bound
        x = worst[name] = _excess(got_win.get()[rows], ref, b)
        if x > 1.0:
            fails.append(f"{name}: error {x:.3g} x its bound")

    if flags & F_:
        cmp("out_f32", w["out_f32"], R["v"], R["e"], False)
        if not exact and not flags & (G_ | L_):
            rl2 = np.linalg.norm(w["out_f32"].get()[rows] - R["v"]) / max(np.linalg.norm(R["v"]), 1e-30)
            if not rl2 < 1e-5:
                fails.append(f"out_f32: rel_l2 {rl2:.3g}")
    if flags & H_:
        cmp("out_bf16", w["out_bf16"], R["v"], R["e"], True)
        if flags & F_ and not (w["out_bf16"].bits() == bf16_bits(w["out_f32"].get())).all():
            fails.append("out_bf16 is not the bf16 rounding of out_f32")
    if flags & C_:
        cmp("out_cen", w["out_cen"], R["vc"], R["ec"], True)
        S = o.geom["slots"]
        if exact:
            bad = int((w["part_out"].bits().reshape(o.M, S, 2)[rows] != R["part"].astype(np.float32).view(np.uint32)).sum())
            if bad:
                fails.append(f"part_out: {bad} partial sums differ from the exact result")
        else:
            x = worst["part_out"] = _excess(w["part_out"].get().reshape(o.M, S, 2)[rows], R["part"], R["epart"])
            if x > 1.0:
                fails.append(f"part_out: error {x:.3g} x its bound")
    if flags & L_:
        x = worst["c_out"] = _excess(w["c_out"].get()[0][rows], R["c_out"], R["e_c"])
        if x > 1.0:
            fails.append(f"c_out: error {x:.3g} x its bound")
    if o.resid == "resid" and not (w["resid"].bits() == o.resid_bits).all():
        fails.append("resid was overwritten")
    return fails, worst


# ------------------------------------------------------------------------------------------------------------------ stand-in
def _load(win, rows, cols, ld=None, off=0):
    """rows x cols elements read as the kernel does: element (m, n) at window start + off + m ld + n of the flat allocation."""
    ld = win.ld if ld is None else ld
    idx = win.off + off + np.arange(rows)[:, None] * ld + np.arange(cols)[None, :]
    b = win.flat()[idx]
    return b.view(np.float32) if win.kind == "f32" else bf16_value(b)


def _store(win, x, ld=None, trunc=False):
    ld = win.ld if ld is None else ld
    x = np.ascontiguousarray(x, np.float32)
    idx = win.off + np.arange(x.shape[0])[:, None] * ld + np.arange(x.shape[1])[None, :]
    win.flat()[idx] = x.view(np.uint32) if win.kind == "f32" else (bf16_trunc_bits(x) if trunc else bf16_bits(x))


def standin(o, fault=None):
    """A float32 NumPy GEMM with every epilogue of dispatch_flags that reads and writes the windows of ``o`` the way the kernel
    addresses them (base + m ld + n), with the launch geometry of ``o.geom`` (K parts, strips, the split row, partial-sum tiles) and
    one ``fault`` of PERTURBED."""
    f32 = np.float32
    w, flags, g, M, N, K, K1 = o.w, o.flags, o.geom, o.M, o.N, o.K, o.K1
    Wm = _load(w["W"], N, K)
    if o.case.role == "slabs":
        taps = [_load(w["A"], M, K1, off=(o.a_row0 + s) * w["A"].ld) for s in SLAB_SHIFTS]
        A = np.concatenate(taps, 1)
    else:
        A = _load(w["A"], M, K1)
        if K1 < K:
            name, off = o.a2 if fault != "a2_through_a" else ("A", 0)
            A = np.concatenate([A, _load(w[name], M, K1, off=off)], 1)
    S = g["S"]
    edges = [p * (K // 64) // S * 64 for p in range(S + 1)]
    parts = [A[:, edges[p]:edges[p + 1]] @ Wm[:, edges[p]:edges[p + 1]].T for p in range(S)]
    if fault == "drop_k_tile":                        # the first K tile of the last K part, in the second tile row (the first of few rows)
        r0 = g["BM"] if M > g["BM"] else 0
        k0 = edges[S - 1]
        parts[S - 1][r0:r0 + g["BM"]] -= A[r0:r0 + g["BM"], k0:k0 + 64] @ Wm[:, k0:k0 + 64].T
    if fault == "strip_wrong_part" and S > 1:
        parts[0][g["m_main"]:] = parts[1][g["m_main"]:]
    acc = np.zeros((M, N), f32)
    resid = None
    if flags & R_:
        resid = _load(w[o.resid], M, N, ld=w["out_f32"].ld if fault == "resid_ld_f32" else None)
        if fault != "bf16_before_resid":
            acc = acc + resid
    for p in parts:
        acc = acc + p
    early = None
    if flags & K_:
        acc = acc + _load(w["row_add"], 1, M)[0][:, None] * _load(w["col_add"], 1, N)
    bias = _load(w["bias"], 1, N) if flags & B_ else f32(0)
    if flags & L_:
        npi = o.np_in
        split = g["split_rows"]
        p = _load(w["part_in"], M, 2 * npi).reshape(M, npi, 2)
        if fault == "part_in_no_offset" and split:
            p = np.concatenate([p[:split], p[:M - split]])
        inv_d = f32(1.0) / f32(o.norm_dim)
        dm = p[:, :, 0].sum(1, dtype=f32) * inv_d
        r = f32(1.0) / np.sqrt(np.maximum(p[:, :, 1].sum(1, dtype=f32) * inv_d - dm * dm, f32(0)) + f32(o.eps))
        if fault == "rstd_neighbour":
            r = np.roll(r, 1)
        v = acc * r[:, None] + (_load(w["colsum"], 1, N) * (-dm * r)[:, None] + bias)
        _store(w["c_out"], (_load(w["row_c"], 1, M)[0] + dm)[None, :])
    else:
        v = acc + bias if fault != "bias_after_gelu" or not flags & G_ else acc
    if flags & G_:
        v = gelu64(v.astype(np.float64)).astype(f32)
        if fault == "bias_after_gelu":
            v = v + bias
    if fault == "bf16_before_resid" and flags & R_:
        early, v = v, v + resid
    if flags & F_:
        _store(w["out_f32"], v, ld=N if fault == "out_stride_n" else None)
    if flags & H_:
        _store(w["out_bf16"], v if early is None else early, trunc=fault == "bf16_trunc")
        if fault == "store_past_n":
            w["out_bf16"].flat()[w["out_bf16"].off + (M - 1) * w["out_bf16"].ld + N + np.arange(4)] = 0
    if flags & C_:
        vc = v - _load(w["row_c"], 1, M)[0][:, None]
        _store(w["out_cen"], vc, trunc=fault == "bf16_trunc")
        if fault == "store_past_n":
            w["out_cen"].flat()[w["out_cen"].off + (M - 1) * w["out_cen"].ld + N + np.arange(4)] = 0
        BN, slots = g["BN"], g["slots"]
        part = np.zeros((M, slots, 2), f32)
        for t in range(1 if g["finish"] else slots):
            tt = (t + 1) % slots if fault == "slot_neighbour" and slots > 1 else t
            x = vc if g["finish"] else vc[:, tt * BN:(tt + 1) * BN]
            part[:, t, 0], part[:, t, 1] = x.sum(1, dtype=f32), (x * x).sum(1, dtype=f32)
        _store(w["part_out"], part.reshape(M, -1))
    if fault == "store_past_n" and flags & F_ and not flags & (H_ | C_):
        w["out_f32"].flat()[w["out_f32"].off + (M - 1) * w["out_f32"].ld + N + np.arange(4)] = 0


# fault -> (what a kernel with it does, the data sets on which a check must see it)
BOTH = ("lattice", "workflow")
PERTURBED = dict(
    out_stride_n=("an output written with row stride N in place of its ld", BOTH),
    resid_ld_f32=("resid read with ld_f32", BOTH),
    a2_through_a=("A2 read through A", BOTH),
    drop_k_tile=("one K tile of one K part dropped for one tile row", BOTH),
    strip_wrong_part=("strip rows taken from the wrong K part", BOTH),
    bf16_trunc=("a bf16 copy truncated, not rounded to nearest even", BOTH),
    bf16_before_resid=("a bf16 copy taken before the residual add", BOTH),
    slot_neighbour=("a partial-sum slot summed over the neighbouring columns", BOTH),
    part_in_no_offset=("part_in not offset in the second launch of the split form", BOTH),
    store_past_n=("a store 4 columns past N in the last row", BOTH),
    bias_after_gelu=("bias added after GELU", BOTH),
    rstd_neighbour=("rstd of the neighbouring row", BOTH),
)

# Small launches with made-up geometries for the stand-ins (the CPU test): every role, K parts, strips, the split row, a ragged last
# partial-sum tile, the finish kernel's convention.  (case, geometry)
STANDIN_CASES = [
    (_c(300, 136, 256, "plain", -1, "standin"), dict(BM=128, BN=64, slots=3, S=2, m_main=256, split_rows=0, finish=False)),
    (_c(300, 136, 256, "two-slab", -1, "standin"), dict(BM=128, BN=64, slots=3, S=1, m_main=300, split_rows=0, finish=False)),
    (_c(300, 136, 256, "two-slab-producer", -1, "standin"), dict(BM=128, BN=64, slots=3, S=2, m_main=256, split_rows=0, finish=False)),
    (_c(300, 136, 1024, "producer", -1, "standin"), dict(BM=128, BN=128, slots=2, S=2, m_main=300, split_rows=0, finish=True)),
    (_c(300, 136, 128, "consumer", -1, "standin"), dict(BM=128, BN=128, slots=2, S=1, m_main=300, split_rows=128, finish=False)),
    (_c(100, 72, 64, "slabs", -1, "standin"), dict(BM=64, BN=64, slots=2, S=1, m_main=100, split_rows=0, finish=False)),
]
