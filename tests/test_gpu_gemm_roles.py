"""The two roles of a workgroup in a 256 x 256 GEMM launch with remainder rows (uspace_amd/csrc/gemm.hip, "XTRA"): the workgroups of a
few tile rows own a 16-row strip besides their tile, the others own none.  gemm_kernel compiles the tile once per role (the strip
owner's body, the strip-free body) and picks one per workgroup; profiles/strip_roles.md.

Role equality.  The rows of every tile row that owns a strip are made copies of the rows of a tile row that owns none, operand by
operand (activations, residual, per-row LayerNorm values); every output of the two tile rows -- fp32, bf16, the centred copy, the
per-row partial sums, c_out -- must then be the same bits, whichever role computed it.  The strip rows, and the tile rows compared,
are also held to float64 with the bounds of tests/gemm_cases.py, every operand inside NaN-canary guards.

Same bits as before.  sha256 of every output window of every launch equals tests/golden/gemm_strip_launch_bits.npz, recorded with
tests/golden/make_gemm_strip_launch_bits.py from commit 4323b82, the commit before the role bodies (one body, a second copy of the
K loop in the store-only epilogues, run-time tests in the residual ones): the role bodies are bit-equal to it, and a later change to
the strip code that is meant to be bit-equal is held to it as well.  (A first form of the owner's strip epilogue was not: batched for
LayerNorm producers too, it left other bits on 21776 x 516 x 64, C|B|R|F, 16-byte stores, a full strip.)  The digests pin the arithmetic as this toolchain compiles it; re-record them with a toolchain that contracts
the epilogue's multiply-adds differently.

Shapes: form 0 with strips as the `0-strip` cases of tests/gemm_cases.py (85 x 3 tiles, the last tile column ragged) with 1, 16 and
17 remainder rows (one partial strip, one full, two), and the headline geometry 64 x 4 tiles + 64 rows (the super-tile block order,
owners in tile rows 0, 8, 16, 24).  K = 64 (a single K tile) and 192; the two-slab launch needs K = 2 K1 with K1 a power of two and a
multiple of 64, so it runs K = 128 (a single K tile per slab) and 256.  Each epilogue runs on a layout that keeps the 16-byte bf16
stores and on one that rules them out."""
import functools
import hashlib
import os

import numpy as np
import pytest

from tests import gemm_cases as GC
from tests.gemm_cases import B_, C_, F_, G_, H_, K_, L_, R_

pytestmark = pytest.mark.gpu

GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_strip_launch_bits.npz")
BM = 256
# (flags, role of tests/gemm_cases.py, the two layouts: 16-byte bf16 stores allowed / ruled out -- an epilogue without bf16 outputs
# runs in place and with a separate residual instead)
FLAG_SETS = (
    (L_ | B_ | H_, "consumer", ("b", "c")),                  # qkv
    (L_ | B_ | G_ | H_, "consumer", ("b", "d")),             # fc1
    (C_ | B_ | R_ | F_, "producer", ("b", "c")),             # proj / fc2 feeding a norm
    (B_ | R_ | F_ | H_, "plain", ("b", "d")),                # fc2 with the bf16 copy
    (B_ | R_ | F_, "plain", ("a", "e")),                     # fc2
    (K_ | C_ | B_ | F_, "two-slab-producer", ("b", "c")),    # skip_linear, two slabs
)
SHAPES = ((21761, 516), (21776, 516), (21777, 516), (16448, 1024))      # 1, 16, 17 remainder rows; 64 on the super-tile grid
PARAMS = [(M, N, ki, fi) for (M, N) in SHAPES for ki in ((0, 1) if N == 516 else (0,)) for fi in range(len(FLAG_SETS))]
OUT_NAMES = ("out_f32", "out_bf16", "out_cen", "part_out", "c_out")


def k_of(role, ki):
    return ((128, 256) if role.startswith("two-slab") else (64, 192))[ki]


def param_id(p):
    M, N, ki, fi = p
    flags, role, _ = FLAG_SETS[fi]
    return f"{M}x{N}x{k_of(role, ki)}-{GC.flag_name(flags)}"


def owner_tile_rows(tiles_m, n_strip):
    """The tile rows whose workgroups own a strip (the kernel's strip_of_tile_row is below n_strip)."""
    sk = (lambda t: (t & 7) * (tiles_m >> 3) + (t >> 3)) if tiles_m % 8 == 0 else (lambda t: t)
    return [t for t in range(tiles_m) if sk(t) < n_strip]


def role_data(c, owners, src):
    """make_data of the case with the rows of every owner tile row replaced by those of tile row ``src`` (copies: the cached arrays
    of make_data stay as they are)."""
    d = dict(GC.make_data(c, "workflow"))
    for name in ("A", "resid", "row_c", "row_add", "part_in"):
        if name in d and d[name].shape[0] == c.M:
            x = d[name].copy()
            for t in owners:
                x[t * BM:(t + 1) * BM] = x[src * BM:(src + 1) * BM]
            d[name] = x
    return d


@functools.lru_cache(maxsize=None)
def outcome(p):
    """Run the launches of one parameter set once.  Returns {layout: dict(fails, unequal, digest)}: the float64 / canary failures, the
    outputs on which an owner tile row differs from its source, and the sha256 of every output window."""
    from uspace_amd import _hip
    from tests.test_gpu_gemm_parity import Workspaces, launch
    lib = _hip.lib()
    M, N, ki, fi = p
    flags, role, layouts = FLAG_SETS[fi]
    c = GC._c(M, N, k_of(role, ki), role, 0, "roles", strip=True)
    plan = GC.plan_of(lib, c)
    assert plan[0] == 0 and plan[2] == BM and plan[3] == 256 and plan[6] > 0, plan       # form 0, 256 x 256 tiles, strips
    tiles_m, n_strip = plan[4], plan[6]
    owners = owner_tile_rows(tiles_m, n_strip)
    assert len(owners) == n_strip and tiles_m * BM + 16 * (n_strip - 1) < M <= tiles_m * BM + 16 * n_strip
    src = next(t for t in range(tiles_m) if t not in owners)
    g = GC.geometry(c, plan)
    d = role_data(c, owners, src)
    rows = np.unique(np.concatenate([np.arange(t * BM, (t + 1) * BM) for t in owners + [src]] + [np.arange(tiles_m * BM, M)]))
    ws = Workspaces(lib, c)
    res, cache = {}, {}
    for layout in layouts:
        o = GC.build_ops(c, flags, layout, d, g)
        ws.arm()
        assert launch(_hip, o, ws) == 0
        fails, worst = GC.check(o, GC.reference(c, d, flags, g, rows, cache))
        assert ws.written() == (False, False)
        outs = {}
        for n in OUT_NAMES:
            if n in o.w:
                b = o.w[n].bits()
                outs[n] = b.reshape(M, -1) if n != "c_out" else b.reshape(M, 1)
        unequal = [f"{n}: tile row {t} differs from tile row {src} in {int((x[t * BM:(t + 1) * BM] != x[src * BM:(src + 1) * BM]).sum())} elements"
                   for n, x in outs.items() for t in owners if not np.array_equal(x[t * BM:(t + 1) * BM], x[src * BM:(src + 1) * BM])]
        h = hashlib.sha256()
        for n, x in outs.items():
            h.update(n.encode())
            h.update(np.ascontiguousarray(x).tobytes())
        print(f"{param_id(p)} layout {layout}: owners {owners} source {src}, " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
        res[layout] = dict(fails=fails, unequal=unequal, digest=np.frombuffer(h.digest(), np.uint8))
    return res


def golden_key(p, layout):
    return f"{param_id(p)}-{layout}"


@pytest.mark.parametrize("p", PARAMS, ids=param_id)
def test_strip_owners_and_the_other_workgroups_compute_the_same_bits(p):
    for layout, r in outcome(p).items():
        assert not r["fails"], (layout, r["fails"])              # strip rows and the compared tile rows against float64; canaries
        assert not r["unequal"], (layout, r["unequal"])


@pytest.mark.parametrize("p", PARAMS, ids=param_id)
def test_outputs_are_the_recorded_bits(p):
    golden = np.load(GOLDEN_FILE)
    for layout, r in outcome(p).items():
        assert np.array_equal(r["digest"], golden[golden_key(p, layout)]), (layout, "outputs differ from the recorded ones")
