"""Launches of the two-stage 256 x 256 form of the bf16 GEMM (uspace_amd/csrc/gemm.hip) whose output bits are pinned: a helper of
tests/golden/make_gemm_epilogue_digests.py (records them) and tests/test_gpu_gemm_epilogue_bits.py (holds the kernel to them), not a
test.  The epilogue of that form may change how it stores (which lanes write which 16 bytes, cache policy) and when it starts (under
the MFMAs of the last K tile; profiles/epilogue_forms.md); it may not change a bit of any output.

Shapes.  The smallest [M, N] for which uspace_gemm_plan_k answers "form 0, 256 x 256 tiles" for K = 128 and K = 4096, producers and
the other roles alike (found on the host by scanning M = 256 r and M = 256 r + 64 for N = 256 ... 2048; `check_plan` asserts it
again).  N = 1024 so that K = 4096 >= 4 N, the fc2 geometry (the condition of the whole-line fp32 stores that were measured and dropped):
    16448 x 1024   64 x 4 tiles, one round of the 256 CUs, 64 remainder rows = 4 strips (the super-tile block order; owner and
                   strip-free role bodies)
    13568 x 1024   53 x 4 tiles, no remainder rows (the smallest M without; the plain block order)
    32832 x 1024   128 x 4 tiles = two rounds, 4 strips: both role bodies and second-round workgroups
K = 128 and 4096: 2 and 64 K tiles, so the peeled last K tile follows a peeled and a steady-state tile.

Flag sets: the six epilogues a folded U-ViT forward launches on this form and the GELU epilogue of the unfolded one.  Every operand
and output is a window inside a NaN-canary allocation with guard rows (tests/gemm_cases.py); the layouts keep the 16-byte bf16 stores
(the interior path), residual epilogues also run in place, as the forward does."""
import ctypes
import functools
import hashlib

import numpy as np

from tests import gemm_cases as GC
from tests.gemm_cases import B_, C_, F_, G_, H_, K_, L_, R_

SHAPES = ((16448, 1024, 4), (13568, 1024, 0), (32832, 1024, 4))          # M, N, remainder strips
KS = (128, 4096)
FLAG_SETS = (
    (L_ | B_ | H_, "consumer", ("b",)),                      # qkv
    (L_ | B_ | G_ | H_, "consumer", ("b",)),                 # fc1
    (C_ | B_ | R_ | F_, "producer", ("b", "a")),             # proj / fc2 feeding a norm
    (B_ | R_ | F_ | H_, "plain", ("b", "a")),                # fc2 with the bf16 copy
    (B_ | R_ | F_, "plain", ("b", "a")),                     # fc2
    (K_ | C_ | B_ | F_, "two-slab-producer", ("b",)),        # skip_linear, two slabs
    (B_ | G_ | H_, "plain", ("b",)),                         # fc1 of the unfolded forward
)
PARAMS = [(M, N, K, fi) for (M, N, _) in SHAPES for K in KS for fi in range(len(FLAG_SETS))]
OUT_NAMES = ("out_f32", "out_bf16", "out_cen", "part_out", "c_out")


def param_id(p):
    M, N, K, fi = p
    return f"{M}x{N}x{K}-{GC.flag_name(FLAG_SETS[fi][0])}"


def case_of(p):
    M, N, K, fi = p
    return GC._c(M, N, K, FLAG_SETS[fi][1], 0, "epilogue")


def check_plan(lib, p):
    """The launch takes the two-stage 256 x 256 form (with the strips of SHAPES); returns out[8] of uspace_gemm_plan_k."""
    M, N, K, fi = p
    strips = dict((s[:2], s[2]) for s in SHAPES)[(M, N)]
    out = (ctypes.c_int * 8)()
    for producer in (0, 1):
        assert lib.uspace_gemm_plan_k(M, N, K, producer, out) == 0
        assert (out[0], out[2], out[3], out[6]) == (0, 256, 256, strips), (p, producer, list(out))
    assert lib.uspace_gemm_plan_k(M, N, K, int(GC.is_producer(case_of(p))), out) == 0
    return list(out)


@functools.lru_cache(maxsize=1)
def make_data(M, N, K):
    """Seeded operands for every role of one [M, N, K] (bf16-rounded Gaussians at the scale of the operator tests, rows with differing
    means in the residual, the statistics of a LayerNorm producer for the consumers), shared by the flag sets.  One set is cached (up
    to 0.7 GB): whoever runs the cases ends with ``make_data.cache_clear()``."""
    g = np.random.default_rng(1000003 * M + 1009 * N + 17 * K)
    d = {"dataset": "workflow"}      # (the key gemm_cases.reference reads to tell Gaussian from lattice data; build_ops takes the same dict)
    d["A"] = GC.bf16_round(g.standard_normal((M, K), np.float32))
    d["W"] = GC.bf16_round(g.standard_normal((N, K), np.float32) * np.float32(0.1))
    d["bias"] = g.standard_normal(N, np.float32)
    mean = g.standard_normal((M, 1), np.float32) * np.float32(2.0)
    d["resid"] = g.standard_normal((M, N), np.float32) * np.float32(1.5) + mean
    d["row_c"] = (mean[:, 0] + np.float32(0.05) * g.standard_normal(M, np.float32)).astype(np.float32)
    d["row_add"], d["col_add"] = g.standard_normal(M, np.float32) * np.float32(3.0), d["W"][:, K // 2:].sum(1).astype(np.float32)
    npi = 1 + M % 8
    wq = g.random((M, npi)) + 0.1
    wq /= wq.sum(1, keepdims=True)
    var = 0.5 + 2.0 * g.random(M)
    dm = (g.random(M) * 0.6 - 0.3) * np.sqrt(var)
    d["part_in"] = np.stack([(K * dm)[:, None] * wq, (K * (var + dm * dm))[:, None] * wq], 2).astype(np.float32)
    d["colsum"] = d["W"].sum(1).astype(np.float32)
    return d


def run(p):
    """The launches of one parameter set.  Returns {layout: dict(fails=[...], digests={output: sha256 hex})}: canaries that changed,
    outputs left unwritten or a separate residual overwritten, and the digest of every output window."""
    from uspace_amd import _hip
    from tests.test_gpu_gemm_parity import Workspaces, launch
    lib = _hip.lib()
    M, N, K, fi = p
    flags, _, layouts = FLAG_SETS[fi]
    c = case_of(p)
    geom = GC.geometry(c, check_plan(lib, p))
    d = make_data(M, N, K)
    ws = Workspaces(lib, c)
    res = {}
    for layout in layouts:
        o = GC.build_ops(c, flags, layout, d, geom)
        ws.arm()
        assert launch(_hip, o, ws) == 0
        assert ws.written() == (False, False)
        strays = {name: win.strays() for name, win in o.w.items()}
        fails = [f"{name}: {n} canaries changed" for name, n in strays.items() if n]
        if o.resid == "resid" and not (o.w["resid"].bits() == o.resid_bits).all():
            fails.append("resid was overwritten")
        digests = {}
        for name in OUT_NAMES:
            if name in o.w:
                bits = o.w[name].bits()
                n_left = int((bits == o.w[name].canary).sum())
                if n_left:
                    fails.append(f"{name}: {n_left} elements still hold the canary")
                digests[name] = hashlib.sha256(bits.tobytes()).hexdigest()
        res[layout] = dict(fails=fails, digests=digests)
    return res
