"""The bf16 GEMM (uspace_gemm_bf16_ext / uspace_gemm_slabs_bf16) against float64 on every form the dispatcher launches, every epilogue
and strided, guarded operands: tests/gemm_cases.py holds the cases, layouts, data, references and checks, tests/test_gemm_cases.py
shows on the CPU that these checks pass fp32 arithmetic done right and fail a dozen subtly wrong kernels.

Every operand and output is a window inside a larger allocation filled with NaN canaries; after each launch every canary must be
unchanged, lattice data (small integers) must come out bit-equal to float64, Gaussian data within the worst-case bound of fp32
summation, and the two workspaces must have been written exactly by the launches listed as K-split / K-split tail."""
import ctypes

import numpy as np
import pytest
import torch

from tests import gemm_cases as GC
from tests.gemm_cases import B_, C_, F_, H_, R_, CASES

pytestmark = pytest.mark.gpu

SIGNED = {"f32": np.int32, "bf16": np.int16}
OUTPUTS = ("out_f32", "out_bf16", "out_cen", "part_out", "c_out", "resid")
WS_CANARY = GC.CANARY_F32                      # (below 2^31: the same number as an int32)
USPACE_ERR_ARG = -1


@pytest.fixture(scope="module")
def hip():
    from uspace_amd import _hip
    _hip.lib()
    return _hip


class Workspaces:
    """split_ws and sk_ws of the size the library asks for (a token size where it asks for none), refilled with NaN canaries before every
    launch, and fresh zeroed arrival counters."""

    def __init__(self, lib, c):
        M, N, K = c.M, c.N, GC.full_k(c)
        self.split = torch.empty(max(lib.uspace_gemm_split_ws_bytes(M, N, K), 1 << 16) // 4, dtype=torch.int32, device="cuda")
        self.sk = torch.empty(max(lib.uspace_gemm_sk_ws_bytes(M, N, K), 1 << 16) // 4, dtype=torch.int32, device="cuda")

    def arm(self):
        self.split.fill_(WS_CANARY)
        self.sk.fill_(WS_CANARY)
        self.counters = torch.zeros(256, dtype=torch.int32, device="cuda")

    def written(self):
        return bool((self.split != WS_CANARY).any().item()), bool((self.sk != WS_CANARY).any().item())


def launch(hip, o, ws, **override):
    """Upload the allocations of ``o``, launch on the windows inside them, download what the launch may have written.  ``override``
    replaces single arguments (the refused-argument test)."""
    lib, w = hip.lib(), o.w
    t = {n: torch.from_numpy(x.buf.view(SIGNED[x.kind])).cuda() for n, x in w.items()}

    def p(name, extra=0):
        return ctypes.c_void_p(t[name].data_ptr() + (w[name].off + extra) * w[name].itemsize) if name in w else None

    def ld(name):
        return override.get("ld_" + name, w[name].ld if name in w else 0)

    flags = o.flags
    a_ptr = override.get("A_ptr", p("A", o.a_row0 * w["A"].ld))
    M, lda = override.get("M", o.M), override.get("lda", w["A"].ld)
    out = (a_ptr, lda)
    tail = (flags, p("bias"), p(o.resid) if o.resid else None, ld(o.resid) if o.resid else 0, p("out_f32"), ld("out_f32"),
            p("out_bf16"), ld("out_bf16"))
    if o.case.role == "slabs":
        shifts = (ctypes.c_int * 9)(*GC.SLAB_SHIFTS)
        rc = lib.uspace_gemm_slabs_bf16(*out, p("W"), ld("W"), M, o.N, o.K1, 9, shifts, *tail, hip.stream_ptr())
    else:
        ext = hip.GemmExt()
        for name in ("row_c", "out_cen", "part_out", "part_in", "colsum", "c_out", "row_add", "col_add"):
            setattr(ext, name, p(name).value if name in w else None)
        ext.ld_cen, ext.np_in, ext.norm_dim, ext.eps = ld("out_cen"), getattr(o, "np_in", 0), o.norm_dim, o.eps
        ext.split_ws, ext.split_ws_bytes = ws.split.data_ptr(), ws.split.numel() * 4
        ext.sk_ws, ext.sk_ws_bytes, ext.sk_counters = ws.sk.data_ptr(), ws.sk.numel() * 4, ws.counters.data_ptr()
        a2 = (p(o.a2[0], o.a2[1]), override.get("lda", w[o.a2[0]].ld)) if o.a2 else (None, 0)
        rc = lib.uspace_gemm_bf16_ext(*out, *a2, o.K1, p("W"), ld("W"), M, o.N, o.K, *tail, ctypes.byref(ext), hip.stream_ptr())
    torch.cuda.synchronize()
    for n in OUTPUTS:
        if n in w:
            w[n].buf[...] = t[n].cpu().numpy().view(w[n].dtype)
    return rc


WORST = {}      # (form, output kind) -> the largest error over bound seen on workflow data (printed, not asserted)


@pytest.mark.parametrize("dataset", GC.DATA_SETS)
@pytest.mark.parametrize("c", CASES, ids=GC.case_id)
def test_gemm_matches_float64_on_guarded_strided_operands(hip, c, dataset):
    lib = hip.lib()
    plan = GC.plan_of(lib, c)
    assert plan[0] == c.form, plan
    ex = dict(c.expect)
    g = GC.geometry(c, plan, lib.uspace_gemm_split_ws_bytes(c.M, c.N, c.K) if "ksplit" in ex else 0)
    rows = GC.sample_rows(c, g, plan[7] if c.form == 6 else 0)
    d = GC.make_data(c, dataset)
    ws = Workspaces(lib, c)
    cache = {}
    for flags, layout in GC.launches(c):
        o = GC.build_ops(c, flags, layout, d, g)
        ws.arm()
        assert launch(hip, o, ws) == 0
        fails, worst = GC.check(o, GC.reference(c, d, flags, g, rows, cache))
        split_written, sk_written = ws.written()
        print(f"{GC.case_id(c)} {dataset} {GC.flag_name(flags)} layout {layout}: form {plan[0]}, split_ws {split_written}, sk_ws {sk_written}, "
              + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
        for k, v in worst.items():
            key = (c.form, "ksplit" if g["finish"] else "", k)
            WORST[key] = max(WORST.get(key, 0.0), v)
        assert not fails, (GC.flag_name(flags), layout, fails)
        # the workspaces are the witnesses of the two K-split forms: written by them, bit-identical after every other launch
        assert split_written == ("ksplit" in ex), (GC.flag_name(flags), layout)
        assert sk_written == (c.form == 6), (GC.flag_name(flags), layout)
    print("worst error / bound so far:", {f"form{k[0]}{k[1]} {k[2]}": float(f"{v:.3g}") for k, v in sorted(WORST.items())})


@pytest.mark.parametrize("what,flags,override", [
    ("lda & 7", B_ | R_ | F_ | H_, dict(lda=68)),
    ("ldw & 7", B_ | R_ | F_ | H_, dict(ld_W=68)),
    ("ld_f32 & 3", B_ | R_ | F_ | H_, dict(ld_out_f32=66)),
    ("ld_resid & 3", B_ | R_ | F_ | H_, dict(ld_resid=70)),
    ("ld_bf16 & 3", B_ | R_ | F_ | H_, dict(ld_out_bf16=66)),
    ("ld_cen & 3", C_ | B_ | R_ | F_, dict(ld_out_cen=66)),
    ("M lda >= 2^30", B_ | R_ | F_ | H_, dict(lda=1 << 20)),
])
def test_gemm_refuses_what_the_header_rules_out(hip, what, flags, override):
    """Row strides the ABI rules out and operands beyond its 32-bit byte offsets come back as USPACE_ERR_ARG with nothing written."""
    c = GC._c(1024, 64, 64, "producer" if flags & C_ else "plain", 5, "refused")
    g = GC.geometry(c, GC.plan_of(hip.lib(), c))
    o = GC.build_ops(c, flags, "e", GC.make_data(c, "lattice"), g)
    ws = Workspaces(hip.lib(), c)
    ws.arm()
    if what.startswith("M lda"):     # (an allocation of the whole claimed extent, so that nothing here depends on the refusal)
        big = torch.empty(1 << 30, dtype=torch.bfloat16, device="cuda")
        override = dict(override, A_ptr=ctypes.c_void_p(big.data_ptr()))
    assert launch(hip, o, ws, **override) == USPACE_ERR_ARG
    assert all(o.w[n].strays() == 0 and o.w[n].untouched() for n in OUTPUTS if n in o.w and n != "resid")
    assert o.w["resid"].strays() == 0 and np.array_equal(o.w["resid"].bits(), o.resid_bits)
    assert ws.written() == (False, False)
    assert launch(hip, o, ws) == 0                 # ... and the same operands with the strides they have are taken
