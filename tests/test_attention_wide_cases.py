"""tests/attention_wide_cases.py pinned on the CPU: the coverage of its case list, its plan mirror against uspace_attention_wide_plan of
the built library, the float64 model of the streamed arithmetic against the plain float64 softmax, the sensitivity of the bounds of
tests/test_gpu_attention_wide.py to four planted faults, the VAE workspace beyond 1 024 latent positions, and the new symbols."""
import ctypes
import importlib.util
import os
import re

import pytest
import torch

from tests import attention_wide_cases as WC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
USPACE_ERR_ARG = -1
FACTOR = 10.0          # a planted fault lies at least this many bounds away


def _threads():
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 16))
    return n


# ------------------------------------------------------------------------------------------------------------------ coverage
def test_cases_cover_the_issue_shapes():
    assert len(set(WC.CASES)) == len(WC.CASES)
    small = {(c[1], c[2]) for c in WC.CASES if c[0] == 3 and c[1] <= 129}
    assert small == {(N, C) for N in (1, 31, 32, 33, 63, 65, 129) for C in WC.WIDTHS}
    shapes = {c[:3] for c in WC.CASES}
    assert {(2, 1089, 128), (3, 1600, 256), (2, 1025, 512), (1, 4096, 512)} <= shapes
    assert [c[4] for c in WC.CASES if c[:3] == (1, 4096, 512)] == [256]
    for C in WC.WIDTHS:                                   # both rescale paths at every width
        assert {c[3] for c in WC.CASES if c[2] == C} >= {"first", "last"}
    # every branch of the plan is reachable at the N the GPU test uses for it
    assert WC.branch_batches(129) == {1: 1, 2: 52, 4: 86}
    assert [WC.plan(b, 129, 512)[2] for b in (1, 51, 52, 85, 86)] == [1, 1, 2, 2, 4]


# ------------------------------------------------------------------------------------------------------------------ plan
def test_mirror_matches_the_plan_of_the_built_library():
    from uspace_amd import _hip
    plan = _hip.lib().uspace_attention_wide_plan
    out = (ctypes.c_int * 6)()
    seen = set()
    for N in list(range(1, 300)) + [1023, 1024, 1025, 1089, 1600, 4095, 4096, 4097, 16384]:
        bb = WC.branch_batches(N)
        for B in {1, 2, 3, 8, 31, 255, 256, 257} | {b + d for b in bb.values() if b for d in (-1, 0, 1) if b + d > 0}:
            for C in WC.WIDTHS:
                assert plan(B, N, C, out) == 0, (B, N, C)
                assert tuple(out) == WC.plan(B, N, C), (B, N, C, list(out))
                assert out[5] == 256 * C <= 160 * 1024 and out[3] == B * -(-N // out[1]) and out[4] == 64 * out[2]
                seen.add(out[2])
    assert seen == {1, 2, 4}


def test_plan_and_launch_refuse_bad_arguments():
    from uspace_amd import _hip
    L_ = _hip.lib()
    out = (ctypes.c_int * 6)()
    for B, N, C in ((0, 40, 64), (1, 0, 64), (-1, 40, 64), (1, -3, 64), (1, 40, 0), (1, 40, 32), (1, 40, 96), (1, 40, 192),
                    (1, 40, 1024), (1, 40, -64), (2 ** 16, 2 ** 15, 64)):                  # B * N = 2^31
        assert L_.uspace_attention_wide_plan(B, N, C, out) == USPACE_ERR_ARG, (B, N, C)
    assert L_.uspace_attention_wide_plan(1, 40, 64, None) == USPACE_ERR_ARG
    assert L_.uspace_attention_wide_plan(2 ** 10, 2 ** 20, 512, out) == 0                  # B * N = 2^30 fits
    p = ctypes.c_void_p(4096)
    ok = dict(q=p, k=p, v=p, ld=64, out=p, ld_out=64, B=1, N=40, C=64, scale=0.125)

    def launch(**kw):                                     # refused before the GPU is touched
        a = dict(ok, **kw)
        return L_.uspace_attention_wide_bf16(a["q"], a["k"], a["v"], a["ld"], a["out"], a["ld_out"], a["B"], a["N"], a["C"],
                                             a["scale"], None)

    for bad in (dict(q=None), dict(k=None), dict(v=None), dict(out=None), dict(B=0), dict(N=0), dict(C=96), dict(ld=56), dict(ld=68),
                dict(ld_out=60), dict(ld_out=66), dict(q=ctypes.c_void_p(4104)), dict(out=ctypes.c_void_p(4100)), dict(scale=0.0),
                dict(scale=-1.0), dict(scale=float("inf")), dict(scale=float("nan")), dict(B=2 ** 16, N=2 ** 15)):
        assert launch(**bad) == USPACE_ERR_ARG, bad


def test_kernels_use_no_scratch():
    """Code-object metadata of the built library (tools/kernel_resources.py; no GPU): one instantiation per width, none with scratch,
    all compiled for 4 waves at most (one per SIMD, so each has the whole 512-entry register file); the LDS is dynamic."""
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"):
        pytest.skip("llvm-objdump not available")
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    ks = [k for k in kr.kernels() if "attn_wide_kernel" in k["name"]]
    assert len(ks) == len(WC.WIDTHS) and not any("attention_kernel" in k["name"] or "attn_stream" in k["name"] for k in ks)
    for k in ks:
        assert k["scratch"] == 0 and k["wg"] == 256 and k["lds"] == 0 and k["vgpr"] <= 512, k


# ------------------------------------------------------------------------------------------------------------------ the model
def test_model_is_the_plain_softmax_without_rounding_and_every_fault_moves_it():
    n = _threads()
    try:
        B, N, C = 3, 150, 64
        q, k, v, scale = WC.make_qkv(B, N, C, "last")
        ref, peak = WC.reference(q, k, v, B, N, C, scale)
        assert float((WC.streamed(q, k, v, B, N, C, scale, rnd=False) - ref).abs().max()) < 1e-12
        one = WC.streamed(q, k, v, B, N, C, scale, kt=N)                                  # one tile: P rounded against the row maximum
        s = WC._d(q, B, N, C) @ WC._d(k, B, N, C).transpose(1, 2) * scale
        pu = WC._bf(torch.exp(s - s.amax(-1, keepdim=True)))
        assert torch.equal(one, WC._bf(pu @ WC._d(v, B, N, C) / pu.sum(-1, keepdim=True)))
        rows = WC.sample_rows(N, 20)
        assert torch.equal(WC.streamed(q, k, v, B, N, C, scale, rows=rows), WC.streamed(q, k, v, B, N, C, scale)[:, rows])
        for f in ("mask_late", "rescale_dropped", "v_neighbour"):
            assert float((WC.streamed(q, k, v, B, N, C, scale, fault=f, rnd=False) - ref).abs().max()) > 1e-2, f
        # nothing to mask at a multiple of the key tile, nothing to rescale in one tile
        q, k, v, scale = WC.make_qkv(B, 64, C, "last")
        assert torch.equal(WC.streamed(q, k, v, B, 64, C, scale, fault="mask_late"), WC.streamed(q, k, v, B, 64, C, scale))
        q, k, v, scale = WC.make_qkv(B, 31, C, "last")
        assert torch.equal(WC.streamed(q, k, v, B, 31, C, scale, fault="rescale_dropped"), WC.streamed(q, k, v, B, 31, C, scale))
    finally:
        torch.set_num_threads(n)


def test_data_sets_are_peaked_and_put_the_maximum_where_they_say():
    n = _threads()
    try:
        for N, C in ((129, 64), (1025, 512), (65, 256)):
            for data in WC.DATA_SETS:
                q, k, v, scale = WC.make_qkv(2, N, C, data)
                s = WC._d(q, 2, N, C) @ WC._d(k, 2, N, C).transpose(1, 2) * scale
                peak = torch.softmax(s, -1).amax(-1)
                assert float(peak.median()) > 0.3, (N, C, data, float(peak.median()))
                tile = s.argmax(-1) // WC.KT
                if data == "first":
                    assert float((tile == 0).double().mean()) > 0.9
                if data == "last":
                    assert float((tile == (N - 1) // WC.KT).double().mean()) > 0.9
                    assert float((s.argmax(-1) == N - 1).double().mean()) > 0.4
        q, k, v, scale = WC.make_qkv(3, 65, 512, "constv")
        ref, peak = WC.reference(q, k, v, 3, 65, 512, scale)
        assert float(peak.min()) > 0.3
        u = WC._d(v, 3, 65, 512)
        assert float((ref - u).abs().max()) < 1e-12 and torch.equal(u, u[:, :1].expand_as(u))
    finally:
        torch.set_num_threads(n)


_SMALL = [c for c in WC.CASES if c[1] <= 129]


@pytest.mark.parametrize("C", WC.WIDTHS)
def test_streamed_model_stays_under_the_ceiling_and_the_gpu_bounds(C):
    """The model's own distance from the plain float64 softmax, per width over the small cases: under the analytic ceiling, and under
    the GPU test's bounds (3 x what the kernel measured) -- the kernel is that arithmetic with fp32 logits."""
    n = _threads()
    try:
        rel = ma = 0.0
        for B, N, Cc, data, _ in _SMALL:
            if Cc != C:
                continue
            q, k, v, scale = WC.make_qkv(B, N, C, data)
            ref, _ = WC.reference(q, k, v, B, N, C, scale)
            got = WC.streamed(q, k, v, B, N, C, scale)
            rel, ma = max(rel, WC.rel_l2(got, ref)), max(ma, WC.max_abs(got, ref, v, B, N, C))
        print(f"\n[model C={C}] rel={rel:.3e} maxabs={ma:.3e} bounds={WC.bounds(C)}")
        assert ma <= WC.CEILING, (rel, ma)
        assert rel <= WC.bounds(C)[0] and ma <= WC.bounds(C)[1], (rel, ma, WC.bounds(C))
    finally:
        torch.set_num_threads(n)


# ------------------------------------------------------------------------------------------------------------------ sensitivity
@pytest.mark.parametrize("C", WC.WIDTHS)
@pytest.mark.parametrize("fault", WC.FAULTS)
def test_every_fault_lands_beyond_ten_bounds(fault, C):
    """What a kernel with the fault would store (the model with the fault planted) against the GPU test's reference, in the GPU test's
    metrics, on the data set meant to expose it: at least 10 x the bound.  'unrounded_sum' moves a row by 2^-8 at most, which no bound
    above the output's own rounding can see; the 'constv' set, whose bound is exact equality, does: the faulty result must differ."""
    n = _threads()
    try:
        B, N = 3, 65
        if fault == "unrounded_sum":
            q, k, v, scale = WC.make_qkv(B, N, C, "constv")
            u = WC._d(v, B, N, C)
            assert torch.equal(WC.streamed(q, k, v, B, N, C, scale), u)                   # the sound arithmetic: u, bit for bit
            bad = WC.streamed(q, k, v, B, N, C, scale, fault=fault)
            wrong = int((bad != u).sum())
            print(f"\n[sensitivity {fault} C={C}] elements off u: {wrong} of {u.numel()}, maxabs={WC.max_abs(bad, u, v, B, N, C):.3e} (bound 0)")
            assert wrong >= 20               # a whole bf16 ulp each, where the common P rounds far enough and u's mantissa is large
            return
        q, k, v, scale = WC.make_qkv(B, N, C, "last")
        ref, _ = WC.reference(q, k, v, B, N, C, scale)
        bad = WC.streamed(q, k, v, B, N, C, scale, fault=fault)
        b_rel, b_ma = WC.bounds(C)
        r_rel, r_ma = WC.rel_l2(bad, ref) / b_rel, WC.max_abs(bad, ref, v, B, N, C) / b_ma
        print(f"\n[sensitivity {fault} C={C}] rel / bound = {r_rel:.3g}, maxabs / bound = {r_ma:.3g}")
        assert min(r_rel, r_ma) >= FACTOR, (r_rel, r_ma)
    finally:
        torch.set_num_threads(n)


# ------------------------------------------------------------------------------------------------------------------ workspace
def _vae_cfg(ch, mult, nrb, res):
    from uspace_amd import _hip
    return _hip.VaeConfig(ch, (ctypes.c_int * 4)(*(list(mult) + [0] * (4 - len(mult)))), len(mult), nrb, res)


def test_vae_workspace_grows_linearly_beyond_1024_latent_positions():
    """Where the wide kernel is taken the workspace holds no [HW, HW] buffer.  At the two-level configuration of
    tests/test_gpu_vae_anysize.py the whole workspace is below what the HW^2 * 6 bytes of S and P alone would be, at 512 and at 1 024;
    at the SD configuration (three upsamples: the 128-channel full-size maps alone outweigh HW^2 * 6 at 512^2) it grows by the ratio
    of the maps, 4, from 512 to 1 024 -- with the quadratic term it would be 6."""
    from uspace_amd import _hip
    L_ = _hip.lib()
    for fn in (L_.uspace_vae_workspace_bytes, L_.uspace_vae_enc_workspace_bytes):
        for res in (512, 1024):
            hw = (res // 2) ** 2
            total = fn(ctypes.byref(_vae_cfg(64, (1, 2), 1, res)), 1)
            assert 0 < total < hw * hw * 6, (res, total)
        sd = [fn(ctypes.byref(_vae_cfg(128, (1, 2, 4, 4), 2, res)), 1) for res in (256, 512, 1024)]
        assert sd[0] > (32 * 32) ** 2 * 6                                                  # 1 024 tokens keep S and P
        assert 3.9 < sd[2] / sd[1] < 4.05, sd
        assert sd[1] < 4.05 * sd[0], sd


# ------------------------------------------------------------------------------------------------------------------ symbols
def test_new_symbols_are_declared_and_bound():
    from uspace_amd import _hip
    header = open(os.path.join(ROOT, "include", "uspace_hip.h")).read()
    assert re.search(r"#define USPACE_ABI_VERSION 11\b", header)
    for name in ("uspace_attention_wide_bf16", "uspace_attention_wide_plan"):
        assert re.search(r"USPACE_API int " + name + r"\(", header), name
        assert callable(getattr(_hip.lib(), name))
    assert re.search(r"uspace_attention_wide_bf16\(const uint16_t\* q, const uint16_t\* k, const uint16_t\* v, int ld,\s+"
                     r"uint16_t\* out, int ld_out, int B, int N, int C, float scale,\s+uspace_stream_t stream\);", header)
