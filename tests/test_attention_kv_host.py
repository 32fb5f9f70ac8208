"""No GPU: the plan of the few-keys / many-queries attention (uspace_attention_kv_plan against its mirror and its own promises),
the kernels the library holds for it, the refusals, and that the resident kernel's bounds separate the float64 model from the
planted faults on this kernel's cases."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

from tests import attention_kv_cases as K
from uspace_amd._hip import attention_kv_plan as _feature  # noqa: F401  (every test here is about attention_kv: none passes without it)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cases_cover_what_they_must():
    cs = K.cases()
    assert {c[2] for c in cs} == set(K.LK) and {c[1] for c in cs} >= set(K.LQ) and {c[3] for c in cs} == set(K.HEADS)
    assert {(c[1], c[2]) for c in cs} >= {(lq, lk) for lq in K.LQ for lk in K.LK} and max(c[0] for c in cs) == 3
    assert [(c[1], c[3]) for c in cs[-4:]] == list(K.WORKFLOW) and all(c[2] == 256 for c in cs[-4:])
    assert {K.plan(*c[:4])["NT"] for c in cs} == {6, 17, 21}


def test_plan_mirror_and_promises():
    from uspace_amd import _hip
    g = np.random.default_rng(5)
    shapes = [c[:4] for c in K.cases()] + [(1, 16384, 256, 1), (64, 16384, 256, 1), (600, 100, 97, 1), (3, 1, 1, 1), (1, 10 ** 6, 336, 2)]
    shapes += [(int(g.integers(1, 40)), int(g.integers(1, 20000)), int(g.integers(1, 337)), int(g.integers(1, 9))) for _ in range(300)]
    for B, Lq, Lk, H in shapes:
        p = _hip.attention_kv_plan(B, Lq, Lk, H)
        assert p == K.plan(B, Lq, Lk, H), (B, Lq, Lk, H)
        n_qt = -(-Lq // 16)
        assert p["NT"] * 16 >= Lk and p["block"] == 64 * p["NW"] and p["lds"] <= 160 * 1024
        assert p["chunk"] % p["NW"] == 0 and p["chunk"] >= p["NW"]
        assert (p["nchunks"] - 1) * p["chunk"] < n_qt <= p["nchunks"] * p["chunk"] and p["grid"] == B * H * p["nchunks"]
    # one 512^2 image, stage 0: 1 024 query tiles of one head, 512 resident workgroups -> the floor of one tile per wave decides
    assert _hip.attention_kv_plan(1, 16384, 256, 1) == dict(NT=17, NW=4, chunk=4, nchunks=256, grid=256, block=256, lds=(272 + 288) * 128)
    # a batch that fills the machine by itself: one chunk per 512 / (B H) share
    assert _hip.attention_kv_plan(64, 16384, 256, 1)["nchunks"] == 8


def test_refusals_need_no_device():
    from uspace_amd import _hip
    L = _hip.lib()
    out = (ctypes.c_int * 7)()
    for B, Lq, Lk, H in ((1, 16, 337, 1), (1, 16, 0, 1), (0, 16, 16, 1), (1, 0, 16, 1), (1, 16, 16, 0)):
        assert L.uspace_attention_kv_plan(B, Lq, Lk, H, out) == -1
    assert L.uspace_attention_kv_plan(1, 16, 16, 1, None) == -1
    with pytest.raises(ValueError):
        K.plan(1, 16, 337, 1)
    buf = ctypes.create_string_buffer(8192)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 255) // 256 * 256)
    call = L.uspace_attention_kv_bf16
    assert call(p, 64, p, 128, p, 64, 1, 16, 337, 1, None) == -1                  # too many keys
    assert call(p, 64, p, 128, p, 64, 1, 16, 16, 2, None) == -1                   # rows narrower than the heads
    assert call(p, 68, p, 128, p, 64, 1, 16, 16, 1, None) == -1                   # ldq not a multiple of 8
    assert call(p, 64, p, 132, p, 64, 1, 16, 16, 1, None) == -1
    assert call(p, 64, p, 128, p, 66, 1, 16, 16, 1, None) == -1
    assert call(ctypes.c_void_p(p.value + 8), 64, p, 128, p, 64, 1, 16, 16, 1, None) == -1
    assert call(None, 64, p, 128, p, 64, 1, 16, 16, 1, None) == -1


def test_library_holds_the_four_kernels_without_scratch():
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"):
        pytest.skip("llvm-objdump not available")
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    ks = kr.kernels()
    mine = {n: k for k, n in zip(ks, kr.demangle([k["name"] for k in ks])) if "attention_kv_kernel" in n}
    assert sorted(n.split("<")[1].split(">")[0] for n in mine) == ["10, 4", "17, 4", "21, 8", "6, 4"]
    for n, k in mine.items():
        assert k["scratch"] == 0 and k["vgpr"] + k["agpr"] <= 256, (n, k)
    seg = [k for k, n in zip(ks, kr.demangle([k["name"] for k in ks]))
           if any(s in n for s in ("dwconv3x3_gelu_kernel", "bilinear_kernel", "seg_labels_kernel", "seg_pair_counts_kernel", "seg_region_sse_kernel",
                                   "seg_pack_dw_kernel", "seg_pack_cls_kernel", "seg_take_columns_kernel"))]
    assert len(seg) == 9 and all(k["scratch"] == 0 for k in seg)          # bilinear_kernel has two instantiations


@pytest.mark.parametrize("case", [c for c in K.cases() if c[1] <= 960], ids=K.case_id)
def test_bounds_separate_the_model_from_the_faults(case):
    """The rounding model lies inside the bounds against the plain float64 softmax, and every planted fault lies at least 10 x
    above the bound tied to it (per head for the faults that move a whole head, per row otherwise) on the data set meant for it."""
    B, Lq, Lk, H, data = case
    q, kv = K.make_q_kv(B, Lq, Lk, H, data)
    tight, loose = (K.per_head(K.attention_kv_f64(q, kv, H, r), H) for r in (True, False))
    assert K.head_err(tight, loose) < K.TOL["att_loose"]
    for name, applies in K.FAULTS.items():
        if not applies(case):
            continue
        bad = K.per_head(K.attention_kv_f64(q, kv, H, True, fault=name), H)
        if name in ("last_key_dropped", "last_key_doubled"):
            # one key of Lk: what it moves is its share of a row -- seen on 'flat' data with few keys, or by the row it leads
            if not (data in ("flat", "voff") and 2 <= Lk <= 17):
                continue
        if name == "scale_1/sqrtC" and data == "flat":
            continue                                           # near-uniform P does not feel the temperature
        e = K.head_err(bad, tight)
        assert e >= 10 * K.TOL["att_tight"], (name, e)
