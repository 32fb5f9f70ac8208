"""CPU-only checks of the memorisation primitives: the inputs and float64 references of tests/neighbor_cases.py (the gap condition
that lets the GPU test demand exact indices, a hand-computed example, planted faults), the host logic of
uspace_amd/tools/neighbors.py and the ABI surface of uspace_metric_topk."""
import ctypes
import importlib.util
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import metric_cases as MC
from tests import neighbor_cases as NC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------- the cases
@pytest.mark.parametrize("case", MC.CASES, ids=str)
def test_gap_condition(case):
    """A condition on the inputs, not a tolerance: among every row's first k + 1 neighbours, k up to 16, consecutive distances lie
    at least 1000 selection ceilings apart in all three directions, and every authenticity decision has a relative gap of at
    least 1e-4.  A case that breaks it is replaced, not skipped."""
    real, fake = MC.sets_of(case)
    gaps = [NC.check_gaps(fake, real, NC.K_MAX), NC.check_gaps(real, real, NC.K_MAX, self_base=0), NC.check_gaps(real, fake, NC.K_MAX)]
    a = NC.ref_authenticity(fake, real)
    print(f"{case}: smallest gap in ceilings {min(gaps):.3e}, smallest authenticity gap {a['gap']:.3e}, authentic {a['pct']:.1f} %")
    assert a["gap"] >= NC.MIN_AUTH_GAP
    assert 20.0 < a["pct"] < 60.0                                  # neither outcome is trivial
    for k in NC.ks_of(case):
        assert NC.gap_ceilings(fake, real, k) >= min(gaps)         # fewer neighbours: fewer gaps


def test_edge_cases_meet_the_gap_condition_and_take_the_paths_they_are_named_for():
    edges = NC.edge_cases()
    for name, (x, y, k, index_base, self_base) in edges.items():
        NC.check_gaps(x, y, k, self_base, index_base)
    assert len(edges["ny_below_k"][1]) < edges["ny_below_k"][2]
    assert len(edges["ny_1"][1]) == 1 and len(edges["nx_1"][0]) == 1 and edges["F_1"][0].shape[1] == 1
    assert edges["F_3"][0].shape[1] == 3 and edges["F_66"][0].shape[1] == 66                     # F % 4 != 0: scalar loads
    d2, idx = NC.ref_topk(*edges["ny_below_k"][:3])
    assert np.isposinf(d2[:, 3:]).all() and (idx[:, 3:] == -1).all() and np.isfinite(d2[:, :3]).all()
    x, y, k, index_base, self_base = edges["self_on_a_shard"]
    assert index_base > 0 and self_base > index_base
    d2, idx = NC.ref_topk(x, y, k, index_base, self_base)
    assert (idx != (self_base + np.arange(len(x)))[:, None]).all() and (d2 > 0).all() and idx.min() >= index_base
    q, bank = NC.duplicate_bank()
    NC.check_gaps(q, bank, NC.K_MAX)
    for group in NC.DUP_COLUMNS:
        assert all((bank[c] == bank[group[0]]).all() for c in group)
    assert len({c // 128 for c in NC.DUP_COLUMNS[0]}) == 3 and len({c // 128 for c in NC.DUP_COLUMNS[1]}) == 1
    assert list(np.argsort(NC.arrival_key(np.array(NC.DUP_COLUMNS[1])))) == [1, 2, 0]            # met as 144, 240, 129
    idx = NC.ref_topk(q, bank, 3)[1]
    assert all(tuple(idx[i]) == NC.DUP_COLUMNS[i % 2] for i in range(12))
    q, bank, copies = NC.exact_copy_case()
    d2, idx = NC.ref_topk(q, bank, 1)
    assert (d2[:len(copies), 0] == 0.0).all() and tuple(idx[:len(copies), 0]) == copies and (d2[len(copies):] > 0).all()


def test_hand_made_example():
    """Four training points, five generated and three held-out ones in the plane; every number is in the comments of
    tests/neighbor_cases.py and can be read off by eye."""
    d2, idx = NC.ref_topk(NC.HAND_FAKE, NC.HAND_TRAIN, 2)
    assert d2[:, 0].tolist() == NC.HAND_L_FAKE and idx[:, 0].tolist() == [0, 1, 2, 3, 0]
    assert d2[4].tolist() == [4, 4] and idx[4].tolist() == [0, 1]                                 # a tie: the smaller index first
    d2, idx = NC.ref_topk(NC.HAND_TRAIN, NC.HAND_TRAIN, 1, self_base=0)
    assert d2[:, 0].tolist() == [16, 16, 100, 100] and idx[:, 0].tolist() == [1, 0, 0, 2]
    a = NC.ref_authenticity(NC.HAND_FAKE, NC.HAND_TRAIN)
    assert a["authentic"].tolist() == [False, True, False, True, False] and a["pct"] == 40.0
    l_test = NC.ref_topk(NC.HAND_TEST, NC.HAND_TRAIN, 1)[0][:, 0]
    assert l_test.tolist() == NC.HAND_L_TEST
    assert NC.ref_u(NC.HAND_L_FAKE, l_test) == NC.HAND_U == 6.0 and NC.ref_u(NC.HAND_L_FAKE, l_test, "u_without_ties") == 5.0
    assert NC.ref_zu(NC.HAND_L_FAKE, l_test) == pytest.approx(-1.5 / np.sqrt(11.25), rel=1e-15)
    from uspace_amd.tools.neighbors import mann_whitney_z
    assert mann_whitney_z(NC.HAND_L_FAKE, l_test) == pytest.approx(-1.5 / np.sqrt(11.25), rel=NC.Z_RTOL)


def _moved(good, bad, F):
    """Does the faulty (d2, idx) fall outside what the GPU test accepts around the true one?"""
    if bad[0].shape != good[0].shape or (bad[1] != good[1]).any():
        return True
    fin = np.isfinite(good[0])
    if (np.isfinite(bad[0]) != fin).any():
        return True
    return bool((np.abs(bad[0][fin] - good[0][fin]) > NC.refined_bound(good[0][fin], F)).any())


def test_planted_faults_move_the_results():
    """Every planted fault moves at least one result of the case named for it beyond the bounds of the GPU test."""
    edges = NC.edge_cases()
    q, bank = NC.duplicate_bank()
    cq, cbank, _ = NC.exact_copy_case()
    real0, fake0 = MC.sets_of(MC.CASES[0])
    named = {
        "self_included": (edges["self_on_a_shard"], edges["self_whole_set"]),
        "ties_by_arrival": ((q, bank, 1, 0, -1), (q, bank, 3, 0, -1)),
        "index_base_dropped": (edges["F_66"], edges["self_on_a_shard"]),
        "kth_is_k_plus_1": ((fake0, real0, 1, 0, -1), (fake0, real0, 16, 0, -1), edges["ny_below_k"]),
        "rows_columns_swapped": ((fake0, real0, 3, 0, -1), tuple(MC.sets_of(MC.CASES[5])[::-1]) + (5, 0, -1)),     # 257 x 300; 64 x 64
        "unrefined": ((cq, cbank, 1, 0, -1),),
    }
    assert set(named) == set(NC.TOPK_FAULTS)
    for fault, cases in named.items():
        for x, y, k, index_base, self_base in cases:
            good = NC.ref_topk(x, y, k, index_base, self_base)
            assert _moved(good, NC.ref_topk(x, y, k, index_base, self_base, fault=fault), x.shape[1]), (fault, k)
            assert not _moved(good, NC.ref_topk(x, y, k, index_base, self_base), x.shape[1])
    # the copy that the Gram value misses: 1e-13 where 0.0 is demanded
    bad = NC.ref_topk(cq[:5], cbank, 1, fault="unrefined")[0][:, 0]
    assert (bad >= 0).all() and (bad > 0).any() and bad.max() < 1e-10
    for case in MC.CASES:
        real, fake = MC.sets_of(case)
        good, bad = NC.ref_authenticity(fake, real), NC.ref_authenticity(fake, real, "auth_radius_of_query")
        assert (good["authentic"] != bad["authentic"]).any() and good["pct"] != bad["pct"], case
        fake, test, train, cells = NC.copying_sets(case)
        l_fake, l_test = NC.ref_topk(fake, train, 1)[0][:, 0], NC.ref_topk(test, train, 1)[0][:, 0]
        NC.check_rank_gaps(l_fake, l_test)
        assert (l_fake[:4] == l_test[:4]).all()                    # the planted ties
        z, z_bad = NC.ref_zu(l_fake, l_test), NC.ref_zu(l_fake, l_test, "u_without_ties")
        assert abs(z - z_bad) > 1e6 * NC.Z_RTOL * abs(z), case
        if case[0] != 4:
            kept = [c for c in range(3) if (cells[0] == c).sum() >= NC.MIN_CELL and (cells[1] == c).sum() >= NC.MIN_CELL]
            assert kept and len(kept) < len(np.unique(cells[2]))   # min_cell drops a cell
            zc = NC.ref_zu_cells(l_fake, l_test, cells, NC.MIN_CELL)
            assert abs(zc - z) > 1e-3 and abs(zc - NC.ref_zu_cells(l_fake, l_test, cells, NC.MIN_CELL, "u_without_ties")) > 1e-6


# ------------------------------------------------------------------------------------------- host logic
def test_mann_whitney_and_cells_on_the_host():
    from uspace_amd.tools.neighbors import mann_whitney_z
    rng = np.random.default_rng(0)
    for m, n in ((1, 1), (5, 3), (40, 60)):
        a, b = rng.integers(0, 12, m).astype(np.float64), rng.integers(0, 12, n).astype(np.float64)      # many ties
        want = NC.ref_zu(a, b)
        assert abs(mann_whitney_z(a, b) - want) <= NC.Z_RTOL * abs(want) + 1e-300
    assert mann_whitney_z([1.0, 2.0], [3.0, 4.0]) < 0 < mann_whitney_z([3.0, 4.0], [1.0, 2.0])
    assert mann_whitney_z([1.0, 1.0], [1.0, 1.0]) == 0.0
    with pytest.raises(ValueError):
        mann_whitney_z([], [1.0])


def test_shard_merge_on_hand_written_lists():
    from uspace_amd.tools.neighbors import merge_topk
    inf = float("inf")
    d_a = torch.tensor([[1.0, 4.0, 4.0], [0.0, inf, inf], [inf, inf, inf]], dtype=torch.float64)
    i_a = torch.tensor([[7, 2, 9], [3, -1, -1], [-1, -1, -1]], dtype=torch.int32)
    d_b = torch.tensor([[0.5, 4.0, 6.0], [0.0, 2.0, inf], [inf, inf, inf]], dtype=torch.float64)
    i_b = torch.tensor([[130, 128, 129], [200, 201, -1], [-1, -1, -1]], dtype=torch.int32)
    d, i = merge_topk(d_a, i_a, d_b, i_b, 3)
    assert d.dtype == torch.float64 and i.dtype == torch.int32
    assert d.tolist() == [[0.5, 1.0, 4.0], [0.0, 0.0, 2.0], [inf, inf, inf]]
    assert i.tolist() == [[130, 7, 2], [3, 200, 201], [-1, -1, -1]]
    d, i = merge_topk(d_b, i_b, d_a, i_a, 3)                      # the order of the shards does not matter: ties go by index
    assert i.tolist() == [[130, 7, 2], [3, 200, 201], [-1, -1, -1]]
    d, i = merge_topk(d_a, i_a, d_b, i_b, 5)
    assert i[0].tolist() == [130, 7, 2, 9, 128] and d[0].tolist() == [0.5, 1.0, 4.0, 4.0, 4.0]


def _cpu_sets(F=8):
    g = torch.Generator().manual_seed(0)
    return torch.randn(20, F, generator=g), torch.randn(12, F, generator=g), torch.randn(30, F, generator=g)


def test_value_errors_come_before_any_device_work(tmp_path):
    from uspace_amd.tools import neighbors as N
    fake, test, train = _cpu_sets()
    for k in (0, 17, 1.5):
        with pytest.raises(ValueError):
            N.nearest_neighbors(fake, train, k=k)
    with pytest.raises(ValueError):
        N.nearest_neighbors(fake, train[:, :4])
    with pytest.raises(ValueError):
        N.nearest_neighbors(fake, train, exclude_self=True)       # 20 rows against 30: not one set
    for rows in (0, -1, 2.5):
        with pytest.raises(ValueError):
            N.nearest_neighbors(fake, train, shard_rows=rows)
    with pytest.raises(ValueError):
        N.nearest_neighbors(torch.zeros(7), train)
    with pytest.raises(ValueError):
        N.authenticity(fake, train[:1])                           # a single training sample has no other one
    with pytest.raises(ValueError):
        N.authenticity(fake[:, :4], train)
    with pytest.raises(ValueError):
        N.copying_zscore(fake, test[:, :4], train)
    cells = (np.zeros(20, np.int64), np.zeros(12, np.int64), np.zeros(30, np.int64))
    with pytest.raises(ValueError):
        N.copying_zscore(fake, test, train, cells=cells[:2])
    with pytest.raises(ValueError):
        N.copying_zscore(fake, test, train, cells=(cells[0], cells[1][:5], cells[2]))
    with pytest.raises(ValueError):
        N.copying_zscore(fake, test, train, cells=(cells[0], cells[1].astype(np.float64), cells[2]))
    with pytest.raises(ValueError):
        N.copying_zscore(fake, test, train, cells=cells, min_cell=13)            # the only cell holds 12 test samples
    with pytest.raises(ValueError):
        N.copying_zscore(fake, test, train, cells=cells, min_cell=0)
    with pytest.raises(ValueError):
        N.neighbor_grid(torch.zeros(2, 3, 8, 8), torch.zeros(5, 3, 8, 8), np.zeros((3, 2), np.int64), str(tmp_path / "g.png"))
    with pytest.raises(ValueError):
        N.neighbor_grid(torch.zeros(2, 3, 8, 8), torch.zeros(5, 3, 8, 8), np.full((2, 2), 5), str(tmp_path / "g.png"))
    with pytest.raises(ValueError):
        N.neighbor_grid(torch.zeros(2, 3, 8, 8), torch.zeros(5, 3, 4, 4), np.zeros((2, 2), np.int64), str(tmp_path / "g.png"))
    with pytest.raises(ValueError):
        N.calculate_memorization_given_paths(("/nonexistent/a",), device="cpu")
    with pytest.raises(ValueError):
        N.calculate_memorization_given_paths(("/nonexistent/a", "/nonexistent/b"), device="cpu", k=17)
    with pytest.raises(RuntimeError):
        N.calculate_memorization_given_paths(("/nonexistent/a", "/nonexistent/b"), device="cpu")
    assert not os.path.exists(str(tmp_path / "g.png"))


def test_cpu_tensors_raise_uspace_hip_error():
    """Valid arguments on the CPU get as far as the kernel call's device check: there is no CPU path."""
    from uspace_amd._hip import UspaceHipError, metric_topk
    from uspace_amd.tools import neighbors as N
    from uspace_amd.tools.feature_metrics import FeatureBank
    fake, test, train = _cpu_sets()
    with pytest.raises(UspaceHipError):
        N.nearest_neighbors(fake, train, k=3)
    with pytest.raises(UspaceHipError):
        N.nearest_neighbors(fake.numpy(), train.numpy(), k=3, shard_rows=8)
    with pytest.raises(UspaceHipError):
        N.nearest_neighbors(FeatureBank.from_features(train), FeatureBank.from_features(train), exclude_self=True)
    with pytest.raises(UspaceHipError):
        N.authenticity(fake, train)
    with pytest.raises(UspaceHipError):
        N.copying_zscore(fake, test, train)
    with pytest.raises(UspaceHipError):
        metric_topk(fake, train, 3)


def test_neighbor_grid_needs_no_gpu(tmp_path):
    """The figure is host work: rows of (query, its neighbours), an empty slot left as the padding value, only the named files
    of a folder opened."""
    from PIL import Image
    from uspace_amd.tools.neighbors import neighbor_grid
    g = torch.Generator().manual_seed(2)
    bank = (torch.rand(6, 3, 8, 10, generator=g) * 255).to(torch.uint8)
    q = (torch.rand(2, 3, 8, 10, generator=g) * 255).to(torch.uint8)
    os.makedirs(tmp_path / "bank")
    for i, a in enumerate(bank.permute(0, 2, 3, 1).numpy()):
        if i in (1, 4, 5):
            Image.fromarray(a).save(str(tmp_path / "bank" / f"{i}.png"))
        else:
            open(str(tmp_path / "bank" / f"{i}.png"), "wb").write(b"not an image")               # never opened
    idx = torch.tensor([[4, 1, -1], [5, 4, 1]], dtype=torch.int32)
    grid = neighbor_grid(q.float() / 255, str(tmp_path / "bank"), idx, str(tmp_path / "g.png"), padding=1, pad_value=1.0)
    pic = np.array(Image.open(str(tmp_path / "g.png")))
    assert tuple(grid.shape) == (3, 2 * 9 + 1, 4 * 11 + 1) and pic.shape == (2 * 9 + 1, 4 * 11 + 1, 3)
    tile = lambda r, c: pic[1 + 9 * r:9 * (r + 1), 1 + 11 * c:11 * (c + 1)].astype(int)
    want = lambda t: t.permute(1, 2, 0).numpy().astype(int)
    for r in range(2):                                             # (ToPILImage truncates x / 255 * 255: a level may drop by one)
        assert np.abs(tile(r, 0) - want(q[r])).max() <= 1
        for c in range(3):
            j = int(idx[r, c])
            assert (tile(r, c + 1) == 255).all() if j < 0 else np.abs(tile(r, c + 1) - want(bank[j])).max() <= 1
    same = neighbor_grid(q.float() / 255, bank.float() / 255, idx, str(tmp_path / "h.png"), padding=1, pad_value=1.0)
    assert torch.equal(same, grid)


def test_path_function_mirrors_the_fid_signature():
    from uspace_amd.tools import neighbors as N
    from uspace_amd.tools.fid_score import calculate_fid_given_paths
    fid = inspect.signature(calculate_fid_given_paths).parameters
    got = inspect.signature(N.calculate_memorization_given_paths).parameters
    assert list(got)[:len(fid)] == list(fid)
    for n in fid:
        assert got[n].default == fid[n].default, n
    assert got["k"].default == 1 and got["cells"].default is None and got["shard_rows"].default is None


# ------------------------------------------------------------------------------------------- ABI
def test_abi_surface():
    hdr = open(os.path.join(ROOT, "include", "uspace_hip.h")).read()
    declared = set(re.findall(r"USPACE_API\s+[\w\s\*]+?\b(uspace_\w+)\s*\(", hdr))
    from uspace_amd import _hip
    lib = ctypes.CDLL(os.path.join(ROOT, "uspace_amd", "libuspace_hip.so"))
    name = "uspace_metric_topk"
    assert name in declared and name in _hip.SIGNATURES and hasattr(lib, name)
    args = re.search(name + r"\s*\(([^)]*)\)", hdr).group(1).split(",")
    assert len(args) == 13 and len(_hip.SIGNATURES[name][1]) == 13 and _hip.SIGNATURES[name][0] is ctypes.c_int
    assert re.search(r"#define USPACE_ABI_VERSION 11\b", hdr) and _hip.ABI_VERSION == 11 and _hip.lib().uspace_abi_version() == 11
    assert callable(_hip.metric_topk)


def test_argument_errors_need_no_gpu():
    """The entry point validates before it launches: USPACE_ERR_ARG (-1) and USPACE_ERR_WORKSPACE (-3) come back without a device."""
    from uspace_amd import _hip
    L = _hip.lib()
    p = ctypes.c_void_p(64)                  # never dereferenced: every call below is refused first
    big = 1 << 20

    def topk(x=p, nx=100, y=p, ny=50, F=4, k=3, index_base=0, self_base=-1, d2=p, idx=p, ws=p, ws_bytes=big):
        return L.uspace_metric_topk(x, nx, y, ny, F, k, index_base, self_base, d2, idx, ws, ws_bytes, None)

    assert topk(k=0) == -1 and topk(k=17) == -1 and topk(F=0) == -1
    for name in ("x", "y", "d2", "idx", "ws"):
        assert topk(**{name: None}) == -1, name
    assert topk(nx=(1 << 24) + 1, ws_bytes=1 << 40) == -1 and topk(ny=(1 << 24) + 1, ws_bytes=1 << 40) == -1
    assert topk(nx=0) == -1 and topk(ny=0) == -1
    assert topk(self_base=-2) == -1 and topk(index_base=-1) == -1
    assert topk(index_base=2 ** 31 - 49) == -1 and topk(self_base=2 ** 31 - 99) == -1           # the last index is 2^31: beyond int32
    assert topk(ws_bytes=(100 + 50) * 8 - 1) == -3
    assert L.uspace_metric_workspace_bytes(100, 50, 0, 0) == (100 + 50) * 8


def test_kernels_have_no_scratch():
    """Code-object metadata of the built library (tools/kernel_resources.py; no GPU): the fifth instantiation of the engine and the
    refinement kernel do not spill, and the engine stays within the 256 registers of __launch_bounds__(256, 2).  The other four
    consumers keep the LDS they had: 64 x 36 + 128 x 36 floats and, where the consumer uses it, 64 x 16 doubles."""
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"):
        pytest.skip("llvm-objdump not available")
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    ks = kr.kernels()
    names = kr.demangle([k["name"] for k in ks])
    gram = {re.search(r"gram_kernel<.*?(\w+Consumer)>", n).group(1): k for k, n in zip(ks, names) if "gram_kernel<" in n}
    assert sorted(gram) == ["KnnConsumer", "ManifoldConsumer", "PolyConsumer", "RbfConsumer", "TopkConsumer"]
    for name, k in gram.items():
        assert k["scratch"] == 0 and k["vgpr"] + k["agpr"] <= 256 and k["wg"] == 256, (name, k)
        assert k["lds"] <= (64 + 128) * 36 * 4 + 64 * 16 * 8 + (64 * 16 * 4 if name == "TopkConsumer" else 0), (name, k)
    assert gram["TopkConsumer"]["lds"] == (64 + 128) * 36 * 4 + 64 * 16 * 8 + 64 * 16 * 4
    refine = [k for k, n in zip(ks, names) if "topk_refine_kernel" in n]
    assert len(refine) == 1 and refine[0]["scratch"] == 0 and refine[0]["wg"] == 1024
