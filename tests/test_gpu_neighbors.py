"""GPU checks of the memorisation primitives (uspace_metric_topk in uspace_amd/csrc/metrics.hip, uspace_amd/tools/neighbors.py)
against the float64 references, cases and bounds of tests/neighbor_cases.py."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import metric_cases as MC
from tests import neighbor_cases as NC

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()                # (a copy: the cached cases are read-only)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int64 if t.dtype == torch.float64 else t.dtype)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _same(a, b):
    return _same_bits(a[0], b[0]) and _same_bits(a[1], b[1])


def _topk(x, y, k, index_base=0, self_base=-1, ws=None):
    from uspace_amd import _hip
    d2, idx = _hip.metric_topk(x if torch.is_tensor(x) else _dev(x), y if torch.is_tensor(y) else _dev(y), k, index_base, self_base, ws=ws)
    torch.cuda.synchronize()
    assert d2.dtype == torch.float64 and idx.dtype == torch.int32 and d2.shape == idx.shape == (len(x), k)
    return d2, idx


def _check(got, x, y, k, index_base=0, self_base=-1):
    """Indices exactly, distances within 4 F u ref, tails (+inf, -1); returns the worst |got - ref| / bound."""
    NC.check_gaps(x, y, k, self_base, index_base)
    ref_d2, ref_idx = NC.ref_topk(x, y, k, index_base, self_base)
    d2, idx = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert (idx == ref_idx).all(), np.argwhere(idx != ref_idx)[:5]
    tail = ref_idx < 0
    assert np.isposinf(d2[tail]).all() and np.isfinite(d2[~tail]).all()
    with np.errstate(invalid="ignore"):                            # (inf - inf between two empty slots)
        assert (np.diff(d2, axis=1)[~tail[:, 1:]] >= 0).all()
    err, bound = np.abs(d2[~tail] - ref_d2[~tail]), NC.refined_bound(ref_d2[~tail], x.shape[1])
    assert (err <= bound).all()
    assert (d2[~tail][ref_d2[~tail] == 0.0] == 0.0).all()
    with np.errstate(invalid="ignore", divide="ignore"):
        r = err / bound
    return float(np.nanmax(r)) if r.size and not np.isnan(r).all() else 0.0


@functools.lru_cache(maxsize=None)
def _gpu_of(case, k):
    real, fake = MC.sets_of(case)
    return _topk(fake, real, k)


# ------------------------------------------------------------------------------------------- against the references
@pytest.mark.parametrize("case", MC.CASES, ids=str)
def test_topk_against_the_reference(case):
    """Every case at k = 1, the case's k and 16, generated against real and the real set against itself without self."""
    real, fake = MC.sets_of(case)
    for k in NC.ks_of(case):
        if k > len(real) - 1:
            continue
        r1 = _check(_gpu_of(case, k), fake, real, k)
        r2 = _check(_topk(real, real, k, 0, 0), real, real, k, 0, 0)
        print(f"{case} k={k}: worst |d2 - ref| / (4 F u ref): fake->real {r1:.3e}, real->real {r2:.3e}")


@pytest.mark.parametrize("name", sorted(NC.edge_cases()))
def test_edge_cases(name):
    x, y, k, index_base, self_base = NC.edge_cases()[name]
    r = _check(_topk(x, y, k, index_base, self_base), x, y, k, index_base, self_base)
    print(f"{name}: nx {len(x)} ny {len(y)} F {x.shape[1]} k {k}: worst ratio {r:.3e}")


def test_short_rows_end_in_inf_and_minus_one():
    x, y, k, _, _ = NC.edge_cases()["ny_below_k"]
    d2, idx = _topk(x, y, k)
    assert torch.isposinf(d2[:, 3:]).all() and (idx[:, 3:] == -1).all() and torch.isfinite(d2[:, :3]).all()
    one = _dev(y[:1])
    d2, idx = _topk(one, one, 2, 0, 0)                           # the only column is the row itself: nothing is eligible
    assert torch.isposinf(d2).all() and (idx == -1).all()


def test_duplicates_come_out_in_index_order():
    q, bank = NC.duplicate_bank()
    for k in (1, 2, 3, 5, 16):
        _check(_topk(q, bank, k), q, bank, k)
    d2, idx = _topk(q, bank, 3)
    idx, d2 = idx.cpu().numpy(), d2.cpu().numpy()
    for i in range(12):
        assert tuple(idx[i]) == NC.DUP_COLUMNS[i % 2] and d2[i, 0] == d2[i, 1] == d2[i, 2]
    assert (idx != NC.ref_topk(q, bank, 3, fault="ties_by_arrival")[1]).any()


def test_an_exact_copy_reports_zero_in_slot_0():
    q, bank, copies = NC.exact_copy_case()
    for k in (1, 16):
        got = _topk(q, bank, k)
        _check(got, q, bank, k)
        d2, idx = got[0].cpu().numpy(), got[1].cpu().numpy()
        n = len(copies)
        assert (d2[:n, 0] == 0.0).all() and tuple(idx[:n, 0]) == copies and (d2[n:, 0] > 0).all()


# ------------------------------------------------------------------------------------------- bit-equality and invariance
@pytest.mark.parametrize("case", [MC.CASES[0], MC.CASES[3]], ids=str)
def test_bit_equal_run_to_run_and_on_a_poisoned_workspace(case):
    from uspace_amd import _hip
    real, fake = MC.sets_of(case)
    x, y = _dev(fake), _dev(real)
    for k in (1, 16):
        first = _gpu_of(case, k)
        assert _same(first, _topk(x, y, k))
        ws = _hip.metric_workspace(len(fake), len(real), device=x.device, fill=0xFF)
        assert torch.isnan(ws.view(torch.float64)).all()
        assert _same(first, _topk(x, y, k, ws=ws))


def test_a_row_alone_and_the_other_rows_order():
    case = MC.CASES[0]
    real, fake = MC.sets_of(case)
    base = _gpu_of(case, 16)
    y = _dev(real)
    for i in (0, 70, len(fake) - 1):
        got = _topk(_dev(fake[i:i + 1]), y, 16)
        assert _same(got, (base[0][i:i + 1], base[1][i:i + 1])), i
    perm = np.random.default_rng(3).permutation(len(fake))
    got = _topk(_dev(fake[perm]), y, 16)
    p = torch.from_numpy(perm).cuda()
    assert _same(got, (base[0][p], base[1][p]))


def test_permuting_the_bank_permutes_the_indices():
    case = MC.CASES[0]                                            # no duplicates: every index is decided by the distances
    real, fake = MC.sets_of(case)
    base = _gpu_of(case, 16)
    perm = np.random.default_rng(4).permutation(len(real))       # row perm[j] of the original sits at j
    d2, idx = _topk(fake, real[perm], 16)
    assert _same_bits(d2, base[0])
    assert torch.equal(torch.from_numpy(perm).cuda()[idx.long()].to(torch.int32), base[1])


@pytest.mark.parametrize("case", [MC.CASES[0], MC.CASES[1]], ids=str)
def test_sharded_equals_unsharded(case):
    """300 bank rows walked in shards of 128 (and of 1 .. a shard larger than the bank), merged on the device."""
    from uspace_amd.tools.neighbors import nearest_neighbors
    real, fake = MC.sets_of(case)
    x, y = _dev(fake), _dev(real)
    for k in (1, 16):
        whole = nearest_neighbors(x, y, k)
        assert _same(whole, _gpu_of(case, k))
        for rows in (128, 7 if case[3] == 64 else 150, 1000):
            assert _same(whole, nearest_neighbors(x, y, k, shard_rows=rows)), rows
        self_whole = nearest_neighbors(y, y, k, exclude_self=True)
        assert _same(self_whole, nearest_neighbors(y, y, k, exclude_self=True, shard_rows=128))
        assert not (self_whole[1] == torch.arange(len(real), device="cuda", dtype=torch.int32)[:, None]).any()
    q, bank = NC.duplicate_bank()
    assert _same(nearest_neighbors(_dev(q), _dev(bank), 5), nearest_neighbors(_dev(q), _dev(bank), 5, shard_rows=128))


# ------------------------------------------------------------------------------------------- other entry points and tools
@pytest.mark.parametrize("case", MC.CASES, ids=str)
def test_agrees_with_knn_radius2_and_manifold(case):
    from uspace_amd import _hip
    from uspace_amd.tools.neighbors import nearest_neighbors
    real, fake = MC.sets_of(case)
    x, y, k, F = _dev(real), _dev(fake), case[4], case[3]
    nr, nf = MC.ref_norms2(real), MC.ref_norms2(fake)
    kth = nearest_neighbors(x, x, k, exclude_self=True)[0][:, k - 1].cpu().numpy()
    radius2 = _hip.metric_knn_radius2(x, k).cpu().numpy()
    assert (np.abs(kth - radius2) <= MC.dist_ceiling(nr, nr, F)).all()
    nearest = nearest_neighbors(x, y, 1)[0][:, 0].cpu().numpy()
    min_d2 = _hip.metric_manifold(x, y, None, want_count=False)[1].cpu().numpy()
    assert (np.abs(nearest - min_d2) <= MC.dist_ceiling(nr, nf, F)).all()


@pytest.mark.parametrize("case", MC.CASES, ids=str)
def test_authenticity(case):
    from uspace_amd.tools.feature_metrics import FeatureBank
    from uspace_amd.tools.neighbors import authenticity
    real, fake = MC.sets_of(case)
    ref = NC.ref_authenticity(fake, real)
    assert ref["gap"] >= NC.MIN_AUTH_GAP
    got = authenticity(_dev(fake), _dev(real))
    assert type(got["authenticity_pct"]) is float and got["authenticity_pct"] == ref["pct"]
    assert got["authentic"].dtype == torch.bool and (got["authentic"].cpu().numpy() == ref["authentic"]).all()
    assert (got["idx"].cpu().numpy() == ref["idx"]).all()
    assert (np.abs(got["d2"].cpu().numpy() - ref["d2"]) <= NC.refined_bound(ref["d2"], case[3])).all()
    assert (np.abs(got["train_d2"].cpu().numpy() - ref["train_d2"]) <= NC.refined_bound(ref["train_d2"], case[3])).all()
    again = authenticity(FeatureBank.from_features(_dev(fake)), FeatureBank.from_features(_dev(real)))
    assert again["authenticity_pct"] == got["authenticity_pct"] and _same_bits(again["d2"], got["d2"])


def test_hand_made_example():
    from uspace_amd.tools.neighbors import authenticity, copying_zscore, nearest_neighbors
    fake, test, train = _dev(NC.HAND_FAKE), _dev(NC.HAND_TEST), _dev(NC.HAND_TRAIN)
    got = authenticity(fake, train)
    assert got["d2"].tolist() == NC.HAND_L_FAKE and got["idx"].tolist() == [0, 1, 2, 3, 0]
    assert got["authentic"].tolist() == [False, True, False, True, False] and got["authenticity_pct"] == 40.0
    assert got["train_d2"].tolist() == [16.0, 16.0, 100.0, 100.0]
    assert nearest_neighbors(train, train, 1, exclude_self=True)[1][:, 0].tolist() == [1, 0, 0, 2]
    assert nearest_neighbors(test, train, 1)[0][:, 0].tolist() == NC.HAND_L_TEST
    z = copying_zscore(fake, test, train)
    assert z == pytest.approx((NC.HAND_U - 7.5) / np.sqrt(11.25), rel=NC.Z_RTOL)
    from_arrays = authenticity(NC.HAND_FAKE, NC.HAND_TRAIN)                      # an array has no device: it goes to the ROCm one
    assert from_arrays["d2"].is_cuda and _same_bits(from_arrays["d2"], got["d2"]) and from_arrays["authenticity_pct"] == 40.0
    assert copying_zscore(NC.HAND_FAKE, NC.HAND_TEST.astype(np.float64), NC.HAND_TRAIN) == z
    assert _same(nearest_neighbors(NC.HAND_TEST, train, 2, shard_rows=3), nearest_neighbors(test, train, 2))


@pytest.mark.parametrize("case", MC.CASES, ids=str)
def test_copying_zscore(case):
    from uspace_amd.tools.neighbors import copying_zscore
    fake, test, train, cells = NC.copying_sets(case)
    l_fake, l_test = NC.ref_topk(fake, train, 1)[0][:, 0], NC.ref_topk(test, train, 1)[0][:, 0]
    NC.check_rank_gaps(l_fake, l_test)
    want = NC.ref_zu(l_fake, l_test)
    got = copying_zscore(_dev(fake), _dev(test), _dev(train))
    print(f"{case}: Z_U {got!r} (ref {want!r})")
    assert type(got) is float and abs(got - want) <= NC.Z_RTOL * abs(want)
    assert abs(got - NC.ref_zu(l_fake, l_test, "u_without_ties")) > 1e-6
    if case[0] != 4:                                              # (17 rows: no cell holds ten test samples)
        want = NC.ref_zu_cells(l_fake, l_test, cells, NC.MIN_CELL)
        got = copying_zscore(_dev(fake), _dev(test), _dev(train), cells=cells, min_cell=NC.MIN_CELL)
        print(f"  per cell: {got!r} (ref {want!r})")
        assert abs(got - want) <= NC.Z_RTOL * abs(want)
        got_t = copying_zscore(_dev(fake), _dev(test), _dev(train), cells=tuple(torch.from_numpy(c) for c in cells), min_cell=NC.MIN_CELL)
        assert got_t == got


def test_end_to_end_from_images_and_the_grid(tmp_path):
    """8 generated, 12 training and 7 held-out random 64^2 images through a seeded Inception-v3, two generated ones copies of
    training images: folders, banks and tensors give the same numbers, the copies report 0.0, and the grid's first tile of every
    row is the query."""
    from PIL import Image
    from uspace_amd.tools.feature_metrics import FeatureBank
    from uspace_amd.tools.inception import InceptionV3
    from uspace_amd.tools.neighbors import (authenticity, calculate_memorization_given_paths, copying_zscore, nearest_neighbors,
                                            neighbor_grid)
    model = InceptionV3([3], seed=0).cuda()
    g = torch.Generator().manual_seed(5)
    imgs = {"fake": torch.rand(8, 3, 64, 64, generator=g), "train": torch.rand(12, 3, 64, 64, generator=g),
            "test": torch.rand(7, 3, 64, 64, generator=g)}
    imgs["fake"][1], imgs["fake"][6] = imgs["train"][10], imgs["train"][3]
    banks, quant = {}, {}
    for name, x in imgs.items():
        bank = FeatureBank(2048, device="cuda", model=model)
        bank.update(x)
        banks[name] = bank
        quant[name] = x.mul(255).add(0.5).clamp(0, 255).to(torch.uint8)
        os.makedirs(tmp_path / name)
        for i, a in enumerate(quant[name].permute(0, 2, 3, 1).numpy()):
            Image.fromarray(a).save(str(tmp_path / name / f"{i:02d}.png"))
    want = authenticity(banks["fake"], banks["train"])
    assert want["d2"][1] == 0.0 and want["d2"][6] == 0.0 and want["idx"][1] == 10 and want["idx"][6] == 3
    assert not want["authentic"][1] and not want["authentic"][6]
    z = copying_zscore(banks["fake"], banks["test"], banks["train"])
    paths = tuple(str(tmp_path / n) for n in ("fake", "train", "test"))
    got = calculate_memorization_given_paths(paths, device="cuda", batch_size=12, num_workers=0, model=model, k=3)
    assert got["authenticity_pct"] == want["authenticity_pct"] and _same_bits(got["d2"], want["d2"]) and _same_bits(got["idx"], want["idx"])
    assert got["z_u"] == z and _same(got["neighbors"], nearest_neighbors(banks["fake"], banks["train"], 3))
    banks["train"].save(str(tmp_path / "train.npz"))
    two = calculate_memorization_given_paths((paths[0], str(tmp_path / "train.npz")), device="cuda", batch_size=12, num_workers=0,
                                             model=model, k=3)
    assert "z_u" not in two and two["authenticity_pct"] == want["authenticity_pct"] and _same(two["neighbors"], got["neighbors"])
    print(f"authenticity {got['authenticity_pct']} %, Z_U {z}")
    # the figure: from the folder and from the tensor
    idx = got["neighbors"][1]
    q = quant["fake"].float() / 255
    for bank_images, out in ((paths[1], "a.png"), (quant["train"].float() / 255, "b.png")):
        neighbor_grid(q, bank_images, idx, str(tmp_path / out), padding=2)
        pic = np.array(Image.open(str(tmp_path / out)))
        assert pic.shape == (8 * 66 + 2, 4 * 66 + 2, 3)
        for i in range(8):
            tile = lambda c: pic[2 + 66 * i:66 * (i + 1), 2 + 66 * c:66 * (c + 1)]
            assert np.abs(tile(0).astype(int) - quant["fake"][i].permute(1, 2, 0).numpy().astype(int)).max() <= 1
            for c in range(3):
                assert np.abs(tile(c + 1).astype(int) - quant["train"][int(idx[i, c])].permute(1, 2, 0).numpy().astype(int)).max() <= 1
    assert (np.array(Image.open(str(tmp_path / "a.png"))) == np.array(Image.open(str(tmp_path / "b.png")))).all()


def test_end_to_end_with_a_dino_tower(tmp_path):
    """The same path with ``model=DinoFeatures(tower)``: class-token features of a seeded one-layer tower from PNG folders equal
    the features of the decoded bytes, and a copied training image reports 0.0."""
    from PIL import Image
    from uspace_amd.libs.dino import DinoVisionTransformer
    from uspace_amd.tools.dino_metrics import DinoFeatures
    from uspace_amd.tools.neighbors import authenticity, calculate_memorization_given_paths
    tower = DinoVisionTransformer(seed=0, hidden_size=128, num_attention_heads=2, num_hidden_layers=1, patch_size=8, image_size=32,
                                  table_size=32, layerscale=False, layer_norm_eps=1e-6).cuda()
    ex = DinoFeatures(tower, 8)
    g = torch.Generator().manual_seed(9)
    quant = {"fake": (torch.rand(6, 3, 32, 32, generator=g) * 255).to(torch.uint8), "train": (torch.rand(9, 3, 32, 32, generator=g) * 255).to(torch.uint8)}
    quant["fake"][2] = quant["train"][7]
    feats = {}
    for name, q in quant.items():
        os.makedirs(tmp_path / name)
        for i, a in enumerate(q.permute(0, 2, 3, 1).numpy()):
            Image.fromarray(a).save(str(tmp_path / name / f"{i}.png"))
        feats[name] = ex.features(q.cuda().float() / 255, quantize=False)
    want = authenticity(feats["fake"], feats["train"])
    got = calculate_memorization_given_paths((str(tmp_path / "fake"), str(tmp_path / "train")), device="cuda", batch_size=8, model=ex, k=2)
    assert got["d2"][2] == 0.0 and got["idx"][2] == 7 and not got["authentic"][2]
    assert _same_bits(got["d2"], want["d2"]) and _same_bits(got["idx"], want["idx"]) and got["authenticity_pct"] == want["authenticity_pct"]
    assert got["neighbors"][0].shape == (6, 2) and _same_bits(got["neighbors"][0][:, 0].contiguous(), want["d2"].contiguous())
