"""The segmentation-consistency metric (tools/seg_metrics.py) on the GPU: the two pair reductions against numpy on random label
maps, the metric end to end on a stub parser with an unmoved pair, the ``PairMetrics.parsing`` columns against the standalone
values, and two folders of PNGs.  Counts must be equal; the fp64 region sum is held to ``segops_cases.SSE_RTOL``."""
import numpy as np
import pytest
import torch

from tests import segops_cases as S

pytestmark = pytest.mark.gpu


def tower(L=19):
    from uspace_amd.tools.seg_metrics import LogitsParser
    stub = S.StubParser(L)
    return LogitsParser(stub.logits, L, chunk=3), stub


@pytest.mark.parametrize("hw", [(1, 1), (100, 132), (7, 16), (64, 257)])
@pytest.mark.parametrize("L", [2, 19, 150])
def test_pair_reductions_against_numpy(hw, L):
    from uspace_amd import _hip
    from uspace_amd.tools.seg_metrics import label_overlap, region_difference, outside_from_sums
    la, lb = S.label_pair(3, *hw, L, 1)
    lad, lbd = torch.from_numpy(la).cuda(), torch.from_numpy(lb).cuda()
    out = label_overlap(lad, lbd, L)
    assert out["counts"].dtype == np.int64 and np.array_equal(out["counts"], S.pair_counts_np(la, lb, L))
    ref = S.overlap_np(la, lb, L)
    for k in ("agreement", "iou"):                            # one division of the same integers
        assert out[k].dtype == np.float64 and np.array_equal(out[k], ref[k], equal_nan=True), k
    assert np.allclose(out["miou"], ref["miou"], rtol=0, atol=S.miou_atol(L))
    assert out["agreement"][0] == 1.0 and out["miou"][0] == 1.0
    # labels beyond L are counted nowhere
    if L > 2:
        few = label_overlap(lad, lbd, L - 1)["counts"]
        assert np.array_equal(few, out["counts"][:, :, :L - 1])
    a, b = S.edit_pairs(3, *hw, 2)
    b[0] = (a[0] + 0.25).clamp(0, 1)                       # pair 0: equal labels, moved image
    ad, bd = a.cuda(), b.cuda()
    worst = 0.0
    for region in ([], [0], list(range(0, L, 2)), list(range(L))):         # empty, one label, half, all-covering
        member = np.zeros(L, dtype=np.uint8)
        member[region] = 1
        got = _hip.seg_region_sse(ad, bd, lad, lbd, torch.from_numpy(member).cuda()).cpu().numpy()
        want = S.region_sums_np(a.numpy(), b.numpy(), la, lb, region)
        assert got.dtype == np.float64 and np.array_equal(got[:, 1], want[:, 1])
        worst = max(worst, float((np.abs(got[:, 0] - want[:, 0]) / np.maximum(want[:, 0], 1e-300)).max()))
        assert np.all(np.abs(got[:, 0] - want[:, 0]) <= S.SSE_RTOL * want[:, 0])
        cols = region_difference(ad, bd, lad, lbd, region, L)
        ref_cols = outside_from_sums(got, hw[0] * hw[1])
        for k in ref_cols:
            assert np.array_equal(cols[k], ref_cols[k], equal_nan=True), k
        if len(region) == L:
            assert not got.any() and np.isnan(cols["outside_mse"]).all() and not cols["outside_share"].any()
        if not region:
            assert np.all(got[:, 1] == hw[0] * hw[1])
    print(f"SEG-MEASURE region-sse {hw} L={L}: worst relative error {worst:.3e} (bound {S.SSE_RTOL:.0e})")
    # a pair's row does not depend on the batch or its place in it
    member = torch.ones(L, dtype=torch.uint8).cuda()
    member[0] = 0
    whole = _hip.seg_region_sse(ad, bd, lad, lbd, member)
    order = [2, 0, 1]
    moved = _hip.seg_region_sse(ad[order].contiguous(), bd[order].contiguous(), lad[order].contiguous(), lbd[order].contiguous(), member)
    assert torch.equal(moved, whole[order])
    assert torch.equal(_hip.seg_pair_counts(lad[2:].contiguous(), lbd[2:].contiguous(), L)[0], _hip.seg_pair_counts(lad, lbd, L)[2])


def test_consistency_end_to_end_with_an_unmoved_pair():
    from uspace_amd.tools.seg_metrics import segmentation_consistency, labels_from_logits
    L = 19
    tw, stub = tower(L)
    a, b = S.edit_pairs(4, 100, 132, 3)
    region = [2, 5, 11]
    out = segmentation_consistency(tw, a.cuda(), b.cuda(), region=region)
    assert set(out) == {"agreement", "miou", "iou", "outside_mse", "outside_psnr", "outside_share"}
    assert out["agreement"][0] == 1.0 and out["miou"][0] == 1.0 and out["outside_mse"][0] == 0.0 and np.isposinf(out["outside_psnr"][0])
    assert np.all(out["agreement"][1:] < 1.0) and np.all(out["agreement"] > 0.3) and np.all(out["outside_mse"][1:] > 0)
    # from the parser's own label maps, through the float64 definitions
    # (the levels q / 255 as the device forms them: they can differ from the host's by an ulp, see _inputs.quantize)
    from uspace_amd.tools._inputs import quantize
    qa, qb = (quantize(t.cuda()) for t in (a, b))
    la, lb = (labels_from_logits(stub.logits(q), (100, 132)).cpu().numpy() for q in (qa, qb))
    qa, qb = qa.cpu(), qb.cpu()
    assert len(np.unique(la)) >= 4
    ref = S.overlap_np(la, lb, L)
    for k in ("agreement", "iou"):
        assert np.array_equal(out[k], ref[k], equal_nan=True), k
    assert np.allclose(out["miou"], ref["miou"], rtol=0, atol=S.miou_atol(L))
    sums = S.region_sums_np(qa.numpy(), qb.numpy(), la, lb, region)
    assert np.allclose(out["outside_mse"], sums[:, 0] / (3 * sums[:, 1]), rtol=S.SSE_RTOL, atol=0)
    assert np.array_equal(out["outside_share"], sums[:, 1] / (100 * 132))
    # rows do not depend on the batch; without a region there are no outside columns
    one = segmentation_consistency(tw, a[2:3].cuda(), b[2:3].cuda(), region=region)
    for k in out:
        assert np.array_equal(one[k][0], out[k][2], equal_nan=True), k
    assert set(segmentation_consistency(tw, a.cuda(), b.cuda())) == {"agreement", "miou", "iou"}
    raw = segmentation_consistency(tw, a.cuda(), b.cuda(), region=region, quantize=False)
    assert raw["agreement"][0] == 1.0 and not np.array_equal(raw["outside_mse"], out["outside_mse"])


def test_pair_metrics_parsing_columns_and_folders(tmp_path):
    from PIL import Image
    from uspace_amd.tools.lpips import LPIPS
    from uspace_amd.tools.pair_metrics import PairMetrics
    from uspace_amd.tools.seg_metrics import (COLUMNS, REGION_COLUMNS, SegmentationConsistency, segmentation_consistency,
                                              calculate_segmentation_consistency_given_paths)
    tw, _ = tower(19)
    a, b = S.edit_pairs(4, 96, 96, 4)
    region = [1, 4, 7, 12]
    direct = segmentation_consistency(tw, a.cuda(), b.cuda(), region=region)
    lp = LPIPS("alex", seed=3).cuda()
    plain, with_seg, no_region = (PairMetrics(device="cuda", lpips=lp) for _ in range(3))
    assert with_seg.parsing is None
    with_seg.parsing = SegmentationConsistency(tw, region)
    no_region.parsing = SegmentationConsistency(tw)
    for pm in (plain, with_seg, no_region):
        pm.update(a[:3], b[:3])
        pm.update(a[3:], b[3:])
    v0, v1 = plain.values, with_seg.values
    assert list(v0) == ["lpips", "ssim", "psnr"] and list(v1) == list(v0) + list(COLUMNS + REGION_COLUMNS)
    assert list(no_region.values) == list(v0) + list(COLUMNS)
    for k in v0:
        assert np.array_equal(v0[k], v1[k]), k
    for k in COLUMNS + REGION_COLUMNS:
        assert v1[k].dtype == np.float64 and np.array_equal(v1[k], direct[k], equal_nan=True), k
    res = with_seg.compute()
    assert res["n"] == 4 and res["miou"] == float(np.mean(direct["miou"])) and "miou" not in plain.compute()
    with pytest.raises(ValueError, match="before the first update"):
        with_seg.parsing = None

    acc = SegmentationConsistency(tw, region)
    acc.update(a[:1].cuda(), b[:1].cuda())
    acc.update(a[1:].cuda(), b[1:].cuda())
    assert acc.n == 4
    for k, v in acc.values.items():
        assert np.array_equal(v, direct[k], equal_nan=True), k

    qa, qb = ((t * 255 + 0.5).clamp(0, 255).to(torch.uint8) for t in (a, b))
    for d, q in (("a", qa), ("b", qb)):
        (tmp_path / d).mkdir()
        for i in range(4):
            Image.fromarray(q[i].permute(1, 2, 0).numpy()).save(tmp_path / d / f"{i:03d}.png")
    out = calculate_segmentation_consistency_given_paths(tmp_path / "a", tmp_path / "b", tw, region, device="cuda", batch_size=3)
    assert out["n"] == 4
    for k in direct:                                            # the written PNGs hold the quantised numbers
        assert np.array_equal(out["values"][k], direct[k], equal_nan=True), k
    assert out["agreement"] == float(np.mean(direct["agreement"]))
    (tmp_path / "b" / "extra.png").write_bytes((tmp_path / "b" / "000.png").read_bytes())
    with pytest.raises(ValueError, match="pair up"):
        calculate_segmentation_consistency_given_paths(tmp_path / "a", tmp_path / "b", tw, device="cuda")
