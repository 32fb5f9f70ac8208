"""No GPU: the float64 restatements of tests/segops_cases.py against torch's own float64 operators, the metric's host arithmetic
on hand-made label maps, the margin rule on the chosen logits, and the argument refusals of the C entry points (which return
before anything is launched)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import segops_cases as S
from uspace_amd.tools import seg_metrics as _feature  # noqa: F401  (the references checked here exist for the operators: none passes without them)


@pytest.mark.parametrize("src,dst", S.RESIZES)
def test_bilinear_restatement_is_torch_float64(src, dst):
    x = S.rng(*src, *dst).normal(0, 1, (2,) + src + (5,))
    want = torch.nn.functional.interpolate(torch.from_numpy(x).permute(0, 3, 1, 2), size=dst, mode="bilinear", align_corners=False)
    got = S.bilinear_f64(x, *dst)
    assert float(np.abs(got - want.permute(0, 2, 3, 1).numpy()).max()) <= 1e-14 * float(np.abs(x).max())
    if src == dst:
        assert np.array_equal(got, x)


def test_source_taps_are_exact():
    i0, i1, lam = S.source_taps(4, 16)                 # scale 1/4: coordinates -0.375, -0.125, 0.125, ...
    assert list(i0[:4]) == [0, 0, 0, 0] and list(lam[:4]) == [0.0, 0.0, 0.125, 0.375] and i1[-1] == 3 and i0[-1] == 3
    i0, i1, lam = S.source_taps(7, 7)
    assert np.array_equal(i0, np.arange(7)) and not lam.any()
    assert np.array_equal(S.source_taps(1, 5)[0], np.zeros(5)) and np.array_equal(S.source_taps(1, 5)[1], np.zeros(5))


@pytest.mark.parametrize("hw", S.MAPS)
def test_dwconv_restatement_is_torch_float64(hw):
    x, w, b = S.dwconv_inputs(2, *hw, 8, 1)
    v, s = S.dwconv_preact_f64(x, w, b)
    tw = torch.from_numpy(w.astype(np.float64)).t().reshape(8, 1, 3, 3)
    want = torch.nn.functional.conv2d(torch.from_numpy(x.astype(np.float64)).permute(0, 3, 1, 2), tw, torch.from_numpy(b.astype(np.float64)),
                                      padding=1, groups=8)
    assert float(np.abs(v - want.permute(0, 2, 3, 1).numpy()).max()) <= 1e-13 and np.all(s >= np.abs(v) - 1e-12)
    gel = torch.nn.functional.gelu(want).permute(0, 2, 3, 1).numpy()
    assert float(np.abs(S.gelu_f64(v) - gel).max()) <= 1e-14
    # the bound is above what bf16 storage alone costs and below a percent of the value
    ref = S.gelu_f64(v)
    assert np.all(S.dwconv_bound(v, s, ref) >= np.abs(S.bf16_round(ref) - ref))
    big = np.abs(ref) > 0.5
    assert not big.any() or np.all(S.dwconv_bound(v, s, ref)[big] < 0.01 * np.abs(ref)[big])


@pytest.mark.parametrize("hw", S.MAPS)
@pytest.mark.parametrize("L", S.LABEL_COUNTS)
def test_margin_rule_leaves_out_few_pixels_of_the_chosen_logits(hw, L):
    """The share of pixels whose float64 top-two margin is under LABEL_MARGIN max |logit|, on the logits the GPU test uses: the
    test may leave out at most 0.1 %, so the float64 model alone must stay under that."""
    z = S.logits_map(2, *hw, L, 7)
    lab, margin = S.labels_f64(z, 4 * hw[0], 4 * hw[1])
    share = float(np.mean(margin <= S.LABEL_MARGIN * np.abs(z).max()))
    print(f"SEG-MEASURE margin-share {hw} L={L}: {share:.2e}")
    assert share <= S.LABEL_UNDER_MARGIN_SHARE
    t = torch.nn.functional.interpolate(torch.from_numpy(z.astype(np.float64)).permute(0, 3, 1, 2), size=lab.shape[1:], mode="bilinear",
                                        align_corners=False).argmax(dim=1).numpy()
    assert np.array_equal(lab[margin > 1e-9], t[margin > 1e-9])
    assert len(np.unique(lab)) >= min(L, 2) or hw == (1, 1)


def test_lowest_index_wins_a_tie_in_the_restatement():
    z = np.zeros((1, 2, 2, 4), dtype=np.float32)
    z[..., 1] = z[..., 3] = 2.0
    lab, margin = S.labels_f64(z, 8, 8)
    assert np.all(lab == 1) and np.all(margin == 0)
    assert np.all(S.labels_f64(z, 8, 8, without=[1])[0] == 3)


HAND_A = np.array([[[0, 0, 1, 1], [0, 0, 1, 1], [2, 2, 2, 2]]], dtype=np.uint8)
HAND_B = np.array([[[0, 0, 0, 1], [0, 1, 1, 1], [2, 2, 3, 3]]], dtype=np.uint8)


def test_overlap_on_hand_made_maps():
    from uspace_amd.tools.seg_metrics import overlap_from_counts
    counts = S.pair_counts_np(HAND_A, HAND_B, 5)
    assert counts[0].tolist() == [[4, 4, 4, 0, 0], [4, 4, 2, 2, 0], [3, 3, 2, 0, 0]]
    out = overlap_from_counts(counts, 12)
    assert out["agreement"][0] == 8 / 12
    want_iou = [3 / 5, 3 / 5, 2 / 4, 0.0]
    assert np.array_equal(out["iou"][0, :4], want_iou) and np.isnan(out["iou"][0, 4])
    assert out["miou"][0] == sum(want_iou) / 4
    ref = S.overlap_np(HAND_A, HAND_B, 5)
    for k in ("agreement", "miou", "iou"):
        assert np.array_equal(out[k], ref[k], equal_nan=True), k
    same = overlap_from_counts(S.pair_counts_np(HAND_A, HAND_A, 5), 12)
    assert same["agreement"][0] == 1.0 and same["miou"][0] == 1.0
    none = overlap_from_counts(np.zeros((1, 3, 5), dtype=np.int64), 12)            # every label beyond L
    assert np.isnan(none["miou"][0]) and none["agreement"][0] == 0.0


def test_region_sums_on_hand_made_maps():
    from uspace_amd.tools.seg_metrics import outside_from_sums
    a = np.zeros((1, 3, 3, 4))
    b = a.copy()
    b[0, :, 0, 0] = 0.5           # label 0 in both maps
    b[0, :, 2, 3] = 0.25          # 2 in a, 3 in b
    b[0, 1, 0, 2] = 1.0           # 1 in a, 0 in b
    s = S.region_sums_np(a, b, HAND_A, HAND_B, [3])
    assert s[0].tolist() == [3 * 0.25 + 1.0, 10.0]
    out = outside_from_sums(s, 12)
    assert out["outside_mse"][0] == 1.75 / 30 and out["outside_share"][0] == 10 / 12
    assert out["outside_psnr"][0] == 10 * np.log10(1 / (1.75 / 30))
    s = S.region_sums_np(a, b, HAND_A, HAND_B, [0, 3])
    assert s[0].tolist() == [0.0, 5.0]
    out = outside_from_sums(s, 12)
    assert out["outside_mse"][0] == 0.0 and np.isposinf(out["outside_psnr"][0])
    out = outside_from_sums(S.region_sums_np(a, b, HAND_A, HAND_B, [0, 1, 2, 3]), 12)       # nothing is outside
    assert np.isnan(out["outside_mse"][0]) and np.isnan(out["outside_psnr"][0]) and out["outside_share"][0] == 0.0
    assert S.region_sums_np(a, b, HAND_A, HAND_B, [])[0].tolist() == [3 * 0.25 + 3 * 0.0625 + 1.0, 12.0]


def test_accumulator_and_argument_checks_without_a_device():
    from uspace_amd import _hip
    from uspace_amd.tools import seg_metrics as M
    tower = M.LogitsParser(lambda x: x, 19)
    acc = M.SegmentationConsistency(tower, region=[3, 1, 3])
    assert acc.region == [1, 3] and acc.column_names == M.COLUMNS + M.REGION_COLUMNS and acc.n == 0
    assert M.SegmentationConsistency(tower).column_names == M.COLUMNS
    with pytest.raises(ValueError, match="no pairs"):
        acc.compute()
    with pytest.raises(ValueError):
        M.SegmentationConsistency(tower, region=[19])
    for bad in (0, 257, 2.0, True):
        with pytest.raises(ValueError):
            M.LogitsParser(lambda x: x, bad)
    x = torch.zeros(1, 3, 8, 8)
    with pytest.raises(_hip.UspaceHipError):
        M.segmentation_consistency(tower, x, x)
    with pytest.raises(_hip.UspaceHipError):
        M.label_overlap(torch.zeros(1, 4, 4, dtype=torch.uint8), torch.zeros(1, 4, 4, dtype=torch.uint8), 3)
    # means leave NaN rows out and keep +inf
    acc._parts["agreement"] = [np.array([1.0, 0.5])]
    acc._parts["miou"] = [np.array([1.0, np.nan])]
    acc._parts["iou"] = [np.array([[1.0, np.nan] + [np.nan] * 17, [0.5, 0.25] + [np.nan] * 17])]
    acc._parts["outside_mse"] = [np.array([0.0, np.nan])]
    acc._parts["outside_psnr"] = [np.array([np.inf, np.nan])]
    acc._parts["outside_share"] = [np.array([0.5, 0.0])]
    res = acc.compute()
    assert res["n"] == 2 and res["agreement"] == 0.75 and res["miou"] == 1.0 and res["outside_mse"] == 0.0
    assert res["outside_psnr"] == np.inf and res["iou"][0] == 0.75 and res["iou"][1] == 0.25 and np.isnan(res["iou"][2])


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """USPACE_ERR_ARG (-1) is returned ahead of the launch, so this needs no device; the pointers are never followed."""
    from uspace_amd import _hip
    L = _hip.lib()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 255) // 256 * 256)
    assert L.uspace_seg_labels_u8(p, 1, 4, 4, 257, p, 16, 16, None) == -1
    assert L.uspace_seg_labels_u8(p, 1, 4, 4, 0, p, 16, 16, None) == -1
    assert L.uspace_seg_labels_u8(p, 1, 4, 4, 19, p, 16385, 16, None) == -1
    assert L.uspace_seg_labels_u8(None, 1, 4, 4, 19, p, 16, 16, None) == -1
    assert L.uspace_seg_labels_u8(p, 0, 4, 4, 19, p, 16, 16, None) == -1
    assert L.uspace_dwconv3x3_gelu_bf16(p, p, p, ctypes.c_void_p(p.value + 1024), 1, 4, 4, 12, None) == -1          # C % 8
    assert L.uspace_dwconv3x3_gelu_bf16(p, p, p, p, 1, 4, 4, 8, None) == -1                                         # in place
    assert L.uspace_dwconv3x3_gelu_bf16(ctypes.c_void_p(p.value + 2), p, p, ctypes.c_void_p(p.value + 1024), 1, 4, 4, 8, None) == -1
    assert L.uspace_dwconv3x3_gelu_bf16(p, p, p, ctypes.c_void_p(p.value + 1024), 1, 0, 4, 8, None) == -1
    assert L.uspace_bilinear_nhwc_f32(p, 1, 4, 4, 8, p, 8, 8, 8, 1, None) == -1                                     # coff + C > ldo
    assert L.uspace_bilinear_nhwc_f32(p, 1, 4, 4, 8, p, 8, 8, 16, -1, None) == -1
    assert L.uspace_bilinear_nhwc_f32(p, 1, 4, 0, 8, p, 8, 8, 8, 0, None) == -1
    assert L.uspace_seg_pair_counts(p, p, 1, 16, 257, p, None) == -1
    assert L.uspace_seg_pair_counts(p, p, 1, 0, 19, p, None) == -1
    assert L.uspace_seg_pair_counts(p, p, 65536, 16, 19, p, None) == -1
    assert L.uspace_seg_region_sse_f64(p, p, p, p, p, 0, 1, 4, 4, p, None) == -1
    assert L.uspace_seg_region_sse_f64(p, p, p, p, None, 19, 1, 4, 4, p, None) == -1
    assert L.uspace_seg_region_sse_f64(p, p, p, p, p, 19, 1, 4, 16385, p, None) == -1
