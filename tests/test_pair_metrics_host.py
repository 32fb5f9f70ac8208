"""Paired metrics without a GPU: the C-ABI's declarations and queries, the float64 restatement of tests/lpips_stages.py against
independent facts, the planted faults against the GPU tolerances, the LPIPS weight loader and the folder pairing."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import lpips_stages as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("uspace_lpips_num_params", "uspace_lpips_param_numel", "uspace_lpips_weight_bytes", "uspace_lpips_workspace_bytes",
         "uspace_lpips_pack_weights", "uspace_lpips_forward", "uspace_lpips_tap", "uspace_lpips_distance_workspace_bytes",
         "uspace_lpips_distance_f64", "uspace_ssim_workspace_bytes", "uspace_ssim_f64", "uspace_psnr_workspace_bytes",
         "uspace_psnr_f64")


def _seeded(net):
    from uspace_amd.tools.lpips import LPIPS
    m = LPIPS(net, seed=3)
    return m, {k: v.detach() for k, v in m.state_dict().items()}


# ------------------------------------------------------------------------------------------- ABI
def test_every_new_export_is_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "uspace_hip.h")).read()
    declared = set(re.findall(r"USPACE_API\s+[\w\s\*]+?\b(uspace_\w+)\s*\(", hdr))
    from uspace_amd import _hip
    lib = ctypes.CDLL(os.path.join(ROOT, "uspace_amd", "libuspace_hip.so"))
    for name in NAMES:
        assert name in declared and name in _hip.SIGNATURES and hasattr(lib, name), name
    assert declared == set(_hip.SIGNATURES)
    assert _hip.lib().uspace_abi_version() == _hip.ABI_VERSION == 11
    assert "#define USPACE_ABI_VERSION 11" in hdr
    mk = open(os.path.join(ROOT, "uspace_amd", "csrc", "Makefile")).read()
    assert "lpips.hip" in mk and "conv_f32.h" in mk


def test_parameter_queries_without_gpu():
    from uspace_amd import _hip
    from uspace_amd.tools.lpips import NETS, state_dict_layout
    L = _hip.lib()
    for net, tensors, conv_elems, lin_elems in (("alex", 15, 2469696, 1152), ("vgg", 31, 14714688, 1472)):
        i = NETS[net]
        assert L.uspace_lpips_num_params(i) == tensors
        numels = [L.uspace_lpips_param_numel(i, k) for k in range(tensors)]
        assert sum(numels) == conv_elems + lin_elems and sum(numels[-5:]) == lin_elems
        assert numels == [int(np.prod(shape)) for _k, shape in state_dict_layout(net)]          # the module's state_dict order
        assert L.uspace_lpips_param_numel(i, tensors) == -1 and L.uspace_lpips_param_numel(i, -1) == -1
        assert L.uspace_lpips_weight_bytes(i) >= 4 * sum(numels)
    assert L.uspace_lpips_num_params(2) == -1 and L.uspace_lpips_num_params(-1) == -1
    assert L.uspace_lpips_param_numel(2, 0) == -1 and L.uspace_lpips_weight_bytes(2) == 0 and L.uspace_lpips_workspace_bytes(2, 1, 64, 64) == 0


def test_workspace_bytes_grow_with_batch_and_area():
    from uspace_amd import _hip
    L = _hip.lib()
    for net in (0, 1):
        wb = lambda B, H, W: L.uspace_lpips_workspace_bytes(net, B, H, W)
        assert 0 < wb(1, 64, 64) < wb(2, 64, 64) < wb(16, 64, 64)
        assert wb(1, 64, 64) < wb(1, 64, 128) < wb(1, 256, 256)
        assert wb(0, 64, 64) == 0 and wb(1, 0, 64) == 0 and wb(1, 8, 8) == 0          # too small for either stack
    assert L.uspace_lpips_workspace_bytes(0, 1, 30, 64) == 0 < L.uspace_lpips_workspace_bytes(0, 1, 31, 31)
    assert L.uspace_lpips_workspace_bytes(1, 1, 15, 64) == 0 < L.uspace_lpips_workspace_bytes(1, 1, 16, 16)
    assert L.uspace_lpips_workspace_bytes(1, 256, 256, 256) == 0                        # 2^31 elements in one tensor
    assert L.uspace_ssim_workspace_bytes(1, 3, 10, 64) == 0 == L.uspace_ssim_workspace_bytes(1, 3, 64, 10)
    assert 0 < L.uspace_ssim_workspace_bytes(1, 3, 11, 11) < L.uspace_ssim_workspace_bytes(2, 3, 64, 64)
    assert 0 < L.uspace_psnr_workspace_bytes(1, 100) < L.uspace_psnr_workspace_bytes(3, 3 * 256 * 256)
    assert L.uspace_lpips_distance_workspace_bytes(1, 9, 100) == 0 < L.uspace_lpips_distance_workspace_bytes(1, 9, 192)


def test_argument_errors_need_no_gpu():
    """The entry points validate before they launch: USPACE_ERR_ARG (-1) and USPACE_ERR_WORKSPACE (-3) come back without a device."""
    from uspace_amd import _hip
    L = _hip.lib()
    p = ctypes.c_void_p(256)                 # never dereferenced: every call below is refused first
    assert L.uspace_lpips_forward(2, p, p, 1 << 30, p, p, 1, 64, 64, 0, p, None, None) == -1
    assert L.uspace_lpips_forward(0, p, p, 1 << 30, p, p, 1, 30, 30, 0, p, None, None) == -1
    assert L.uspace_lpips_forward(0, p, p, 1 << 30, p, p, 1, 64, 64, 0, None, None, None) == -1
    assert L.uspace_lpips_forward(0, p, p, 16, p, p, 1, 64, 64, 0, p, None, None) == -3
    assert L.uspace_lpips_tap(1, p, p, 1 << 30, p, p, 1, 32, 32, 0, 6, p, None) == -1
    assert L.uspace_lpips_pack_weights(0, None, 15, p, 1 << 30, None) == -1
    assert L.uspace_lpips_distance_f64(p, p, p, 1, 9, 100, p, 1 << 20, p, None) == -1
    assert L.uspace_lpips_distance_f64(p, p, p, 1, 9, 192, p, 0, p, None) == -3
    assert L.uspace_ssim_f64(p, p, 1, 3, 10, 10, 1.0, p, 1 << 20, p, None) == -1
    assert L.uspace_ssim_f64(p, p, 1, 3, 64, 64, 0.0, p, 1 << 20, p, None) == -1
    assert L.uspace_ssim_f64(p, p, 1, 3, 64, 64, 1.0, p, 8, p, None) == -3
    assert L.uspace_psnr_f64(p, p, 0, 100, 1.0, p, 1 << 20, p, None) == -1
    assert L.uspace_psnr_f64(p, p, 1, 100, 1.0, p, 0, p, None) == -3


def test_python_stage_shapes_match_the_restatement():
    from uspace_amd.tools.lpips import stage_shapes
    for net, H, W in (("alex", 64, 64), ("alex", 70, 95), ("alex", 256, 256), ("vgg", 32, 32), ("vgg", 38, 51)):
        _m, sd = _seeded(net)
        x = S.scaled(S.images(1, H, W, seed=1))
        shapes = [tuple(x.shape[2:]) + (3,)]
        for s in range(1, 6):
            x = S.stage(sd, net, s, x)
            shapes.append((x.shape[2], x.shape[3], x.shape[1]))
        assert shapes == stage_shapes(net, H, W), (net, H, W)


# ------------------------------------------------------------------------------------------- the restatement against independent facts
def test_ssim_restatement():
    from scipy.ndimage import gaussian_filter
    a, b = (t.numpy().astype(np.float64) for t in S.pair(2, 40, 52, seed=3))
    assert np.allclose(S.ssim(a, a), 1.0, atol=1e-12)
    assert abs(S.window().sum() - 1) < 1e-15 and len(S.window()) == 11
    # moments by scipy's Gaussian filter (radius int(3.5 * 1.5 + 0.5) = 5), read on the interior where no boundary rule enters
    f = lambda t: gaussian_filter(t, sigma=(0, 0, 1.5, 1.5), truncate=3.5)[..., 5:-5, 5:-5]
    mx, my = f(a), f(b)
    sxx, syy, sxy = f(a * a) - mx * mx, f(b * b) - my * my, f(a * b) - mx * my
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    ref = (((2 * mx * my + c1) * (2 * sxy + c2)) / ((mx * mx + my * my + c1) * (sxx + syy + c2))).mean((1, 2, 3))
    assert np.allclose(S.ssim(a, b), ref, rtol=0, atol=1e-12)
    assert np.all(S.ssim(a, b) < 0.99) and np.allclose(S.ssim(a, b), S.ssim(b, a), atol=1e-15)
    assert np.allclose(S.ssim(255 * a, 255 * b, 255.0), S.ssim(a, b), atol=1e-12)
    one = S.ssim(a[:, :, :11, :11], b[:, :, :11, :11])                     # a single window: the weighted moments of the patch
    w2 = np.outer(S.window(), S.window())
    m = lambda t: (w2 * t[:, :, :11, :11]).sum((2, 3))
    mx, my = m(a), m(b)
    ref1 = (((2 * mx * my + c1) * (2 * (m(a * b) - mx * my) + c2)) /
            ((mx * mx + my * my + c1) * (m(a * a) - mx * mx + m(b * b) - my * my + c2))).mean(1)
    assert np.allclose(one, ref1, atol=1e-13)


def test_psnr_restatement():
    a = 0.25 + 0.5 * S.images(2, 9, 13, seed=1).numpy().astype(np.float64)
    for delta in (0.5, 2.0 ** -5, 1e-3):
        assert np.allclose(S.psnr(a, a + delta), -20 * np.log10(delta), atol=1e-9)
    assert np.allclose(S.psnr(255 * a, 255 * (a + 0.1), 255.0), 20.0, atol=1e-9)
    assert np.all(np.isposinf(S.psnr(a, a)))


@pytest.mark.parametrize("net", ["alex", "vgg"])
def test_lpips_restatement(net):
    _m, sd = _seeded(net)
    H, W = (70, 95) if net == "alex" else (38, 51)
    x0, x1 = S.pair(2, H, W, seed=6)
    d01, layers = S.lpips(sd, net, x0, x1, normalize=True)
    d10, _ = S.lpips(sd, net, x1, x0, normalize=True)
    d00, l00 = S.lpips(sd, net, x0, x0, normalize=True)
    assert torch.all(d00 == 0) and torch.all(l00 == 0)
    assert torch.allclose(d01, d10, rtol=1e-13, atol=0) and torch.all(d01 > 0)
    assert layers.shape == (5, 2) and torch.allclose(layers.sum(0), d01, rtol=1e-15, atol=0)
    # normalize=True on [0, 1] images is normalize=False on the same images mapped to [-1, 1]
    assert torch.allclose(S.lpips(sd, net, 2 * x0.double() - 1, 2 * x1.double() - 1)[0], d01, rtol=1e-12, atol=0)
    # the head by its definition on one pixel, by hand
    g = torch.Generator().manual_seed(0)
    a, b, w = torch.rand(1, 64, 1, 1, generator=g).double(), torch.rand(1, 64, 1, 1, generator=g).double(), torch.rand(64, generator=g).double()
    av, bv = a.flatten() / (a.norm() + 1e-10), b.flatten() / (b.norm() + 1e-10)
    assert torch.allclose(S.distance(a, b, w), (w * (av - bv) ** 2).sum()[None], rtol=1e-14, atol=0)
    assert torch.all(S.distance(torch.zeros(1, 64, 2, 2), torch.zeros(1, 64, 2, 2), w) == 0)      # 0 / (0 + eps) = 0


def test_planted_faults_move_the_restatement_beyond_the_gpu_tolerances():
    from tests.test_gpu_pair_metrics import TOL
    for net, (H, W) in (("alex", (70, 95)), ("vgg", (38, 51))):
        _m, sd = _seeded(net)
        x0, x1 = S.pair(2, H, W, seed=9)
        ref = S.lpips(sd, net, x0, x1, True)[0].numpy()
        for f in S.LPIPS_FAULTS:
            d = np.min(np.abs(S.lpips(sd, net, x0, x1, True, faults=(f,))[0].numpy() - ref) / ref)
            assert d > 10 * TOL["lpips"], (net, f, d)
    a, b = S.pair(2, 64, 64, seed=12)
    ref = S.ssim(a, b)
    for f in S.SSIM_FAULTS:
        d = np.min(np.abs(S.ssim(a, b, faults=(f,)) - ref))
        assert d > 10 * TOL["ssim"], (f, d)


# ------------------------------------------------------------------------------------------- loader and folders
def test_loader_name_mapping_round_trip(tmp_path):
    from uspace_amd.tools.lpips import LPIPS, map_state_dict, state_dict_layout
    for net in ("alex", "vgg"):
        m, sd = _seeded(net)
        assert [(k, tuple(v.shape)) for k, v in sd.items()] == state_dict_layout(net)
        assert all(float(sd[f"lin{k}.weight"].min()) >= 0 for k in range(5))
        # the published naming: torchvision's features.N.* (+ its classifier) and lpips' lin{k}.model.1.weight [1, C, 1, 1]
        pub = {k: v for k, v in sd.items() if k.startswith("features.")}
        pub.update({f"lin{k}.model.1.weight": sd[f"lin{k}.weight"].reshape(1, -1, 1, 1) for k in range(5)})
        pub["classifier.1.weight"] = torch.zeros(4, 4)
        back = map_state_dict(pub, net)
        assert list(back) != [] and all(torch.equal(back[k], sd[k]) for k in sd) and set(back) == set(sd)
        path = str(tmp_path / f"{net}.pth")
        torch.save(pub, path)
        loaded = LPIPS(net, weights=path)
        assert all(torch.equal(v, sd[k]) for k, v in loaded.state_dict().items())
        with pytest.raises(KeyError):
            map_state_dict({k: v for k, v in pub.items() if k != "lin3.model.1.weight"}, net)
        with pytest.raises(KeyError):
            map_state_dict(dict(pub, **{"features.99.weight": torch.zeros(1)}), net)
        with pytest.raises(ValueError):
            map_state_dict(dict(pub, **{"lin0.model.1.weight": torch.zeros(1, 7, 1, 1)}), net)
    assert _seeded("alex")[1]["features.0.weight"].shape == (64, 3, 11, 11)


def test_loader_errors(tmp_path):
    from uspace_amd.tools.lpips import LPIPS
    from uspace_amd.tools.pair_metrics import PairMetrics
    with pytest.raises(FileNotFoundError):
        LPIPS("alex", weights=str(tmp_path / "missing.pth"))
    with pytest.raises(FileNotFoundError):
        LPIPS("vgg")
    with pytest.raises(ValueError):
        LPIPS("squeeze", seed=0)
    with pytest.raises(FileNotFoundError):
        PairMetrics(device="cpu").lpips                          # nothing is downloaded: no weights, no metric


def test_folder_pairing_errors(tmp_path):
    from PIL import Image
    from uspace_amd.tools.pair_metrics import calculate_pair_metrics_given_paths
    rng = np.random.default_rng(0)

    def write(folder, name, h=40, w=40):
        os.makedirs(folder, exist_ok=True)
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(folder, name))
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    for n in ("0.png", "1.png"):
        write(a, n)
        write(b, n)
    write(a, "2.png")
    with pytest.raises(ValueError) as e:
        calculate_pair_metrics_given_paths(a, b, device="cpu")
    assert "2" in str(e.value)
    write(b, "2.png", h=41)
    with pytest.raises(ValueError) as e:
        calculate_pair_metrics_given_paths(a, b, device="cpu")
    assert "size" in str(e.value)
    with pytest.raises(ValueError):
        calculate_pair_metrics_given_paths(str(tmp_path / "empty"), str(tmp_path / "empty"), device="cpu")
