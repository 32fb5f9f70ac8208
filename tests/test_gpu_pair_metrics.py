"""Paired edit-fidelity metrics on the GPU: LPIPS (uspace_amd/tools/lpips.py), SSIM and PSNR (uspace_amd/tools/pair_metrics.py)
on the kernels of csrc/lpips.hip against the float64 restatement of tests/lpips_stages.py.  All weights are seeded (the
pretrained files are not available here).

Tolerances are about 3x what an MI355X measured; the measured values are written beside them.  LPIPS figures are relative
(rel-L2 of activations, |gpu - ref| / ref of distances), SSIM absolute, PSNR absolute in dB.  Planted faults are numeric
mutations of the restatement compared with the unmutated GPU result; each must exceed 10x the tolerance of the quantity it
moves, and the measured distances are in FAULT_MEASURED.

Per-image LPIPS, SSIM and PSNR are bit-identical across B = 1, 3, 16, across ``chunk`` settings and under a NaN-filled
workspace (measured: 0.0 everywhere)."""
import numpy as np
import pytest
import torch

from tests import lpips_stages as S
from tests.util import rel_l2

pytestmark = pytest.mark.gpu
TOL = dict(
    head=3.5e-7,         # measured 1.1e-7: largest over the 18 cases and the zero-vector case (relative, per image)
    scale=1.5e-7,        # measured 4.5e-8: tap stage 0, rel-L2, the five cases
    stage=4e-6,          # measured 1.3e-6: largest over stages 1-5 and the five cases (vgg stage 4; alex 7.5e-7 at most)
    lpips=8e-7,          # measured 2.6e-7 / 7.1e-8 / 1.9e-7 / 9.6e-8 / 4.8e-8: the distance end to end, relative, per image
    layers=3e-5,         # measured 1.0e-5: one layer's term end to end (vgg 32^2, the 2 x 2 map after 13 convolutions; alex 2.9e-6)
    ssim=6e-7,           # measured 2.0e-7 at 11 x 11 (a single window), 3.9e-8 at 12 x 29, 8.7e-9 at 64^2, 1.2e-8 with L = 255; absolute
    psnr=1e-10,          # dB, absolute.  Measured 0.0; all arithmetic is fp64, so the bound is 10 / ln 10 * n * 2^-53 = 6e-12 at n = 12 288
)
# smallest distance over the images of each planted fault, measured (the test asks for > 10 x TOL["lpips"] resp. TOL["ssim"])
FAULT_MEASURED = dict(
    alex=dict(no_scaling=1.0e-1, tap_before_relu=5.3e-2, ceil_mode=3.6e-3, normalize_after_diff=45.0, w_before_square=0.98,
              ignore_normalize=0.81),
    vgg=dict(no_scaling=2.9e-2, tap_before_relu=1.6e-1, ceil_mode=4.5e-3, normalize_after_diff=41.0, w_before_square=0.98,
             ignore_normalize=0.78),
    ssim=dict(uniform_window=7.5e-4, sigma_1=1.3e-3, same_padding=1.3e-3, k2_0_01=1.0e-4),
)


def _cpu_threads():
    torch.set_num_threads(min(torch.get_num_threads(), 16))


_MODELS = {}


def _model(net):
    from uspace_amd.tools.lpips import LPIPS
    if net not in _MODELS:
        _MODELS[net] = LPIPS(net, seed=3).cuda()
    return _MODELS[net]


def _sd(model):
    return {k: v.detach().cpu() for k, v in model.state_dict().items()}


def _nchw(t):
    return t.permute(0, 3, 1, 2).double().cpu()


def _rel(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.max(np.abs(got - ref) / np.abs(ref)))


# --------------------------------------------------------------------------------------------------------- measurements
def _features(B, HW, C, seed):
    """ReLU-like non-negative features (about half the entries are zero) [B, HW, C] for both sides."""
    g = torch.Generator().manual_seed(seed)
    f0 = torch.relu(torch.randn(B, HW, C, generator=g))
    f1 = torch.relu(f0 + 0.3 * torch.randn(B, HW, C, generator=g))
    w = torch.rand(C, generator=g) * (2.0 / C)
    return f0, f1, w


def _head_ref(f0, f1, w):
    return S.distance(f0.permute(0, 2, 1)[..., None], f1.permute(0, 2, 1)[..., None], w).numpy()


def head_errors():
    """{(B, HW, C): max over b of |gpu - ref| / ref} of the distance head alone, plus "zero_vector" (one side's vector all zero
    at pixel 0 of every image; B = 3, HW = 9, C = 192) and "identical" (the largest value for identical inputs: must be 0.0)."""
    from uspace_amd.tools.lpips import lpips_distance
    out = {}
    for i, (B, HW, C) in enumerate(S.HEAD_CASES):
        f0, f1, w = _features(B, HW, C, 100 + i)
        out[(B, HW, C)] = _rel(lpips_distance(f0.cuda(), f1.cuda(), w.cuda()).cpu().numpy(), _head_ref(f0, f1, w))
    f0, f1, w = _features(3, 9, 192, 77)
    f0[:, 0, :] = 0
    got = lpips_distance(f0.cuda(), f1.cuda(), w.cuda()).cpu().numpy()
    assert np.isfinite(got).all()
    out["zero_vector"] = _rel(got, _head_ref(f0, f1, w))
    f0, _, w = _features(3, 225, 512, 78)
    out["identical"] = float(lpips_distance(f0.cuda(), f0.clone().cuda(), w.cuda()).abs().max())
    return out


def _case_inputs(net, B, H, W):
    """(x0, x1, normalize): alex sees images in [0, 1] with normalize=True, vgg the same pair mapped to [-1, 1]."""
    a, b = S.pair(B, H, W, seed=H * 1000 + W)
    return (a, b, True) if net == "alex" else (2 * a - 1, 2 * b - 1, False)


def backbone_errors(case):
    """dict(scale, stages [5], lpips, layers) for one of S.BACKBONE_CASES: rel-L2 of tap stage 0, of every stage against the
    restatement fed the GPU's previous stage, and the largest relative error of the distance (total, per layer) end to end."""
    _cpu_threads()
    net, B, H, W = case
    model = _model(net)
    sd = _sd(model)
    x0, x1, normalize = _case_inputs(net, B, H, W)
    d0, d1 = x0.cuda(), x1.cuda()
    prev = _nchw(model.tap(d0, d1, 0, normalize=normalize))
    res = dict(scale=rel_l2(prev.numpy(), S.scaled(torch.cat([x0, x1]), normalize).numpy()), stages=[])
    for s in range(1, 6):
        got = _nchw(model.tap(d0, d1, s, normalize=normalize))
        res["stages"].append(rel_l2(got.numpy(), S.stage(sd, net, s, prev).numpy()))
        prev = got
    total, layers = model(d0, d1, normalize=normalize, per_layer=True)
    ref_total, ref_layers = S.lpips(sd, net, x0, x1, normalize)
    res["lpips"] = _rel(total.cpu().numpy(), ref_total.numpy())
    res["layers"] = _rel(layers.cpu().numpy(), ref_layers.numpy())
    res["sum"] = float((layers.sum(0) - total).abs().max() / total.abs().max())
    return res


def lpips_fault_distances(net, H, W):
    """{fault: smallest |mutated restatement - gpu| / gpu over the images} of the LPIPS faults at an odd size, normalize=True."""
    _cpu_threads()
    model = _model(net)
    sd = _sd(model)
    x0, x1 = S.pair(2, H, W, seed=9)
    got = model(x0.cuda(), x1.cuda(), normalize=True).cpu().numpy()
    return {f: float(np.min(np.abs(S.lpips(sd, net, x0, x1, True, faults=(f,))[0].numpy() - got) / np.abs(got))) for f in S.LPIPS_FAULTS}


def ssim_errors():
    """{(B, C, H, W): max |gpu - ref|} plus "identical": max |gpu(x, x) - 1| over the cases."""
    from uspace_amd.tools.pair_metrics import ssim
    out, ident = {}, 0.0
    for case in S.SSIM_CASES:
        B, C, H, W = case
        a, b = S.pair(B, H, W, seed=H * 100 + W + B, c=C)
        out[case] = float(np.max(np.abs(ssim(a.cuda(), b.cuda()).cpu().numpy() - S.ssim(a, b))))
        ident = max(ident, float((ssim(a.cuda(), a.clone().cuda()) - 1).abs().max()))
    a, b = S.pair(2, 40, 52, seed=5)
    out["range255"] = float(np.max(np.abs(ssim((a * 255).cuda(), (b * 255).cuda(), 255.0).cpu().numpy() - S.ssim(a * 255, b * 255, 255.0))))
    out["identical"] = ident
    return out


def ssim_fault_distances():
    from uspace_amd.tools.pair_metrics import ssim
    a, b = S.pair(2, 64, 64, seed=12)
    got = ssim(a.cuda(), b.cuda()).cpu().numpy()
    return {f: float(np.min(np.abs(S.ssim(a, b, faults=(f,)) - got))) for f in S.SSIM_FAULTS}


def psnr_errors():
    """dict(random: max |gpu - ref| in dB at three sizes (one beyond a partial sum's 4096 elements and no multiple of it),
    offset: |gpu - closed form| for a constant offset, identical: the value for identical images)."""
    from uspace_amd.tools.pair_metrics import psnr
    out = dict(random=0.0)
    for (B, H, W) in ((1, 11, 11), (3, 37, 41), (2, 64, 64)):
        a, b = S.pair(B, H, W, seed=H + W)
        out["random"] = max(out["random"], float(np.max(np.abs(psnr(a.cuda(), b.cuda()).cpu().numpy() - S.psnr(a, b)))))
    a = (256 + 512 * S.images(2, 33, 47, seed=2)).round() / 1024      # multiples of 2^-10 in [0.25, 0.75]
    delta = 2.0 ** -5                                                 # so a + delta is exact in fp32, also times 255
    got = psnr(a.cuda(), (a + delta).cuda()).cpu().numpy()
    out["offset"] = float(np.max(np.abs(got - (-20 * np.log10(delta)))))
    out["offset_range255"] = float(np.max(np.abs(psnr((a * 255).cuda(), ((a + delta) * 255).cuda(), 255.0).cpu().numpy()
                                                 - S.psnr(a * 255, (a + delta) * 255, 255.0))))
    out["identical"] = psnr(a.cuda(), a.clone().cuda()).cpu().numpy().tolist()
    return out


def batch_diffs():
    """Largest |difference| of every pair's LPIPS (alex 64^2, vgg 32^2), SSIM and PSNR between B = 16 in one launch sequence and
    B = 3 / B = 1 (``chunk`` for LPIPS, slices for SSIM and PSNR), and under NaN-filled workspaces."""
    from uspace_amd import _hip
    from uspace_amd.tools.pair_metrics import psnr, ssim
    res = {}
    for net, size in (("alex", 64), ("vgg", 32)):
        model = _model(net)
        a, b = (t.cuda() for t in S.pair(16, size, size, seed=21))
        full, full_layers = model(a, b, normalize=True, per_layer=True, chunk=16)
        for c in (3, 1):
            t, l = model(a, b, normalize=True, per_layer=True, chunk=c)
            res[(net, "chunk", c)] = max(float((t - full).abs().max()), float((l - full_layers).abs().max()))
        res[(net, "default_chunk")] = float((model(a, b, normalize=True) - full).abs().max())
        res[(net, "moved")] = float((model(a[5:8], b[5:8], normalize=True) - full[5:8]).abs().max())
        ws = model._workspace(16, size, size, a.device)
        ws.view(torch.float32).fill_(float("nan"))
        again = model(a, b, normalize=True, chunk=16)
        res[(net, "nan_ws")] = float((again - full).abs().max()) if bool(torch.isfinite(again).all()) else float("nan")
    a, b = (t.cuda() for t in S.pair(16, 40, 52, seed=22))
    L = _hip.lib()
    for name, fn, nbytes in (("ssim", ssim, L.uspace_ssim_workspace_bytes(16, 3, 40, 52)),
                             ("psnr", psnr, L.uspace_psnr_workspace_bytes(16, 3 * 40 * 52))):
        full = fn(a, b)
        res[(name, 3)] = max(float((fn(a[lo:lo + 3], b[lo:lo + 3]) - full[lo:lo + 3]).abs().max()) for lo in range(0, 15, 3))
        res[(name, 1)] = max(float((fn(a[i:i + 1], b[i:i + 1]) - full[i:i + 1]).abs().max()) for i in range(16))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=a.device)
        ws.view(torch.float64).fill_(float("nan"))
        again = fn(a, b, ws=ws)
        res[(name, "nan_ws")] = float((again - full).abs().max()) if bool(torch.isfinite(again).all()) else float("nan")
    return res


def _tiny_chain():
    """The tiny U-ViT and VAE of tests/test_gpu_vae_encoder.py's edit chain, Euler with few steps."""
    from uspace_amd.flow_matching import CNF
    from uspace_amd.libs.autoencoder import FrozenAutoencoderKL
    from uspace_amd.tools.utils_uvit import get_nnet
    dd = dict(double_z=True, z_channels=4, resolution=64, in_channels=3, out_ch=3, ch=64, ch_mult=[1, 2, 2], num_res_blocks=1,
              attn_resolutions=[], dropout=0.0)
    torch.manual_seed(31)
    vae = FrozenAutoencoderKL(dd, 4, encoder=True).cuda()
    net = get_nnet("uvit", num_classes=-1, img_size=16, patch_size=2, in_chans=4, embed_dim=64, depth=2, num_heads=1,
                   mlp_ratio=4, qkv_bias=False, mlp_time_embed=False).cuda().eval()
    kw = dict(edit_loc=None, dissect_name="none", solver_kwargs=dict(solver="fixed", solver_fix="euler", solver_fix_step=0.25))
    return CNF(net), vae, kw


# ------------------------------------------------------------------------------------------------------------------ tests
def test_head_kernel_alone_matches_the_formula():
    errs = head_errors()
    print("head_errors", errs)
    assert errs.pop("identical") == 0.0
    for k, e in errs.items():
        assert e < TOL["head"], (k, e)


@pytest.mark.parametrize("case", S.BACKBONE_CASES, ids=lambda c: f"{c[0]}-B{c[1]}-{c[2]}x{c[3]}")
def test_backbone_stage_by_stage_and_end_to_end(case):
    r = backbone_errors(case)
    print("backbone_errors", case, r)
    assert r["scale"] < TOL["scale"], r
    for s, e in enumerate(r["stages"], 1):
        assert e < TOL["stage"], (s, e)
    assert r["lpips"] < TOL["lpips"] and r["layers"] < TOL["layers"], r
    assert r["sum"] < 1e-15, r                     # the total is the five layers summed in fp64 (measured 0.0)


def test_per_image_values_bit_identical_across_batches_chunks_and_nan_workspace():
    for k, d in batch_diffs().items():
        assert d == 0.0, (k, d)


def test_ssim_matches_restatement_and_identical_images_give_one():
    from uspace_amd import _hip
    from uspace_amd.tools.pair_metrics import ssim
    errs = ssim_errors()
    print("ssim_errors", errs)
    assert errs.pop("identical") < TOL["ssim"]      # |ssim(x, x) - 1|, measured 0.0
    for k, e in errs.items():
        assert e < TOL["ssim"], (k, e)
    x = torch.rand(1, 3, 10, 10).cuda()
    with pytest.raises(_hip.UspaceHipError):
        ssim(x, x)
    with pytest.raises(_hip.UspaceHipError):
        ssim(torch.rand(1, 3, 64, 10).cuda(), torch.rand(1, 3, 64, 10).cuda())


def test_psnr_closed_forms():
    r = psnr_errors()
    print("psnr_errors", r)
    assert r["identical"] == [float("inf")] * 2
    assert r["offset"] < TOL["psnr"] and r["offset_range255"] < TOL["psnr"] and r["random"] < TOL["psnr"], r


def test_pair_metrics_means_quantisation_and_reset():
    from uspace_amd.tools.pair_metrics import PairMetrics, psnr, ssim
    model = _model("alex")
    pm = PairMetrics(device="cuda", lpips=model)
    a, b = (t.cuda() for t in S.pair(5, 64, 64, seed=31))
    pm.update(a[:3], b[:3])
    pm.update(a[3:], b[3:])
    v, out = pm.values, pm.compute()
    assert out["n"] == 5 == pm.n and all(v[k].shape == (5,) and v[k].dtype == np.float64 for k in ("lpips", "ssim", "psnr"))
    for k in ("lpips", "ssim", "psnr"):
        assert out[k] == float(np.mean(v[k])), k
    # quantize=True is the uint8 round trip done by hand
    qa, qb = ((t * 255 + 0.5).clamp(0, 255).to(torch.uint8).float() / 255 for t in (a, b))
    assert np.array_equal(v["lpips"], model(qa, qb, normalize=True).cpu().numpy())
    assert np.array_equal(v["ssim"], ssim(qa, qb).cpu().numpy()) and np.array_equal(v["psnr"], psnr(qa, qb).cpu().numpy())
    raw = PairMetrics(device="cuda", lpips=model)
    raw.update(a, b, quantize=False)
    assert np.array_equal(raw.values["psnr"], psnr(a, b).cpu().numpy()) and not np.array_equal(raw.values["psnr"], v["psnr"])
    pm.reset()
    assert pm.n == 0
    with pytest.raises(ValueError):
        pm.compute()


def test_reconstruction_fidelity_is_the_composition_of_existing_calls():
    from uspace_amd.tools.pair_metrics import PairMetrics, reconstruction_fidelity
    cnf, vae, kw = _tiny_chain()
    model = _model("alex")
    img = S.images(2, 64, 64, seed=4).cuda()
    torch.manual_seed(8)
    pm = PairMetrics(device="cuda", lpips=model)
    got = reconstruction_fidelity(cnf, vae, img, None, metrics=pm, **kw)
    torch.manual_seed(8)
    z = vae.encode(img * 2 - 1)
    rec = (vae.decode(cnf.decode(cnf.encode(z, None, **kw), None, **kw)) * 0.5 + 0.5).clamp(0, 1)
    by_hand = PairMetrics(device="cuda", lpips=model)
    by_hand.update(img, rec)
    assert got == by_hand.compute() and got["n"] == 2 and np.isfinite([got["lpips"], got["ssim"], got["psnr"]]).all()
    for k in ("lpips", "ssim", "psnr"):
        assert np.array_equal(pm.values[k], by_hand.values[k]), k


def test_planted_faults_exceed_tolerances():
    for net, (H, W) in (("alex", (70, 95)), ("vgg", (38, 51))):
        d = lpips_fault_distances(net, H, W)
        print("lpips_fault_distances", net, d)
        for f, v in d.items():
            assert v > 10 * TOL["lpips"], (net, f, v)
    d = ssim_fault_distances()
    print("ssim_fault_distances", d)
    for f, v in d.items():
        assert v > 10 * TOL["ssim"], (f, v)


def test_cpu_tensor_and_unknown_net_fail_loudly():
    from uspace_amd import _hip
    from uspace_amd.tools.lpips import LPIPS
    from uspace_amd.tools.pair_metrics import psnr
    with pytest.raises(_hip.UspaceHipError):
        _model("alex")(torch.rand(1, 3, 64, 64), torch.rand(1, 3, 64, 64))
    with pytest.raises(_hip.UspaceHipError):
        psnr(torch.rand(1, 3, 8, 8), torch.rand(1, 3, 8, 8))
    with pytest.raises(_hip.UspaceHipError):
        _model("alex")(torch.rand(1, 3, 30, 30).cuda(), torch.rand(1, 3, 30, 30).cuda())      # too small for AlexNet's pools
    with pytest.raises(ValueError):
        LPIPS("squeeze", seed=0)
