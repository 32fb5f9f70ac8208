"""FID on the GPU: the Inception-v3 feature extractor of uspace_amd/tools/inception.py (csrc/inception.hip) against the
float64 restatement of tests/inception_stages.py, the fp64 statistics kernel against numpy, and the FID paths of
uspace_amd/tools/fid_score.py end to end.  All weights are seeded (the pretrained file is not available here).

Tolerances are about 3x what an MI355X measured; the measured values are written beside them.  Planted faults exceed
them by orders of magnitude.  Each is the numeric mutation applied to the restatement, compared with the unmutated GPU
features (end-to-end rel-L2 at 256^2, measured): count_include_pad=True, avg instead of max in Mixed_7c, BN eps 1e-5,
align_corners=True, 1x7 and 7x1 swapped, branch order swapped in Mixed_6b-6e's concat; the values are in FAULT_MEASURED.

Features are bit-identical per image across B = 1, 7, 50, 200 and under a NaN-filled workspace (measured: 0.0), and
the in-memory statistics of sampler output equal the PNG round trip's bit for bit (measured)."""
import os

import numpy as np
import pytest
import torch

from tests import inception_stages as S
from tests.util import rel_l2

pytestmark = pytest.mark.gpu

SIZES = [(256, 256), (299, 299), (137, 201)]
TOL = dict(
    resize=2.5e-5,       # measured 8.5e-6 (256^2), 0.0 (299^2: a copy), 7.1e-6 (137x201): the source index in fp32, as torch
    stage=2.5e-6,        # measured 8.3e-7: largest over stages 1-19 and the three sizes (Mixed_7c; Conv2d_1a 1.0e-7)
    e2e=2e-6,            # measured 6.7e-7 / 3.0e-7 / 5.9e-7: 2048-d features vs the fp64 forward from the raw input
    stats=1e-10,         # measured 6.9e-16 (GPU features) and 7.5e-16 (mean 1e3, std 1), worst batch split
    fid_path=1.6e-6,     # measured 5.3e-7 for both folder/folder and folder/.npz (FID 41.888)
)
# end-to-end rel-L2 of each planted fault at 256^2, measured (the test asks for > 10 x TOL["e2e"])
FAULT_MEASURED = dict(count_include_pad=4.3e-2, avg_7c=1.1e-1, eps_1e_5=1.2e-2, align_corners=4.4e-3, swap_1x7=8.6e-2,
                      swap_concat=4.4e-1)
FAULTS = ("count_include_pad", "avg_7c", "eps_1e-5", "align_corners", "swap_1x7", "swap_concat")


def _cpu_threads():
    torch.set_num_threads(min(torch.get_num_threads(), 16))


def _model(seed=0, blocks=(3,)):
    from uspace_amd.tools.inception import InceptionV3
    return InceptionV3(list(blocks), seed=seed).cuda()


def _sd(model):
    return {k: v.detach().cpu() for k, v in model.state_dict().items()}


def _images(n, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, 3, h, w, generator=g)


def _nchw(t):
    return t.permute(0, 3, 1, 2).double().cpu() if t.dim() == 4 else t.double().cpu()


# --------------------------------------------------------------------------------------------------------- measurements
def stage_errors(model=None, B=3):
    """{(H, W): [rel-L2 of stage s vs the restatement fed the GPU's stage s - 1, s = 0..19] + [end-to-end features]}."""
    _cpu_threads()
    model = model or _model()
    sd = _sd(model)
    out = {}
    for (h, w) in SIZES:
        x = _images(B, h, w, seed=h * 1000 + w)
        xd = x.cuda()
        errs = []
        prev = x.double()
        for s in range(20):
            got = _nchw(model.tap(xd, s))
            ref = S.stage(sd, s, prev)
            errs.append(rel_l2(got.numpy(), ref.numpy()))
            prev = got
        feat = model.features(xd).double().cpu()
        errs.append(rel_l2(feat.numpy(), S.forward(sd, x.double()).numpy()))
        out[(h, w)] = errs
    return out


def fault_distances(model=None, B=3):
    """{fault: rel-L2 of the mutated restatement's features vs the GPU features} at 256^2."""
    _cpu_threads()
    model = model or _model()
    sd = _sd(model)
    x = _images(B, 256, 256, seed=5)
    feat = model.features(x.cuda()).double().cpu().numpy()
    return {f: rel_l2(S.forward(sd, x.double(), faults=(f,)).numpy(), feat) for f in FAULTS}


def batch_diffs(model=None, n=200):
    """max |diff| of every image's 2048-d features between B = 200 (one launch sequence), 50, 7 and 1, and under a
    NaN-filled workspace."""
    model = model or _model()
    x = _images(n, 256, 256, seed=11).cuda()
    full = model.features(x, chunk=n)
    res = {}
    for c in (50, 7, 1):
        res[c] = float((model.features(x, chunk=c) - full).abs().max())
    ws = model._workspace(n, 256, 256, x.device)
    ws.view(torch.float32).fill_(float("nan"))
    again = model.features(x, chunk=n)
    res["nan_ws"] = float((again - full).abs().max()) if bool(torch.isfinite(again).all()) else float("nan")
    return res


def dims_diffs(model=None):
    """dims 64 / 192 / 768: max |features - spatial mean of the tap| (the tap summed in pixel order in fp64, rounded once)."""
    model = model or _model()
    from uspace_amd.tools.inception import BLOCK_STAGE
    x = _images(5, 256, 256, seed=3).cuda()
    res = {}
    for block in (0, 1, 2):
        feat = model.features(x, block).cpu().numpy()
        tap = model.tap(x, BLOCK_STAGE[block]).cpu().numpy().astype(np.float64)
        B, H, W, C = tap.shape
        mean = (np.cumsum(tap.reshape(B, H * W, C), axis=1)[:, -1] / (H * W)).astype(np.float32)
        res[block] = float(np.abs(feat - mean).max())
    return res


def stats_errors(model=None):
    """FIDStatistics vs np.mean / np.cov of the same fp32 features: GPU features of 200 images, and synthetic features
    with a large offset (mean 1e3, std 1); and the spread over batch splits."""
    from uspace_amd.tools.fid_score import FIDStatistics
    model = model or _model()
    feats = {"gpu": model.features(_images(200, 256, 256, seed=21).cuda())}
    g = torch.Generator().manual_seed(9)
    feats["offset"] = (1e3 + torch.randn(300, 2048, generator=g)).float().cuda()
    res = {}
    for name, f in feats.items():
        a = f.cpu().numpy().astype(np.float64)
        mu, sig = a.mean(0), np.cov(a, rowvar=False)
        per_split = []
        for split in ((len(a),), (50,) * (len(a) // 50), (7,) * (len(a) // 7) + ((len(a) % 7,) if len(a) % 7 else ())):
            st = FIDStatistics(2048, device="cuda", model=model)
            lo = 0
            for n in split:
                st.update_features(f[lo:lo + n])
                lo += n
            assert st.n == len(a)
            per_split.append((st.mu, st.sigma))
        res[name] = max(max(np.linalg.norm(m - mu) / np.linalg.norm(mu), np.linalg.norm(s - sig) / np.linalg.norm(sig))
                        for m, s in per_split)
    return res


def _write_pngs(path, imgs_u8):
    from PIL import Image
    os.makedirs(path, exist_ok=True)
    for i, a in enumerate(imgs_u8):
        Image.fromarray(a).save(os.path.join(path, f"{i}.png"))


def _restated_stats(sd, folder):
    """np.mean / np.cov of the fp64-restatement features of a folder's PNGs read as the FID path reads them."""
    import pathlib
    from PIL import Image
    from uspace_amd.tools.fid_score import IMAGE_EXTENSIONS
    files = sorted([f for ext in IMAGE_EXTENSIONS for f in pathlib.Path(folder).glob(f"*.{ext}")])
    x = torch.stack([torch.from_numpy(np.array(Image.open(f).convert("RGB"), dtype=np.uint8)).permute(2, 0, 1) for f in files])
    feats = []
    for lo in range(0, len(x), 16):
        feats.append(S.forward(sd, x[lo:lo + 16].float().double() / 255).numpy())
    a = np.concatenate(feats)
    return a.mean(0), np.cov(a, rowvar=False)


def fid_path_errors(tmp, model=None):
    """calculate_fid_given_paths on two folders of 64 PNGs, and folder vs .npz, vs the FID of fp64-restatement features."""
    _cpu_threads()
    from uspace_amd.tools.fid_score import calculate_fid_given_paths, calculate_frechet_distance
    model = model or _model()
    sd = _sd(model)
    rng = np.random.default_rng(77)
    a = rng.integers(0, 256, (64, 48, 48, 3), dtype=np.uint8)
    b = np.clip(rng.normal(150, 40, (64, 48, 48, 3)), 0, 255).astype(np.uint8)
    pa, pb = os.path.join(tmp, "a"), os.path.join(tmp, "b")
    _write_pngs(pa, a)
    _write_pngs(pb, b)
    fid = calculate_fid_given_paths((pa, pb), device="cuda", batch_size=32, num_workers=0, model=model)
    from uspace_amd.tools.fid_score import compute_statistics_of_path
    mb, sb = compute_statistics_of_path(pb, model, 32, 2048, "cuda", 0)
    npz = os.path.join(tmp, "b.npz")
    np.savez(npz, mu=mb, sigma=sb)
    fid_npz = calculate_fid_given_paths((pa, npz), device="cuda", batch_size=32, num_workers=0, model=model)
    ref = calculate_frechet_distance(*_restated_stats(sd, pa), *_restated_stats(sd, pb))
    return dict(fid=float(fid), fid_npz=float(fid_npz), ref=float(ref), rel=abs(fid - ref) / abs(ref),
                rel_npz=abs(fid_npz - ref) / abs(ref))


class _OneProcess:
    num_processes = 1
    is_main_process = True

    def gather(self, t):
        return t


def sampler_chain(tmp, n=64, bs=32):
    """Seeded U-ViT euler solve -> seeded SD-shape VAE decode: (FIDStatistics.update mu, sigma) and (sample2dir ->
    compute_statistics_of_path mu, sigma) on the same images."""
    import pathlib
    from uspace_amd.flow_matching import CNF
    from uspace_amd.libs.autoencoder import FrozenAutoencoderKL
    from uspace_amd.tools.fid_score import IMAGE_EXTENSIONS, FIDStatistics, compute_statistics_of_path
    from uspace_amd.tools.utils_uvit import get_nnet, sample2dir
    model = _model(seed=4)
    torch.manual_seed(41)
    dd = dict(double_z=True, z_channels=4, resolution=256, in_channels=3, out_ch=3, ch=128, ch_mult=[1, 2, 4, 4],
              num_res_blocks=2, attn_resolutions=[], dropout=0.0)
    vae = FrozenAutoencoderKL(dd, 4).cuda()
    net = get_nnet("uvit", num_classes=-1, img_size=32, patch_size=2, in_chans=4, embed_dim=64, depth=2, num_heads=1,
                   mlp_ratio=4, qkv_bias=False, mlp_time_embed=False).cuda().eval()
    cnf = CNF(net)
    g = torch.Generator().manual_seed(6)
    noise = torch.randn(n, 4, 32, 32, generator=g).cuda()
    kw = dict(edit_loc=None, dissect_name="none", solver_kwargs=dict(solver="fixed", solver_fix="euler", solver_fix_step=0.25))
    with torch.no_grad():
        z = cnf.decode(noise, None, **kw)
        imgs = (vae.decode(z) * 0.5 + 0.5).clamp(0, 1)
    starts = iter(range(0, n, bs))

    def sample_fn(m):
        lo = next(starts)
        return imgs[lo:lo + m]
    path = os.path.join(tmp, "samples")
    sample2dir(_OneProcess(), path, n, bs, sample_fn)
    files = sorted([f for ext in IMAGE_EXTENSIONS for f in pathlib.Path(path).glob(f"*.{ext}")])
    order = [int(f.stem) for f in files]
    st = FIDStatistics(2048, device="cuda", model=model)
    for lo in range(0, n, bs):                     # the PNG path's batches: files in sorted (lexicographic) order
        st.update(imgs[order[lo:lo + bs]])
    m2, s2 = compute_statistics_of_path(path, model, bs, 2048, "cuda", 0)
    return (st.mu, st.sigma), (m2, s2), float(imgs.std())


# ------------------------------------------------------------------------------------------------------------------ tests
def test_stage_parity_every_stage_three_sizes():
    for size, errs in stage_errors().items():
        assert errs[0] < TOL["resize"], (size, 0, errs[0])
        for s, e in enumerate(errs[1:20], 1):
            assert e < TOL["stage"], (size, s, e)
        assert errs[20] < TOL["e2e"], (size, "features", errs[20])


def test_planted_faults_exceed_tolerances():
    for f, d in fault_distances().items():
        assert d > 10 * TOL["e2e"], (f, d)


def test_features_bit_identical_across_batch_sizes_and_nan_workspace():
    for k, d in batch_diffs().items():
        assert d == 0.0, (k, d)


def test_lower_dims_are_the_spatial_mean_of_their_tap():
    for block, d in dims_diffs().items():
        assert d == 0.0, (block, d)


def test_fid_statistics_match_numpy_cov_for_every_batch_split():
    for name, e in stats_errors().items():
        assert e < TOL["stats"], (name, e)


def test_fid_of_folders_and_npz_matches_restated_features(tmp_path):
    r = fid_path_errors(str(tmp_path))
    assert r["rel"] < TOL["fid_path"], r
    assert r["rel_npz"] < TOL["fid_path"], r


def test_in_memory_statistics_equal_png_round_trip(tmp_path):
    (m1, s1), (m2, s2), spread = sampler_chain(str(tmp_path))
    assert spread > 1e-3
    assert np.array_equal(m1, m2) and np.array_equal(s1, s2)


def test_cpu_tensor_fails_loudly():
    from uspace_amd import _hip
    model = _model()
    with pytest.raises(_hip.UspaceHipError):
        model.features(torch.rand(1, 3, 32, 32))
