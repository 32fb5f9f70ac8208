"""VAE encode on the GPU: FrozenAutoencoderKL.encode_moments / sample / encode of the reference (libs/autoencoder.py:215-300,
428-458) through the C-ABI, against the reference's fixtures (tests/golden/vae_encoder_*.npz), the float64 stage reference
of tests/vae_encoder_stages.py, torch's own stride-2 convolution and RNG, and itself (batch invariance).

Tolerances are about 3x what an MI355X measured; the measured values are written beside them.  Planted faults exceed them:
downsample pad on the wrong side and phase maps in the wrong order (downsample 1.15, tiny moments 1.01 / 0.93), RGB read as
BGR (conv_in 1.24, tiny conv_in tap 1.40), logvar not clamped (sample 1e28 ulps), quant_conv transposed (tiny moments 1.09)."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.util import rel_l2

pytestmark = pytest.mark.gpu

SD_DDCONFIG = dict(double_z=True, z_channels=4, resolution=256, in_channels=3, out_ch=3, ch=128,
                   ch_mult=[1, 2, 4, 4], num_res_blocks=2, attn_resolutions=[], dropout=0.0)

TOL = dict(
    tiny_moments=2.4e-2,    # measured 7.8e-3 (bf16 operands through 9 stages, fp32 elsewhere)
    tiny_tap=2.4e-2,        # measured 7.7e-3 (largest over the 9 stages, on the fixture's 8 channels; conv_in 1.3e-7)
    tiny_rec=5.7e-2,        # measured 1.9e-2: decode(mean * scale) of the GPU moments vs the reference's reconstruction
    tiny_z=5.8e-3,          # measured 1.9e-3: sample with the stored eps vs the reference's z
    sd_moments=2.9e-2,      # measured 9.6e-3: default-init SD encoder vs the reference's fp32 CPU moments
    downsample=7.5e-7,      # measured 1.4e-7 / 1.8e-7 / 2.4e-7 at C = 128 / 256 / 512, vs F.pad + F.conv2d(stride 2) in
                            # float64 on the bf16-rounded operands
    conv_in=3.1e-7,         # measured 1.0e-7
    sample_ulps=2.0,        # measured 1.37 ulps of |mean| + |std * eps| (the issue's bound; a missing clamp gives 1e28)
)
# SD shape, per stage (0 conv_in, 1-2 down.0 blocks, 3 downsample, 4-5 down.1, 6 downsample, 7-8 down.2, 9 downsample,
# 10-11 down.3, 12 mid.block_1, 13 mid.attn_1, 14 mid.block_2): tight = bf16 mode, loose = pure float64 (float32 at 256^2)
SD_STAGES = [(256, 128)] * 3 + [(128, 128), (128, 256), (128, 256), (64, 256), (64, 512), (64, 512)] + [(32, 512)] * 6
STAGE_TOL = dict(
    # measured:  1.2e-7  9.1e-5  6.8e-5  1.9e-7  8.0e-5  7.4e-5  2.8e-7  8.1e-5  7.0e-5  4.0e-7  1.1e-4  8.9e-5  5.1e-5  8.1e-5  5.0e-5
    tight=[3.6e-7, 2.7e-4, 2.1e-4, 5.7e-7, 2.4e-4, 2.2e-4, 8.4e-7, 2.4e-4, 2.1e-4, 1.2e-6, 3.5e-4, 2.7e-4, 1.6e-4, 2.4e-4, 1.5e-4],
    # measured:  1.2e-7  2.9e-3  2.2e-3  2.2e-3  3.1e-3  2.3e-3  2.3e-3  3.2e-3  2.2e-3  2.2e-3  2.5e-3  2.0e-3  1.6e-3  1.3e-3  1.4e-3
    loose=[3.6e-7, 8.6e-3, 6.6e-3, 6.7e-3, 9.5e-3, 7.0e-3, 7.0e-3, 9.6e-3, 6.6e-3, 6.7e-3, 7.5e-3, 6.0e-3, 5.0e-3, 3.8e-3, 4.2e-3],
)
QK_GAIN = 2.0


def _fixture(golden_dir, name):
    z = np.load(os.path.join(golden_dir, name))
    return z, json.loads(bytes(z["meta_json"]).decode())


def _cpu_threads():
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 16))
    return n


def _sample_with(vae, moments, eps):
    """The HIP sample kernel with a given eps (what vae.sample runs after drawing eps)."""
    from uspace_amd import _hip
    m = moments.contiguous()
    e = eps.to(torch.float32).contiguous().cuda()
    B, h = m.shape[0], m.shape[2]
    z = torch.empty(B, 4, h, h, dtype=torch.float32, device=m.device)
    _hip.check(_hip.lib().uspace_vae_sample(_hip.ptr(m), _hip.ptr(e), float(vae.scale_factor), _hip.ptr(z), B, h,
                                            _hip.stream_ptr()), "uspace_vae_sample")
    return z


# ------------------------------------------------------------------------------------------------------------------ 1
def tiny_errors(golden_dir):
    from tests import vae_encoder_stages as E
    from uspace_amd.libs.autoencoder import FrozenAutoencoderKL
    z, meta = _fixture(golden_dir, "vae_encoder_tiny.npz")
    torch.manual_seed(meta["weight_seed"])
    vae = FrozenAutoencoderKL(meta["ddconfig"], 4, encoder=True).cuda()
    x = torch.from_numpy(z["x"]).cuda()
    x0 = x.clone()
    m = vae.encode_moments(x)
    out = dict(moments=rel_l2(m.cpu().numpy(), z["moments"]), input_untouched=bool(torch.equal(x, x0)))
    names = meta["taps"][:-1]
    nc = meta["tap_channels"]                 # the fixture keeps channels 0, C/nc, 2C/nc, ... of every tap
    taps = [vae.encode_tap(x, k).cpu() for k in range(len(names))]
    out["taps"] = [rel_l2(t[:, :: t.shape[1] // nc].numpy(), z[f"tap/{n}"]) for t, n in zip(taps, names)]
    zz = _sample_with(vae, m, torch.from_numpy(z["eps"]))
    out["z"] = rel_l2(zz.cpu().numpy(), z["z"])
    mean = torch.chunk(m, 2, dim=1)[0]
    out["rec"] = rel_l2(vae.decode(mean * meta["scale_factor"]).cpu().numpy(), z["rec"])
    out["repeat_equal"] = bool(torch.equal(vae.encode_moments(x), m)) and bool(torch.equal(vae(x, "encode_moments"), m))
    out["chunk1_equal"] = bool(torch.equal(vae.encode_moments(x, chunk=1), m))
    spec = E.EncSpec.from_ddconfig(meta["ddconfig"])
    assert len(spec.stages) == len(names)
    return out


def test_tiny_encoder_matches_reference_golden(golden_dir):
    r = tiny_errors(golden_dir)
    assert r["moments"] < TOL["tiny_moments"], r
    assert max(r["taps"]) < TOL["tiny_tap"], r
    assert r["z"] < TOL["tiny_z"] and r["rec"] < TOL["tiny_rec"], r
    assert r["input_untouched"] and r["repeat_equal"] and r["chunk1_equal"], r


# ------------------------------------------------------------------------------------------------------------------ 2
def sd_vae_every_parameter_counts(seed=1234):
    """The SD autoencoder with the encoder, seeded, with every parameter visible: GroupNorm gamma ~ N(1, 0.2),
    beta ~ N(0, 0.3), conv biases ~ N(0, 0.05), and the encoder's mid-block q / k weights scaled by QK_GAIN."""
    from uspace_amd.libs.autoencoder import FrozenAutoencoderKL
    torch.manual_seed(seed)
    vae = FrozenAutoencoderKL(SD_DDCONFIG, 4, encoder=True)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, p in vae.named_parameters():
            if name.split(".")[-2].startswith("norm"):
                if name.endswith("weight"):
                    p.copy_(1.0 + 0.2 * torch.randn(p.shape, generator=g))
                else:
                    p.copy_(0.3 * torch.randn(p.shape, generator=g))
            elif name.endswith("bias"):
                p.copy_(0.05 * torch.randn(p.shape, generator=g))
        for n in ("q", "k"):
            getattr(vae.encoder.mid.attn_1, n).weight.mul_(QK_GAIN)
    return vae.cuda()


def sd_stage_errors(vae, x):
    """Per stage: {k, H, C, tight, loose}, every stage fed the GPU's previous tap."""
    from tests import vae_encoder_stages as E
    spec = E.EncSpec.from_ddconfig(SD_DDCONFIG)
    sd = {k: v.detach().cpu() for k, v in vae.state_dict().items()}
    dt = lambda H: torch.float32 if H == 256 else torch.float64
    xc = x.cuda()
    n = _cpu_threads()
    try:
        out, prev = [], x
        for k, (_, _, H, Cc) in enumerate(spec.stages):
            got = vae.encode_tap(xc, k).cpu()
            row = dict(k=k, H=int(got.shape[2]), C=int(got.shape[1]), shape_ok=tuple(got.shape) == (x.shape[0], Cc, H, H))
            if row["shape_ok"]:
                row["tight"] = rel_l2(got.numpy(), E.run_stage(spec, sd, k, prev, bf16=True, dtype=dt(H)).numpy())
                row["loose"] = rel_l2(got.numpy(), E.run_stage(spec, sd, k, prev, bf16=False, dtype=dt(H)).numpy())
            out.append(row)
            prev = got
        return out
    finally:
        torch.set_num_threads(n)


def sd_moments_error(golden_dir):
    from uspace_amd.libs.autoencoder import FrozenAutoencoderKL
    z, meta = _fixture(golden_dir, "vae_encoder_sd.npz")
    torch.manual_seed(meta["weight_seed"])
    vae = FrozenAutoencoderKL(meta["ddconfig"], 4, encoder=True).cuda()
    m = vae.encode_moments(torch.from_numpy(z["x_fp16"]).float().cuda())
    return rel_l2(m.cpu().numpy(), z["moments"])


def test_sd_encoder_stage_parity_against_fp64_reference(golden_dir):
    from tests import vae_encoder_stages as E
    spec = E.EncSpec.from_ddconfig(SD_DDCONFIG)
    assert [(h, c) for _, _, h, c in spec.stages] == SD_STAGES
    z, _ = _fixture(golden_dir, "vae_encoder_sd.npz")
    vae = sd_vae_every_parameter_counts()
    for r, (H, Cc) in zip(sd_stage_errors(vae, torch.from_numpy(z["x_fp16"]).float()), SD_STAGES):
        assert (r["H"], r["C"]) == (H, Cc) and r["shape_ok"], r
        assert r["tight"] < STAGE_TOL["tight"][r["k"]], r
        assert r["loose"] < STAGE_TOL["loose"][r["k"]], r
    assert sd_moments_error(golden_dir) < TOL["sd_moments"]


# ------------------------------------------------------------------------------------------------------------------ 3
def downsample_error(C, H, B, seed=3):
    """One Downsample at (C, H): an encoder with no res blocks (conv_in -> downsample), conv_in set to copy image channel
    c % 3 times a per-channel gain, so the downsample's input is a map chosen here; the last image row and column are
    large so a pad on the wrong side (or a shifted phase) shows.  The GPU's own conv_in tap is the input of the check."""
    from uspace_amd.libs.autoencoder import FrozenAutoencoderKL
    dd = dict(SD_DDCONFIG, ch=C, ch_mult=[1, 1, 1], num_res_blocks=0, resolution=H)
    torch.manual_seed(seed)
    vae = FrozenAutoencoderKL(dd, 4, encoder=True)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        w = torch.zeros(C, 3, 3, 3)
        for c in range(C):
            w[c, c % 3, 1, 1] = 0.5 + torch.rand(1, generator=g).item()
        vae.encoder.conv_in.weight.copy_(w)
        vae.encoder.conv_in.bias.copy_(0.1 * torch.randn(C, generator=g))
    vae = vae.cuda()
    x = torch.randn(B, 3, H, H, generator=g)
    x[:, :, -1, :] = 20.0 + 5.0 * torch.randn(B, 3, H, generator=g)
    x[:, :, :, -1] = -20.0 + 5.0 * torch.randn(B, 3, H, generator=g)
    xc = x.cuda()
    inp = vae.encode_tap(xc, 0).cpu().double()
    got = vae.encode_tap(xc, 1).cpu().double()
    wd = vae.encoder.down[0].downsample.conv.weight.detach().cpu().to(torch.bfloat16).double()
    bd = vae.encoder.down[0].downsample.conv.bias.detach().cpu().double()
    ref = F.conv2d(F.pad(inp.to(torch.bfloat16).double(), (0, 1, 0, 1)), wd, bd, stride=2)
    return rel_l2(got.numpy(), ref.numpy()), tuple(got.shape)


@pytest.mark.parametrize("C,H,B", [(128, 256, 3), (256, 128, 1), (512, 64, 5)])
def test_downsample_matches_torch_stride2_conv(C, H, B):
    err, shape = downsample_error(C, H, B)
    assert shape == (B, C, H // 2, H // 2)
    assert err < TOL["downsample"], err


# ------------------------------------------------------------------------------------------------------------------ 4
def conv_in_error():
    """conv_in at 256^2 on images whose three channels differ (a smooth field, its negative square, a constant), against
    float64 with the fp32 weights."""
    from uspace_amd.libs.autoencoder import FrozenAutoencoderKL
    torch.manual_seed(5)
    vae = FrozenAutoencoderKL(SD_DDCONFIG, 4, encoder=True).cuda()
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, 256), torch.linspace(-1, 1, 256), indexing="ij")
    x = torch.stack([torch.stack([torch.sin(3 * xx + b) * torch.cos(2 * yy), -(xx * yy + 0.1 * b) ** 2,
                                  torch.full_like(xx, 0.7 - 0.5 * b)]) for b in range(3)])
    got = vae.encode_tap(x.cuda(), 0).cpu().double()
    ref = F.conv2d(x.double(), vae.encoder.conv_in.weight.detach().cpu().double(),
                   vae.encoder.conv_in.bias.detach().cpu().double(), padding=1)
    return rel_l2(got.numpy(), ref.numpy())


def test_conv_in_reads_nchw_rgb():
    assert conv_in_error() < TOL["conv_in"]


# ------------------------------------------------------------------------------------------------------------------ 5
def sample_ulps(seed=21):
    """vae.sample(m) after torch.manual_seed(seed) against the reference formula with torch.randn_like after the same seed,
    on the device in fp32; logvar spans [-60, 60] so the clamp matters.  Returns (max error in ulps of the terms, eps equal)."""
    from uspace_amd.libs.autoencoder import get_model
    vae = get_model(None)                      # decoder-only: sample needs no encoder
    g = torch.Generator().manual_seed(seed)
    m = torch.randn(5, 8, 32, 32, generator=g)
    m[:, 4:] *= 30.0
    m = m.cuda()
    torch.manual_seed(seed)
    got = vae.sample(m)
    torch.manual_seed(seed)
    mean, logvar = torch.chunk(m, 2, dim=1)
    logvar = torch.clamp(logvar, -30.0, 20.0)
    std = torch.exp(0.5 * logvar)
    eps = torch.randn_like(mean)
    ref = vae.scale_factor * (mean + std * eps)
    mag = vae.scale_factor * (mean.abs() + (std * eps).abs())
    ulps = ((got - ref).abs() / (mag * torch.finfo(torch.float32).eps).clamp_min(1e-38)).max()
    return float(ulps), bool(torch.isfinite(got).all())


def test_sample_matches_reference_rng_and_formula():
    ulps, finite = sample_ulps()
    assert finite and ulps <= TOL["sample_ulps"], ulps


# ------------------------------------------------------------------------------------------------------------------ 6
def largest_chunk_diffs():
    """encode_moments of 126 distinct images as one chunk (the 32-bit bound at 256^2) against single-image encodes of
    images 0, 63 and 125."""
    vae = sd_vae_every_parameter_counts()
    assert vae.max_encode_chunk() == 126
    g = torch.Generator().manual_seed(13)
    x = (torch.rand(126, 3, 256, 256, generator=g) * 2 - 1).cuda()
    full = vae.encode_moments(x, chunk=1000)
    out = []
    for i in (0, 63, 125):
        one = vae.encode_moments(x[i:i + 1].contiguous())
        out.append((i, float((full[i] - one[0]).abs().max())))
    return out


def test_sd_encoder_largest_chunk_matches_single_images():
    """Bit-equal: every GEMM form sums K in the same order, GroupNorm chunks a map per image and the attention runs per
    image, so the batch size does not enter any image's arithmetic."""
    for i, d in largest_chunk_diffs():
        assert d == 0.0, (i, d)


# ------------------------------------------------------------------------------------------------------------------ 7
def edit_chain():
    """Real-image edit on tiny nets (dissect_lfm.py:140-199): image -> VAE encode -> CNF.encode -> CNF.decode -> VAE decode."""
    from uspace_amd.flow_matching import CNF
    from uspace_amd.libs.autoencoder import FrozenAutoencoderKL
    from uspace_amd.tools.utils_uvit import get_nnet
    dd = dict(SD_DDCONFIG, ch=64, ch_mult=[1, 2, 2], num_res_blocks=1, resolution=64)
    torch.manual_seed(31)
    vae = FrozenAutoencoderKL(dd, 4, encoder=True).cuda()
    net = get_nnet("uvit", num_classes=-1, img_size=16, patch_size=2, in_chans=4, embed_dim=64, depth=2, num_heads=1,
                   mlp_ratio=4, qkv_bias=False, mlp_time_embed=False)
    net = net.cuda().eval()
    cnf = CNF(net)
    g = torch.Generator().manual_seed(4)
    img = (torch.rand(2, 3, 64, 64, generator=g) * 2 - 1).cuda()
    kw = dict(edit_loc=None, dissect_name="none",
              solver_kwargs=dict(solver="fixed", solver_fix="euler", solver_fix_step=0.1, solver_adaptive="dopri5",
                                 solver_adaptive_prec=0.01))

    def run():
        torch.manual_seed(8)
        z = vae.encode(img)
        noise = cnf.encode(z, None, **kw)
        back = cnf.decode(noise, None, **kw)
        return z, vae.decode(back)
    z1, r1 = run()
    z2, r2 = run()
    return z1, r1, bool(torch.equal(z1, z2) and torch.equal(r1, r2))


def test_real_image_edit_chain_on_tiny_nets():
    z, rec, det = edit_chain()
    assert z.shape == (2, 4, 16, 16) and rec.shape == (2, 3, 64, 64)
    assert bool(torch.isfinite(z).all()) and bool(torch.isfinite(rec).all()) and float(rec.std()) > 1e-4
    assert det
