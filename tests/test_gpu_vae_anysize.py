"""The VAE at sizes other than the nominal one (FrozenAutoencoderKL takes its size from the tensor, as the reference's Encoder / Decoder
do), and the mid-block attention beyond 1 024 latent positions, where vae.hip launches the streaming kernel of attention_wide.hip.

  tiny model   ch=64, ch_mult (1,2), 1 res block, nominal resolution 64, encoder on, every parameter visible: decode at h = 33 (1 089
               tokens, odd side) and h = 32 and encode_moments at R = 66 and 64, stage by stage -- each stage fed the GPU's own previous
               tap, against the float64 stage reference (oracle/vae_stages.py, tests/vae_encoder_stages.py); which attention a decode
               launched, read from the launch recorder; and the reference's own results at the off-nominal size
               (tests/golden/vae_anysize_tiny.npz, written by tests/golden/make_vae_anysize_golden.py)
  SD shape     mid.attn_1 at 64 x 64 latents against float64, a chunked 512^2 decode against single-image decodes, an encode -> decode
               round trip at 512^2
"""
import json
import os

import numpy as np
import pytest
import torch

from tests.util import rel_l2

pytestmark = pytest.mark.gpu

TINY = dict(double_z=True, z_channels=4, resolution=64, in_channels=3, out_ch=3, ch=64, ch_mult=[1, 2],
            num_res_blocks=1, attn_resolutions=[], dropout=0.0)
QK_GAIN = 2.0
REC_ATTENTION, REC_ATT_WIDE = 1, 4

# rel-L2 of every stage against PURE float64 (no bf16 rounding in the reference), 3 x what an MI355X measured -- the larger of the two
# sizes per stage, listed above each row.  Stage 0 is fp32 arithmetic; the others round their GEMM operands to bf16.
STAGE_TOL = dict(
    # decode: conv_in, mid.block_1, mid.attn_1, mid.block_2, up.1.block.0, up.1.block.1, up.1.upsample, up.0.block.0, up.0.block.1
    # measured h = 33:  1.24e-7  9.06e-4  5.61e-4  8.88e-4  8.40e-4  8.53e-4  2.27e-3  2.81e-3  1.76e-3
    # measured h = 32:  1.24e-7  8.98e-4  5.46e-4  8.79e-4  8.28e-4  8.41e-4  2.27e-3  2.81e-3  1.75e-3
    decode=[3.8e-7, 2.8e-3, 1.7e-3, 2.7e-3, 2.6e-3, 2.6e-3, 6.9e-3, 8.5e-3, 5.3e-3],
    # encode: conv_in, down.0.block.0, down.0.downsample, down.1.block.0, mid.block_1, mid.attn_1, mid.block_2
    # measured R = 66:  9.56e-8  2.68e-3  2.43e-3  3.14e-3  2.13e-3  1.24e-3  1.77e-3
    # measured R = 64:  9.54e-8  2.68e-3  2.43e-3  3.11e-3  2.12e-3  1.22e-3  1.77e-3
    encode=[2.9e-7, 8.1e-3, 7.3e-3, 9.5e-3, 6.4e-3, 3.8e-3, 5.4e-3],
    # SD shape, decoder mid.attn_1 at 64 x 64 latents (4 096 tokens, C = 512), B = 1: measured 4.14e-4 (peak probability 0.70);
    # tests/test_gpu_vae.py measures 4.4e-4 for the same stage at 32 x 32 on the three-launch path
    sd_attn=1.25e-3,
)
# The off-nominal golden comparison measured rel 5.2e-3 / max 5.8e-3 (decode) and 7.4e-3 / 8.4e-3 (moments); the 512^2 round trip of the
# seeded SD weights gives a PSNR of 11.1 dB (seeded weights reconstruct nothing; recorded, not gated).
# tests/test_gpu_vae.py::test_tiny_decoder_matches_reference_golden's tolerances (rel-L2, max |err| / max |ref|)
GOLDEN_TOL = (1.5e-2, 4e-2)


def _cpu_threads():
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 16))
    return n


def tiny_vae_every_parameter_counts(seed=1234):
    """The tiny autoencoder, seeded, with every parameter visible (as tests/test_gpu_vae.py::sd_vae_every_parameter_counts): GroupNorm
    gamma ~ N(1, 0.2), beta ~ N(0, 0.3), conv biases ~ N(0, 0.05), q / k weights of both mid blocks scaled by QK_GAIN."""
    from uspace_amd.libs.autoencoder import FrozenAutoencoderKL
    torch.manual_seed(seed)
    vae = FrozenAutoencoderKL(TINY, 4, encoder=True)
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
        for half in (vae.decoder, vae.encoder):
            for n in ("q", "k"):
                getattr(half.mid.attn_1, n).weight.mul_(QK_GAIN)
    return vae.cuda()


_TINY = {}


def tiny_vae():
    if "vae" not in _TINY:
        _TINY["vae"] = tiny_vae_every_parameter_counts()
        _TINY["sd"] = {k: v.detach().cpu() for k, v in _TINY["vae"].state_dict().items()}
    return _TINY["vae"], _TINY["sd"]


def tiny_latents(B, h, seed=7):
    g = torch.Generator().manual_seed(seed + h)
    return torch.randn(B, 4, h, h, generator=g) * 0.18215 * 4.0


def tiny_images(B, R, seed=3):
    g = torch.Generator().manual_seed(seed + R)
    x = torch.rand(B, 3, R, R, generator=g) * 2 - 1
    x[:, 0] = x[:, 0] * 0.5 + 0.4
    x[:, 2] = -x[:, 2].abs()
    return x


def stage_errors(tap, run_stage, spec, sd, x0):
    """Per stage k: the GPU's tap k against the float64 stage k on the GPU's tap k - 1 -> [(shape ok, rel-L2)]."""
    n = _cpu_threads()
    try:
        out, prev = [], x0
        for k, (_, _, H, Cc) in enumerate(spec.stages):
            got = tap(k).cpu()
            ok = tuple(got.shape) == (x0.shape[0], Cc, H, H)
            out.append((ok, rel_l2(got.numpy(), run_stage(spec, sd, k, prev, bf16=False).numpy()) if ok else float("inf")))
            prev = got
        return out
    finally:
        torch.set_num_threads(n)


def wide_launches(fn):
    """The attention records of the launch recorder around fn(): (wide launches, other attention launches, the wide records)."""
    from uspace_amd import _hip
    torch.cuda.synchronize()
    _hip.prof_all_begin()
    fn()
    torch.cuda.synchronize()
    recs = [r for r in _hip.prof_all_end() if r["kind"] == REC_ATTENTION]
    wide = [r for r in recs if r["flags"] & REC_ATT_WIDE]
    return sum(r["launches"] for r in wide), sum(r["launches"] for r in recs if not r["flags"] & REC_ATT_WIDE), wide


# ------------------------------------------------------------------------------------------------------------------ tiny model
@pytest.mark.parametrize("h", [33, 32])
def test_tiny_decode_stage_parity_at_any_size(h):
    from oracle import vae_stages as S
    vae, sd = tiny_vae()
    spec = S.Spec.from_ddconfig(dict(TINY, resolution=2 * h))
    assert len(spec.stages) == len(STAGE_TOL["decode"])
    z = tiny_latents(2, h)
    zc = z.cuda()
    errs = stage_errors(lambda k: vae.decode_tap(zc, k), S.run_stage, spec, sd, z)
    print(f"\n[tiny decode h={h}] " + " ".join(f"{e:.2e}" for _, e in errs) + f" peak_p={S.attn_peak(spec, sd, vae.decode_tap(zc, 1).cpu()):.3f}")
    img = vae.decode(zc)
    assert img.shape == (2, 3, 2 * h, 2 * h) and bool(torch.isfinite(img).all())
    assert vae.resolution == 64 and vae.z_res == 32                       # the nominal size stays what ddconfig says
    assert list(vae._ws)[-1][0] == ((2, 66) if h == 33 else 2)            # workspace key: (chunk, resolution) off the nominal size
    for k, (ok, e) in enumerate(errs):
        assert ok and e < STAGE_TOL["decode"][k], (k, ok, e)


@pytest.mark.parametrize("R", [66, 64])
def test_tiny_encode_stage_parity_at_any_size(R):
    from tests import vae_encoder_stages as E
    vae, sd = tiny_vae()
    spec = E.EncSpec.from_ddconfig(dict(TINY, resolution=R))
    assert len(spec.stages) == len(STAGE_TOL["encode"]) and spec.z_res == R // 2
    x = tiny_images(2, R)
    xc = x.cuda()
    errs = stage_errors(lambda k: vae.encode_tap(xc, k), E.run_stage, spec, sd, x)
    print(f"\n[tiny encode R={R}] " + " ".join(f"{e:.2e}" for _, e in errs))
    m = vae.encode_moments(xc)
    assert m.shape == (2, 8, R // 2, R // 2) and bool(torch.isfinite(m).all())
    assert vae.encode(xc).shape == (2, 4, R // 2, R // 2)
    for k, (ok, e) in enumerate(errs):
        assert ok and e < STAGE_TOL["encode"][k], (k, ok, e)


def test_recorder_shows_the_wide_kernel_beyond_1024_tokens_only():
    """Flag bit 4 of an attention record marks uspace_attention_wide_bf16 (M = images of the chunk, N = tokens, K = C): exactly one per
    decode and per encode at 33 x 33 latents, none at 32 x 32, where the three-launch path runs as before."""
    vae, _ = tiny_vae()
    z33, z32 = tiny_latents(3, 33).cuda(), tiny_latents(3, 32).cuda()
    n_wide, n_other, recs = wide_launches(lambda: vae.decode(z33))
    assert (n_wide, n_other) == (1, 0) and [(r["M"], r["N"], r["K"]) for r in recs] == [(3, 1089, 128)], recs
    n_wide, n_other, recs = wide_launches(lambda: vae.decode(z33, chunk=2))           # 2 + 1: one launch per chunk
    assert (n_wide, n_other) == (2, 0) and sorted(r["M"] for r in recs) == [1, 2], recs
    assert wide_launches(lambda: vae.decode(z32))[:2] == (0, 0)
    n_wide, n_other, recs = wide_launches(lambda: vae.encode_moments(tiny_images(3, 66).cuda()))
    assert (n_wide, n_other) == (1, 0) and [(r["M"], r["N"], r["K"]) for r in recs] == [(3, 1089, 128)], recs
    assert wide_launches(lambda: vae.encode_moments(tiny_images(3, 64).cuda()))[:2] == (0, 0)


def test_bad_shapes_are_refused_by_name():
    vae, _ = tiny_vae()
    for bad in (torch.zeros(1, 4, 33, 32), torch.zeros(1, 3, 33, 33), torch.zeros(4, 33, 33), torch.zeros(1, 4, 0, 0)):
        with pytest.raises(ValueError, match="square"):
            vae.decode(bad.cuda())
        with pytest.raises(ValueError, match="square"):
            vae.decode_tap(bad.cuda(), 0)
    for bad in (torch.zeros(1, 3, 66, 64), torch.zeros(1, 4, 66, 66), torch.zeros(1, 3, 67, 67), torch.zeros(1, 3, 0, 0)):
        for fn in (vae.encode_moments, vae.encode, lambda x: vae.encode_tap(x, 0)):
            with pytest.raises(ValueError, match="multiple of 2"):
                fn(bad.cuda())
    assert vae.decode(torch.zeros(0, 4, 33, 33).cuda()).shape == (0, 3, 66, 66)
    assert vae.decode(torch.zeros(1, 4, 1, 1).cuda()).shape == (1, 3, 2, 2)
    assert vae.encode_moments(torch.zeros(1, 3, 2, 2).cuda()).shape == (1, 8, 1, 1)


def test_tiny_model_matches_reference_golden_off_nominal(golden_dir):
    """The reference's own decode of [2,4,33,33] and encode_moments of [2,3,66,66] with a model built at nominal resolution 64: the same
    seeded weights here, at the tolerances of the nominal-size golden test."""
    from uspace_amd.libs.autoencoder import FrozenAutoencoderKL
    f = np.load(os.path.join(golden_dir, "vae_anysize_tiny.npz"))
    meta = json.loads(bytes(f["meta_json"]).decode())
    assert meta["ddconfig"]["resolution"] == 64 and f["z_fp16"].shape == (2, 4, 33, 33) and f["x_fp16"].shape == (2, 3, 66, 66)
    assert os.path.getsize(os.path.join(golden_dir, "vae_anysize_tiny.npz")) < 200 * 1024
    torch.manual_seed(meta["weight_seed"])
    vae = FrozenAutoencoderKL(meta["ddconfig"], 4, encoder=True).cuda()
    assert sum(p.numel() for p in vae.parameters()) == meta["n_params"]
    for name, got, ref in (("decode", vae.decode(torch.from_numpy(f["z_fp16"]).float().cuda()), f["img_fp16"]),
                           ("moments", vae.encode_moments(torch.from_numpy(f["x_fp16"]).float().cuda()), f["moments_fp16"])):
        got, ref = got.cpu().numpy(), ref.astype(np.float32)
        assert got.shape == ref.shape
        r, m = rel_l2(got, ref), float(np.abs(got - ref).max() / np.abs(ref).max())
        print(f"\n[anysize golden {name}] rel={r:.3e} max={m:.3e}")
        assert r < GOLDEN_TOL[0] and m < GOLDEN_TOL[1], (name, r, m)


# ------------------------------------------------------------------------------------------------------------------ SD shape
def sd_latents(B, h, seed=7):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 4, h, h, generator=g) * 0.18215 * 4.0


def test_sd_mid_attention_at_64x64_latents_against_fp64():
    """decode_tap(z, 2) -- mid.attn_1 over 4 096 tokens of 512 channels, one wide launch -- against the float64 stage on the GPU's tap 1."""
    from oracle import vae_stages as S
    from tests.test_gpu_vae import SD_DDCONFIG, sd_vae_every_parameter_counts
    vae = sd_vae_every_parameter_counts()
    sd = {k: v.detach().cpu() for k, v in vae.state_dict().items()}
    spec = S.Spec.from_ddconfig(dict(SD_DDCONFIG, resolution=512))
    z = sd_latents(1, 64).cuda()
    t1 = vae.decode_tap(z, 1).cpu()
    n_wide, n_other, recs = wide_launches(lambda: _TINY.__setitem__("t2", vae.decode_tap(z, 2)))
    t2 = _TINY.pop("t2").cpu()
    assert (n_wide, n_other) == (1, 0) and [(r["M"], r["N"], r["K"]) for r in recs] == [(1, 4096, 512)], recs
    assert t2.shape == (1, 512, 64, 64)
    n = _cpu_threads()
    try:
        err = rel_l2(t2.numpy(), S.run_stage(spec, sd, 2, t1, bf16=False).numpy())
        peak = S.attn_peak(spec, sd, t1)
    finally:
        torch.set_num_threads(n)
    print(f"\n[sd attn 64x64] rel={err:.3e} peak_p={peak:.3f}")
    assert peak > 0.3
    assert err < STAGE_TOL["sd_attn"], err


def test_sd_512_decode_chunks_are_bit_equal_and_round_trip_runs():
    """One 512^2 decode of B = 3 with chunk = 2 (2 + 1): finite, and each image bit-equal to its single-image decode (the wide kernel's
    rows depend on neither B nor the grid, like every other kernel of the walk).  Then encode -> decode at 512^2: it runs; the PSNR
    against the input is printed, not gated (seeded weights reconstruct nothing)."""
    from tests.test_gpu_vae_encoder import sd_vae_every_parameter_counts
    vae = sd_vae_every_parameter_counts()
    z = sd_latents(3, 64, seed=11).cuda()
    img = vae.decode(z, chunk=2)
    assert img.shape == (3, 3, 512, 512) and bool(torch.isfinite(img).all()) and float(img.std()) > 1e-4
    for b in range(3):
        assert torch.equal(vae.decode(z[b:b + 1].contiguous())[0], img[b]), b
    yy, xx = torch.meshgrid(torch.linspace(0, 1, 512), torch.linspace(0, 1, 512), indexing="ij")
    x = torch.stack([torch.stack([0.8 * torch.sin((3 + c + b) * 3.0 * xx + c) * torch.cos((2 + b) * 2.5 * yy) for c in range(3)])
                     for b in range(2)]).cuda()
    zz = vae.encode(x)
    assert zz.shape == (2, 4, 64, 64) and bool(torch.isfinite(zz).all())
    rec = vae.decode(zz)
    assert rec.shape == x.shape and bool(torch.isfinite(rec).all())
    mse = float(((rec - x) ** 2).mean())
    print(f"\n[sd 512 round trip] PSNR = {10 * np.log10(4.0 / mse):.2f} dB (seeded weights; recorded, not gated)")
