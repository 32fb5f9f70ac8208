#!/usr/bin/env python3
"""Generate the VAE encoder fixtures under tests/golden/ by IMPORTING the reference (through _refshim.py, as
make_golden.py does for the decoder).  Runs only where the reference is available; the tests read the ``*.npz``.

    python tests/golden/make_vae_encoder_golden.py

  vae_encoder_tiny   libs/autoencoder.py:215-300 Encoder + :412-458 FrozenAutoencoderKL at a tiny configuration
                     (ch=64, ch_mult (1,2,2), 1 res block, 32^2 images -> 8x8 latents: two downsamples; 8x8 is the
                     smallest latent whose 64-token mid attention the GEMM takes, K a multiple of 64): seeded full
                     state_dict (key list, n_params, sha256), 3 images, a tap after every encoder stage and norm_out
                     (every image and pixel, TAP_CHANNELS channels spread evenly over C: random fp32 maps do not compress),
                     moments, a stored eps with sample(moments) drawn by the reference itself, decode(mean * scale)
  vae_encoder_sd     the SD configuration (ch=128, 1-2-4-4, 2 res blocks, 256^2): seeded full state_dict sha256,
                     2 smooth images (fp16-exact values) and the reference's fp32 CPU moments
"""
import hashlib
import json
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _refshim  # noqa: E402

TINY = dict(double_z=True, z_channels=4, resolution=32, in_channels=3, out_ch=3, ch=64, ch_mult=[1, 2, 2],
            num_res_blocks=1, attn_resolutions=[], dropout=0.0)
SD = dict(double_z=True, z_channels=4, resolution=256, in_channels=3, out_ch=3, ch=128, ch_mult=[1, 2, 4, 4],
          num_res_blocks=2, attn_resolutions=[], dropout=0.0)
TINY_SEED, SD_SEED, EPS_SEED = 1234 + 11, 1234 + 13, 99
SCALE = 0.18215
TAP_CHANNELS = 8     # stored channels of a tap: c = 0, C/8, 2C/8, ... (keeps the fixture small)


def reference_model(ae, dd, seed):
    """The reference's FrozenAutoencoderKL with the weights of its construction order under ``seed`` (Encoder,
    Decoder, quant_conv, post_quant_conv): built here in that order, then loaded through its own constructor."""
    torch.manual_seed(seed)
    parts = dict(encoder=ae.Encoder(**dd), decoder=ae.Decoder(**dd),
                 quant_conv=torch.nn.Conv2d(2 * dd["z_channels"], 8, 1), post_quant_conv=torch.nn.Conv2d(4, dd["z_channels"], 1))
    sd = {f"{p}.{k}": v for p, m in parts.items() for k, v in m.state_dict().items()}
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "vae.ckpt")
        torch.save(sd, path)
        model = ae.FrozenAutoencoderKL(dd, 4, path, SCALE)
    return model.eval()


def digest(model):
    sd = model.state_dict()
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(np.ascontiguousarray(v.detach().numpy()).tobytes())
    return list(sd.keys()), int(sum(v.numel() for v in sd.values())), h.hexdigest()


def meta_bytes(meta):
    return np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)


def save(name, **arrays):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **arrays)
    print(f"wrote {name}: {os.path.getsize(path) / 1024:.1f} KiB")


def tap_slice(a, n):
    """Channels 0, C/n, 2C/n, ... of an NCHW map (numpy or torch); the tests slice their maps the same way."""
    return a[:, :: a.shape[1] // n].copy() if isinstance(a, np.ndarray) else a[:, :: a.shape[1] // n].contiguous()


def make_tiny(ae):
    model = reference_model(ae, TINY, TINY_SEED)
    g = torch.Generator().manual_seed(7)
    x = torch.rand(3, 3, 32, 32, generator=g) * 2 - 1
    x[:, 0] = x[:, 0] * 0.5 + 0.4          # distinct channel statistics: an RGB / NCHW mix-up shows
    x[:, 2] = -x[:, 2].abs()
    e = model.encoder
    taps = [("conv_in", e.conv_in), ("down0_b0", e.down[0].block[0]), ("down0_ds", e.down[0].downsample),
            ("down1_b0", e.down[1].block[0]), ("down1_ds", e.down[1].downsample), ("down2_b0", e.down[2].block[0]),
            ("mid1", e.mid.block_1), ("attn", e.mid.attn_1), ("mid2", e.mid.block_2), ("norm_out", e.norm_out)]
    store, hooks = {}, []
    for name, mod in taps:
        hooks.append(mod.register_forward_hook(lambda _m, _a, o, n=name: store.__setitem__(n, o.detach().numpy().copy())))
    with torch.no_grad():
        moments = model(x, "encode_moments")
        for h in hooks:
            h.remove()
        torch.manual_seed(EPS_SEED)
        z = model.sample(moments)
        torch.manual_seed(EPS_SEED)
        eps = torch.randn_like(torch.chunk(moments, 2, dim=1)[0])
        mean = torch.chunk(moments, 2, dim=1)[0]
        rec = model.decode(mean * SCALE)
    keys, n, sha = digest(model)
    meta = dict(ddconfig=TINY, weight_seed=TINY_SEED, eps_seed=EPS_SEED, sha256=sha, keys=keys, n_params=n,
                scale_factor=SCALE, taps=[t for t, _ in taps], tap_channels=TAP_CHANNELS)
    out = {f"tap/{k}": tap_slice(store[k], TAP_CHANNELS) for k, _ in taps}
    out.update(x=x.numpy(), moments=moments.numpy(), eps=eps.numpy(), z=z.numpy(), rec=rec.numpy(), meta_json=meta_bytes(meta))
    save("vae_encoder_tiny.npz", **out)


def smooth_images(n, res, seed):
    """n smooth images in [-1, 1], a different pattern per channel, rounded to fp16-representable values."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, res), torch.linspace(0, 1, res), indexing="ij")
    img = torch.zeros(n, 3, res, res)
    for b in range(n):
        for c in range(3):
            f = torch.randn(4, 4, generator=g)
            v = sum(f[k, 0] * torch.sin((k + 1 + c) * 3.0 * xx + f[k, 1]) * torch.cos((k + 1) * 2.5 * yy + f[k, 2])
                    for k in range(4))
            img[b, c] = 0.8 * torch.tanh(v / 2) + 0.1 * (c - 1)
    return img.to(torch.float16)


def make_sd(ae):
    model = reference_model(ae, SD, SD_SEED)
    x16 = smooth_images(2, 256, 5)
    with torch.no_grad():
        moments = model.encode_moments(x16.to(torch.float32))
    keys, n, sha = digest(model)
    meta = dict(ddconfig=SD, weight_seed=SD_SEED, sha256=sha, n_params=n, n_keys=len(keys), scale_factor=SCALE)
    save("vae_encoder_sd.npz", x_fp16=x16.numpy(), moments=moments.numpy(), meta_json=meta_bytes(meta))


def main():
    _refshim.install()
    import importlib
    ae = importlib.import_module("libs.autoencoder")
    torch.set_grad_enabled(False)
    make_tiny(ae)
    make_sd(ae)


if __name__ == "__main__":
    main()
