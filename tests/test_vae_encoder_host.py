"""VAE encoder without a GPU: the module surface of FrozenAutoencoderKL(encoder=True) against the reference's seeded
weights (libs/autoencoder.py:412-476), checkpoint and get_model rules, the C-ABI's parameter table, and the float64
stage reference of tests/vae_encoder_stages.py against the reference's taps."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from tests.util import rel_l2

SD_DDCONFIG = dict(double_z=True, z_channels=4, resolution=256, in_channels=3, out_ch=3, ch=128,
                   ch_mult=[1, 2, 4, 4], num_res_blocks=2, attn_resolutions=[], dropout=0.0)


def _fixture(golden_dir, name):
    z = np.load(os.path.join(golden_dir, name))
    return z, json.loads(bytes(z["meta_json"]).decode())


def _sha(sd):
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(np.ascontiguousarray(v.numpy()).tobytes())
    return h.hexdigest()


def test_full_model_keys_and_seeded_init_match_reference(golden_dir):
    from uspace_amd.libs.autoencoder import FrozenAutoencoderKL
    z, meta = _fixture(golden_dir, "vae_encoder_tiny.npz")
    torch.manual_seed(meta["weight_seed"])
    vae = FrozenAutoencoderKL(meta["ddconfig"], 4, encoder=True)
    sd = vae.state_dict()
    assert list(sd.keys()) == meta["keys"] and sum(v.numel() for v in sd.values()) == meta["n_params"]
    assert _sha(sd) == meta["sha256"]
    assert not vae.training and not any(p.requires_grad for p in vae.parameters())


def test_sd_full_model_seeded_init_matches_reference(golden_dir):
    from uspace_amd.libs.autoencoder import FrozenAutoencoderKL
    _, meta = _fixture(golden_dir, "vae_encoder_sd.npz")
    torch.manual_seed(meta["weight_seed"])
    vae = FrozenAutoencoderKL(meta["ddconfig"], 4, encoder=True)
    sd = vae.state_dict()
    assert len(sd) == meta["n_keys"] and sum(v.numel() for v in sd.values()) == meta["n_params"] == 83653863
    enc = sum(p.numel() for p in vae.encoder.parameters())
    assert enc == 34163592 and sum(p.numel() for p in vae.quant_conv.parameters()) == 72
    assert _sha(sd) == meta["sha256"]


def test_full_model_loads_strictly(golden_dir):
    from uspace_amd.libs.autoencoder import FrozenAutoencoderKL
    _, meta = _fixture(golden_dir, "vae_encoder_tiny.npz")
    vae = FrozenAutoencoderKL(meta["ddconfig"], 4, encoder=True)
    sd = {k: v.clone() + 1.0 for k, v in vae.state_dict().items()}
    vae.load_state_dict(sd)
    assert torch.equal(vae.encoder.conv_in.weight, sd["encoder.conv_in.weight"])
    assert torch.equal(vae.quant_conv.bias, sd["quant_conv.bias"])
    with pytest.raises(RuntimeError):
        vae.load_state_dict({k: v for k, v in sd.items() if k != "encoder.conv_out.bias"})
    with pytest.raises(RuntimeError):
        vae.load_state_dict({k: v for k, v in sd.items() if k != "quant_conv.weight"})
    with pytest.raises(RuntimeError):
        vae.load_state_dict(dict(sd, **{"encoder.extra.weight": torch.zeros(1)}))


def test_get_model_includes_the_encoder_iff_the_checkpoint_has_one(monkeypatch):
    from uspace_amd.libs import autoencoder as ae
    base = ae.get_model(None)
    assert not base.has_encoder and not hasattr(base, "encoder") and not hasattr(base, "quant_conv")
    assert sum(p.numel() for p in base.parameters()) == 49490199
    assert list(base.state_dict().keys())[0] == "decoder.conv_in.weight"
    full = ae.get_model(None, encoder=True)
    assert full.has_encoder and sum(p.numel() for p in full.parameters()) == 83653863
    keys = list(full.state_dict().keys())
    assert keys[0] == "encoder.conv_in.weight" and keys[-4:] == ["quant_conv.weight", "quant_conv.bias",
                                                                 "post_quant_conv.weight", "post_quant_conv.bias"]
    full_sd = full.state_dict()
    dec_sd = base.state_dict()
    for sd, want in ((full_sd, True), (dec_sd, False)):
        monkeypatch.setattr(torch, "load", lambda *a, _sd=sd, **k: _sd)
        m = ae.get_model("checkpoint.ckpt")
        assert m.has_encoder == want
        assert torch.equal(m.decoder.conv_in.weight, sd["decoder.conv_in.weight"])
    monkeypatch.setattr(torch, "load", lambda *a, **k: full_sd)
    assert not ae.get_model("checkpoint.ckpt", encoder=False).has_encoder     # explicit choice wins; encoder half ignored


def test_encoder_config_queries_without_gpu():
    from uspace_amd import _hip
    from uspace_amd.libs.autoencoder import FrozenAutoencoderKL
    L = _hip.lib()
    mult = (ctypes.c_int * 4)(1, 2, 4, 4)
    cfg = ctypes.byref(_hip.VaeConfig(128, mult, 4, 2, 256))
    n = L.uspace_vae_enc_num_params(cfg)
    assert n == 108
    numel = [L.uspace_vae_enc_param_numel(cfg, i) for i in range(n)]
    assert sum(numel) == 34163664
    vae = FrozenAutoencoderKL(SD_DDCONFIG, 4, encoder=True)
    ps = list(vae.encoder.parameters()) + list(vae.quant_conv.parameters())
    assert numel == [p.numel() for p in ps]
    assert L.uspace_vae_enc_param_numel(cfg, n) < 0
    assert L.uspace_vae_enc_weight_bytes(cfg) >= 34163664 * 2
    assert L.uspace_vae_enc_workspace_bytes(cfg, 8) > 2 * 8 * 258 * 258 * 128 * 4
    assert vae.max_encode_chunk() == 126 and 126 * 258 * 258 * 128 < 2 ** 30 <= 127 * 258 * 258 * 128
    bad = ctypes.byref(_hip.VaeConfig(192, mult, 4, 2, 256))            # ch not a power of two
    assert L.uspace_vae_enc_num_params(bad) < 0 and L.uspace_vae_enc_weight_bytes(bad) == 0
    assert L.uspace_vae_enc_workspace_bytes(cfg, 0) == 0
    # decoder queries unchanged
    assert L.uspace_vae_num_params(cfg) == 140


def test_forward_dispatch_and_errors(golden_dir):
    from uspace_amd import _hip
    from uspace_amd.libs.autoencoder import FrozenAutoencoderKL
    _, meta = _fixture(golden_dir, "vae_encoder_tiny.npz")
    dd = meta["ddconfig"]
    dec_only = FrozenAutoencoderKL(dd, 4)
    x = torch.zeros(1, 3, 32, 32)
    for fn in ("encode", "encode_moments"):
        with pytest.raises(NotImplementedError):
            dec_only(x, fn)
    with pytest.raises(NotImplementedError):
        dec_only.encode_moments(x)
    with pytest.raises(_hip.UspaceHipError):
        dec_only.sample(torch.zeros(1, 8, 8, 8))                       # sample needs no encoder, but a device tensor
    vae = FrozenAutoencoderKL(dd, 4, encoder=True)
    for fn in ("encode", "encode_moments", "decode"):
        with pytest.raises(_hip.UspaceHipError):                          # host tensors: no CPU path
            vae(x if fn != "decode" else torch.zeros(1, 4, 8, 8), fn)
    with pytest.raises(_hip.UspaceHipError):
        vae.sample(torch.zeros(1, 8, 8, 8))
    with pytest.raises(NotImplementedError):
        vae(x, "reconstruct")
    for bad in (dict(dd, double_z=False), dict(dd, in_channels=4), dict(dd, resamp_with_conv=False),
                dict(dd, attn_resolutions=[16])):
        with pytest.raises(NotImplementedError):
            FrozenAutoencoderKL(bad, 4, encoder=True)


def test_fp64_encoder_stage_reference_matches_reference_taps(golden_dir):
    """tests/vae_encoder_stages.py (the GPU tests' yardstick) against the reference's own taps and moments."""
    from tests import vae_encoder_stages as E
    from uspace_amd.libs.autoencoder import FrozenAutoencoderKL
    z, meta = _fixture(golden_dir, "vae_encoder_tiny.npz")
    torch.manual_seed(meta["weight_seed"])
    vae = FrozenAutoencoderKL(meta["ddconfig"], 4, encoder=True)
    sd = vae.state_dict()
    spec = E.EncSpec.from_ddconfig(meta["ddconfig"])
    assert [(h, c) for _, _, h, c in spec.stages] == [(32, 64), (32, 64), (16, 64), (16, 128), (8, 128), (8, 128),
                                                       (8, 128), (8, 128), (8, 128)]
    names = ["conv_in", "down0_b0", "down0_ds", "down1_b0", "down1_ds", "down2_b0", "mid1", "attn", "mid2"]
    taps = {}
    m = E.encode_moments(spec, sd, z["x"], taps=taps)
    nc = meta["tap_channels"]                 # the fixture keeps channels 0, C/nc, 2C/nc, ... of every tap
    for k, n in enumerate(names):
        assert rel_l2(taps[k][:, :: taps[k].shape[1] // nc].numpy(), z[f"tap/{n}"]) < 1e-5, (k, n)
    nt = taps["norm_out"]
    assert rel_l2(nt[:, :: nt.shape[1] // nc].numpy(), z["tap/norm_out"]) < 1e-5
    assert rel_l2(m.numpy(), z["moments"]) < 1e-5
    # bf16 mode rounds where the HIP path does: close to the reference, but not equal
    mb = E.encode_moments(spec, sd, z["x"], bf16=True)
    assert 1e-5 < rel_l2(mb.numpy(), z["moments"]) < 2e-2
    # sample(): the stored eps is what torch.randn_like drew after manual_seed, and the formula gives the reference's z
    torch.manual_seed(meta["eps_seed"])
    mom = torch.from_numpy(z["moments"])
    eps = torch.randn_like(torch.chunk(mom, 2, dim=1)[0])
    assert torch.equal(eps, torch.from_numpy(z["eps"]))
    assert torch.equal(E.sample(mom, eps, meta["scale_factor"]), torch.from_numpy(z["z"]))
