"""Every size the library reports for the packed weight blobs and the workspaces of every model, against
tests/golden/blob_sizes.json (recorded by tests/golden/make_blob_golden.py at the commit named in the file): exact integers, no
margin.  Host queries only; the library loads without a GPU."""
import ctypes
import json
import os

import pytest

from tests import blob_cases as C


@pytest.fixture(scope="module")
def golden(golden_dir):
    return json.load(open(os.path.join(golden_dir, "blob_sizes.json")))["sizes"]


def test_sizes_equal_the_recorded_ones(golden_dir, golden):
    got = C.size_table(golden_dir)
    assert sorted(got) == sorted(golden)
    for name in golden:
        for field in ("num_params", "param_numel", "weight_bytes", "workspace_bytes"):
            assert got[name][field] == golden[name][field], (name, field)
    # the switch of the GEMM's K-split tail is back at its default, and it moved a recorded size (so both settings were taken)
    from uspace_amd import _hip
    assert _hip.lib().uspace_gemm_get_sk() == 1
    assert golden["uvit/L_u/sk1"]["workspace_bytes"] != golden["uvit/L_u/sk0"]["workspace_bytes"]


def test_param_numel_rejects_indices_outside_the_parameters(golden_dir):
    from uspace_amd import _hip
    L = _hip.lib()
    for name, (prefix, cfg, _ws) in C.size_cases(golden_dir).items():
        lead = C.lead_args(cfg)
        numel = getattr(L, prefix + "param_numel")
        n = getattr(L, prefix + "num_params")(*lead)
        assert n > 0 and numel(*lead, -1) < 0 and numel(*lead, n) < 0, name       # U-ViT: n is its first derived entry
        assert numel(*lead, n - 1) > 0, name


def test_invalid_configs_report_no_parameters_and_no_bytes():
    from uspace_amd import _hip
    L = _hip.lib()
    mult = (ctypes.c_int * 4)(1, 2, 4, 4)
    bad = [("uspace_uvit_", _hip.UvitConfig(32, 2, 4, 1000, 20, 16, 4096, 0, 0, 0)),       # embed_dim not a multiple of 64
           ("uspace_uvit_", _hip.UvitConfig(32, 2, 4, 1024, 19, 16, 4096, 0, 0, 0)),       # odd depth
           ("uspace_vae_", _hip.VaeConfig(100, mult, 4, 2, 256)),                           # ch not a multiple of 64
           ("uspace_vae_enc_", _hip.VaeConfig(192, mult, 4, 2, 256)),                       # encoder: ch not a power of two
           ("uspace_clip_", _hip.ClipConfig(49408, 768, 8, 12, 3072, 77, 1e-5)),           # head_dim != 64
           ("uspace_clipv_", _hip.ClipVisionConfig(224, 14, 1024, 12, 24, 4096, 768, 1e-5)),   # heads * 64 != dim
           ("uspace_idnet_", C.idnet_cfg(40, (1, 1, 1, 1), 1)),                             # input_size not a multiple of 16
           ("uspace_dino_", _hip.DinoConfig(224, 14, 1024, 12, 24, 4096, 1, 1e-6)),        # heads * 64 != dim
           ("uspace_lpips_", 2)]                                                            # neither of the two nets (by value)
    for prefix, cfg in bad:
        ref, = C.lead_args(cfg)
        size = (64, 64) if prefix == "uspace_lpips_" else ()       # its workspace depends on the image size too
        assert getattr(L, prefix + "num_params")(ref) < 0 and getattr(L, prefix + "param_numel")(ref, 0) < 0, prefix
        assert getattr(L, prefix + "weight_bytes")(ref) == 0 and getattr(L, prefix + "workspace_bytes")(ref, 8, *size) == 0, prefix
