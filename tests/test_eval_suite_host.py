"""Host side of the Inception Score / sFID / EvalSuite tools (no GPU): the head's state_dict rules, the split rule and the
ValueErrors, the statistics files' keys, the ABI surface of the new entry points, their argument checks, and the resources
of the new kernels."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from uspace_amd.tools import inception

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("uspace_inception_forward_suite", "uspace_inception_logits", "uspace_inception_score_workspace_bytes",
         "uspace_inception_score_f64")
KERNELS = ("gather_channels_kernel", "logits_kernel", "is_lse_kernel", "is_colsum_kernel", "is_marginal_kernel", "is_kl_kernel",
           "is_score_kernel")


# ------------------------------------------------------------------------------------------- the head
def _full_state_dict(classes=1008):
    sd = dict(inception.InceptionV3(seed=3).state_dict())
    for k in list(sd):
        if k.endswith(".bn.running_var"):
            sd[k.replace("running_var", "num_batches_tracked")] = torch.tensor(0)
    g = torch.Generator().manual_seed(8)
    sd["fc.weight"] = torch.randn(classes, 2048, generator=g)
    sd["fc.bias"] = torch.randn(classes, generator=g)
    return sd


def test_head_loads_fc_from_a_full_state_dict(tmp_path):
    sd = _full_state_dict()
    p = str(tmp_path / "w.pth")
    torch.save(sd, p)
    head = inception.InceptionHead(weights=p)
    own = head.state_dict()
    assert list(own) == ["fc.weight", "fc.bias"] and head.num_classes == 1008
    assert torch.equal(own["fc.weight"], sd["fc.weight"]) and torch.equal(own["fc.bias"], sd["fc.bias"])
    assert not any(q.requires_grad for q in head.parameters())
    # the same file still loads into the feature extractor, whose state_dict holds no fc.*
    m = inception.InceptionV3(weights=p)
    assert not any(k.startswith("fc.") for k in m.state_dict()) and len(m.state_dict()) == 94 * 5
    # the class count follows the weight
    head.load_state_dict(_full_state_dict(classes=1000))
    assert head.num_classes == 1000 and tuple(head.fc.bias.shape) == (1000,)


def test_head_without_fc_weight_raises_and_names_the_key(tmp_path):
    sd = _full_state_dict()
    del sd["fc.weight"]
    with pytest.raises(KeyError) as e:
        inception.InceptionHead(seed=0).load_state_dict(sd)
    assert "fc.weight" in str(e.value)
    p = str(tmp_path / "w.pth")
    torch.save(sd, p)
    with pytest.raises(KeyError) as e:
        inception.InceptionHead(weights=p)
    assert "fc.weight" in str(e.value)
    sd = _full_state_dict()
    sd["fc.bias"] = torch.zeros(7)
    with pytest.raises(ValueError):
        inception.InceptionHead(seed=0).load_state_dict(sd)


def test_head_missing_weights_raise_without_download(tmp_path, monkeypatch):
    monkeypatch.setattr(torch.hub, "get_dir", lambda: str(tmp_path))

    def no_network(*a, **k):
        raise AssertionError("network access attempted")
    monkeypatch.setattr(torch.hub, "load_state_dict_from_url", no_network)
    monkeypatch.setattr(torch.hub, "download_url_to_file", no_network)
    with pytest.raises(FileNotFoundError) as e:
        inception.InceptionHead()
    msg = str(e.value)
    assert os.path.join(str(tmp_path), "checkpoints") in msg and inception.FID_WEIGHTS_FILE in msg


def test_seeded_head_is_reproducible_and_fails_loudly_on_cpu():
    from uspace_amd._hip import UspaceHipError
    a, b = inception.InceptionHead(num_classes=40, seed=5, std=0.1), inception.InceptionHead(num_classes=40, seed=5, std=0.1)
    assert tuple(a.fc.weight.shape) == (40, 2048) and torch.equal(a.fc.weight, b.fc.weight) and torch.equal(a.fc.bias, b.fc.bias)
    assert abs(float(a.fc.weight.std()) - 0.1) < 0.01 and abs(float(a.fc.bias.std()) - 0.5) < 0.2
    with pytest.raises(UspaceHipError):
        a.logits(torch.zeros(2, 2048))
    with pytest.raises(UspaceHipError):
        inception.InceptionV3(seed=0).suite(torch.rand(1, 3, 32, 32))


# ------------------------------------------------------------------------------------------- the score's host logic
def test_split_rule_and_value_errors():
    from uspace_amd._hip import UspaceHipError
    from uspace_amd.tools.inception_score import InceptionScore, inception_score, split_bounds
    from tests import eval_suite_cases as EC
    for (N, _C, splits) in EC.IS_CASES + [(10, 2, 3)]:
        assert split_bounds(N, splits) == EC.split_bounds(N, splits)
    assert split_bounds(10, 3) == [(0, 3), (3, 6), (6, 10)]
    x = torch.zeros(9, 5)
    for splits in (10, 0, -1, 2.5):
        with pytest.raises(ValueError):
            inception_score(x, splits=splits)
    with pytest.raises(ValueError):
        inception_score(torch.zeros(9), splits=1)
    with pytest.raises(UspaceHipError):                     # valid arguments reach the device check: there is no CPU path
        inception_score(x, splits=3)
    acc = InceptionScore(device="cpu", model=object(), head=object())
    assert len(acc) == 0
    with pytest.raises(ValueError):
        acc.compute(splits=1)                               # nothing added yet
    with pytest.raises(ValueError):
        acc.update_features(torch.zeros(3, 100))
    with pytest.raises(UspaceHipError):
        acc.update_logits(torch.zeros(3, 5))


def test_is_path_function_mirrors_the_fid_signature():
    import inspect
    from uspace_amd.tools.fid_score import calculate_fid_given_paths
    from uspace_amd.tools.inception_score import calculate_is_given_path
    from uspace_amd.tools.sfid_score import calculate_sfid_given_paths
    fid = inspect.signature(calculate_fid_given_paths).parameters
    for fn in (calculate_is_given_path, calculate_sfid_given_paths):
        got = inspect.signature(fn).parameters
        for n in ("device", "batch_size", "num_workers", "model"):
            assert got[n].default == fid[n].default, (fn.__name__, n)
    assert inspect.signature(calculate_is_given_path).parameters["splits"].default == 10
    with pytest.raises(RuntimeError):
        calculate_is_given_path("/nonexistent/a", device="cpu")
    with pytest.raises(RuntimeError):
        calculate_sfid_given_paths(("/nonexistent/a", "/nonexistent/b"), device="cpu")


# ------------------------------------------------------------------------------------------- statistics files
def _spd(n, seed):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((n, n))
    return rng.standard_normal(n), a @ a.T / n + np.eye(n)


def test_npz_keys_mu_sigma_against_mu_s_sigma_s(tmp_path):
    from uspace_amd.tools import fid_score, sfid_score
    from uspace_amd.tools.eval_suite import EvalSuite
    (m1, s1), (m2, s2), (m3, s3), (m4, s4) = (_spd(6, i) for i in range(4))
    pool_only, spatial_only, both = (str(tmp_path / n) for n in ("pool.npz", "spatial.npz", "both.npz"))
    np.savez(pool_only, mu=m1, sigma=s1)
    np.savez(spatial_only, mu_s=m2, sigma_s=s2)
    np.savez(both, mu=m3, sigma=s3, mu_s=m4, sigma_s=s4)
    # sFID reads mu_s / sigma_s and never mu / sigma
    want = fid_score.calculate_frechet_distance(m2, s2, m4, s4)
    assert sfid_score.calculate_sfid_given_paths((spatial_only, both), device="cpu") == want
    with pytest.raises(KeyError) as e:
        sfid_score.calculate_sfid_given_paths((pool_only, both), device="cpu")
    assert "mu_s" in str(e.value) and "pool.npz" in str(e.value)
    # FID reads mu / sigma of the same files
    assert fid_score.calculate_fid_given_paths((pool_only, both), device="cpu", model=object()) == \
        fid_score.calculate_frechet_distance(m1, s1, m3, s3)
    with pytest.raises(KeyError):
        sfid_score.load_statistics(spatial_only, "fid")
    assert sorted(EvalSuite.load(both)) == ["mu", "mu_s", "sigma", "sigma_s"] and sorted(EvalSuite.load(pool_only)) == ["mu", "sigma"]
    assert sfid_score.spatial_dims() == 2023 and sfid_score.spatial_dims(15, 768) == 17 * 17 * 768
    for bad in ((0, 7), (19, 7), (14, 0), (14, 769)):
        with pytest.raises(ValueError):
            sfid_score.spatial_dims(*bad)


def test_spatial_statistics_interface_and_save_keys(tmp_path):
    """SpatialFIDStatistics is FIDStatistics with dims 2023; finalisation and the saved keys need no kernel."""
    from uspace_amd.tools.fid_score import FIDStatistics
    from uspace_amd.tools.sfid_score import SpatialFIDStatistics
    st = SpatialFIDStatistics(device="cpu", model=object())
    assert isinstance(st, FIDStatistics) and st.dims == 2023 and st.n == 0
    for name in ("update", "update_features", "reset", "save", "mu", "sigma", "model"):
        assert hasattr(SpatialFIDStatistics, name), name
    with pytest.raises(ValueError):
        st.mu
    assert SpatialFIDStatistics(device="cpu", spatial_channels=3).dims == 17 * 17 * 3
    rng = np.random.default_rng(0)
    x = rng.standard_normal((40, 2023))
    st.n, st.shift = 40, torch.zeros(2023, dtype=torch.float64)
    st.s1, st.s2 = torch.from_numpy(x.sum(0)), torch.from_numpy(x.T @ x)
    p = str(tmp_path / "s.npz")
    st.save(p)
    with np.load(p) as f:
        assert sorted(f.keys()) == ["mu_s", "sigma_s"] and f["sigma_s"].shape == (2023, 2023)
        assert np.allclose(f["mu_s"], x.mean(0), atol=1e-12) and np.allclose(f["sigma_s"], np.cov(x, rowvar=False), atol=1e-10)


# ------------------------------------------------------------------------------------------- ABI
def test_every_new_export_is_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "uspace_hip.h")).read()
    declared = set(re.findall(r"USPACE_API\s+[\w\s\*]+?\b(uspace_\w+)\s*\(", hdr))
    from uspace_amd import _hip
    lib = ctypes.CDLL(os.path.join(ROOT, "uspace_amd", "libuspace_hip.so"))
    for name in NAMES:
        assert name in declared and name in _hip.SIGNATURES and hasattr(lib, name), name
    assert declared == set(_hip.SIGNATURES)
    assert _hip.lib().uspace_abi_version() == _hip.ABI_VERSION
    for fn in ("inception_logits", "inception_score_splits"):
        assert callable(getattr(_hip, fn))
    mk = open(os.path.join(ROOT, "uspace_amd", "csrc", "Makefile")).read()
    assert "inception_score.hip" in mk


def test_score_workspace_bytes_without_gpu():
    """The layout is the library's own business: the size is positive for valid arguments, grows with N, C and splits, and is
    0 for invalid ones."""
    from uspace_amd import _hip
    wb = _hip.lib().uspace_inception_score_workspace_bytes
    for good in ((1000, 1008, 7), (50000, 1008, 10), (50000, 1008, 1), (10, 1, 10), (1, 1, 1)):
        assert wb(*good) >= 8 * (good[0] + good[2] * good[1]), good          # at least a double per row and per (split, class)
    assert wb(1000, 1008, 7) < wb(2000, 1008, 7) and wb(1000, 40, 7) < wb(1000, 1008, 7) and wb(1000, 1008, 1) < wb(1000, 1008, 7)
    for bad in ((9, 5, 10), (10, 5, 0), (10, 0, 1), (0, 5, 1), ((1 << 24) + 1, 5, 1), (1 << 24, 5, 1), (10, 65537, 1)):
        assert wb(*bad) == 0, bad


def test_argument_errors_need_no_gpu():
    """The entry points validate before they launch: USPACE_ERR_ARG (-1) and USPACE_ERR_WORKSPACE (-3) come back without a device."""
    from uspace_amd import _hip
    L = _hip.lib()
    p = ctypes.c_void_p(64)                  # never dereferenced: every call below is refused first
    assert L.uspace_inception_logits(p, p, None, p, 2, 24, 5, None) == -1          # K % 16
    assert L.uspace_inception_logits(p, p, None, p, 2, 0, 5, None) == -1
    assert L.uspace_inception_logits(p, p, None, p, 0, 16, 5, None) == -1
    assert L.uspace_inception_logits(p, p, None, p, 2, 16, 0, None) == -1
    assert L.uspace_inception_logits(p, None, None, p, 2, 16, 5, None) == -1
    assert L.uspace_inception_logits(ctypes.c_void_p(68), p, None, p, 2, 16, 5, None) == -1      # 16-byte loads
    assert L.uspace_inception_score_f64(p, 9, 5, 10, p, 1 << 20, p, None) == -1    # N < splits
    assert L.uspace_inception_score_f64(p, 9, 5, 0, p, 1 << 20, p, None) == -1
    assert L.uspace_inception_score_f64(p, 9, 5, 3, p, 1 << 20, None, None) == -1
    assert L.uspace_inception_score_f64(p, 9, 5, 3, p, L.uspace_inception_score_workspace_bytes(9, 5, 3) - 1, p, None) == -3
    suite = lambda stage, ch, pool=p: L.uspace_inception_forward_suite(p, p, 1 << 20, p, 1, 8, 8, pool, p, stage, ch, None)
    assert suite(0, 7) == -1 and suite(19, 7) == -1 and suite(14, 0) == -1 and suite(14, 769) == -1 and suite(8, 257) == -1
    assert suite(14, 7, pool=None) == -1
    assert suite(14, 7) == -3                                                      # valid arguments: the workspace is too small
    # the library's channel count of every stage is the Python side's: all of a stage's channels pass, one more does not
    for stage in range(1, 19):
        c = inception.STAGE_SHAPES[stage][2]
        assert suite(stage, c) == -3 and suite(stage, c + 1) == -1, stage


def test_new_kernels_use_no_scratch_and_no_lds():
    import importlib.util
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    ks = kr.kernels()
    names = dict(zip([k["name"] for k in ks], kr.demangle([k["name"] for k in ks])))
    found = set()
    for k in ks:
        for s in KERNELS:
            if s in names[k["name"]]:
                found.add(s)
                assert k["scratch"] == 0, names[k["name"]]
                assert k["lds"] == 0, names[k["name"]]                 # none of them declares LDS: nothing to overrun
                assert k["vgpr"] + k["agpr"] <= 128, names[k["name"]]
    assert found == set(KERNELS), sorted(set(KERNELS) - found)
