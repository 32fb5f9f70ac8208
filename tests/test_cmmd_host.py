"""Host-side checks of uspace_amd/tools/cmmd.py without a GPU: the 336-pixel preset, the argument errors, the bank round trip and
the path API.  Where a test needs the kernel's sums it swaps ``_hip.metric_rbf_sums`` for the float64 reference of
tests/cmmd_cases.py; the kernel itself is checked in tests/test_gpu_cmmd.py."""
import math

import numpy as np
import pytest
import torch

from tests import cmmd_cases as C
from tests.clip_vision_cases import TINY_VISION
from uspace_amd.libs.clip import CLIP_L_336_VISION, CLIP_L_VISION, CLIPVisionTransformer
from uspace_amd.tools import cmmd as M
from uspace_amd.tools.feature_metrics import FeatureBank


@pytest.fixture
def on_host(monkeypatch):
    """``rbf_mmd2`` on CPU tensors: the device check dropped, the sums from the float64 reference; records the calls."""
    calls = []

    def sums(x, y, gamma, normalize=False, ws=None):
        calls.append((tuple(x.shape), tuple(y.shape), gamma, normalize))
        s, _, _ = C.ref_sums(x.numpy(), y.numpy(), math.sqrt(1.0 / (2.0 * gamma)), normalize)
        return torch.from_numpy(s)

    monkeypatch.setattr(M._hip, "metric_rbf_sums", sums)
    monkeypatch.setattr(M, "_device_features", lambda t, name: t.detach().to(torch.float32).contiguous())
    return calls


def _sets(case=C.CASES[3]):
    x, y = C.sets_of(case)
    return torch.from_numpy(np.array(x)), torch.from_numpy(np.array(y))


def test_the_336_preset_has_577_tokens():
    assert CLIP_L_336_VISION == dict(CLIP_L_VISION, image_size=336) and CLIP_L_VISION["image_size"] == 224
    cfg = dict(CLIP_L_336_VISION, num_hidden_layers=1)              # the token count does not depend on the depth
    assert CLIPVisionTransformer(**cfg).tokens == 577
    assert (CLIP_L_336_VISION["image_size"] // CLIP_L_336_VISION["patch_size"]) ** 2 + 1 == 577
    assert CLIP_L_336_VISION["projection_dim"] == 768 and CLIP_L_336_VISION["num_hidden_layers"] == 24


def test_scores_are_the_definition(on_host):
    x, y = _sets()
    ref = C.ref_of(C.CASES[3], 1)
    assert M.cmmd_score(y, x) == pytest.approx(ref["score"], abs=ref["bound"])         # the V-statistic is symmetric in its sets
    assert on_host[-1] == ((130, 67), (17, 67), 1.0 / 200.0, True)
    assert M.rbf_mmd2(x, y, C.SIGMA) * 1000.0 == pytest.approx(ref["score"], abs=ref["bound"])
    u = C.ref_of(C.CASES[3], 0, True)
    assert M.rbf_mmd2(x, y, C.SIGMA, normalize=False, unbiased=True) * 1000.0 == pytest.approx(u["score"], abs=u["bound"])
    assert on_host[-1][3] is False
    assert M.rbf_mmd2(FeatureBank.from_features(x), FeatureBank.from_features(y), C.SIGMA) * 1000.0 == pytest.approx(ref["score"], abs=ref["bound"])
    assert M.mmd2_from_sums([2.0, 6.0, 3.0], 2, 3) == (2.0 + 2) / 4 + (6.0 + 3) / 9 - 2 * 3.0 / 6
    assert M.mmd2_from_sums([2.0, 6.0, 3.0], 2, 3, unbiased=True) == 2.0 / 2 + 6.0 / 6 - 2 * 3.0 / 6


def test_value_errors(on_host):
    x, y = _sets()
    with pytest.raises(ValueError, match="widths differ"):
        M.rbf_mmd2(x, y[:, :60], 10.0)
    with pytest.raises(ValueError, match="at least one row"):
        M.rbf_mmd2(x[:0], y, 10.0)
    with pytest.raises(ValueError, match="at least one row"):
        M.cmmd_score(x, FeatureBank.from_features(y[:0]))
    for sigma in (0.0, -1.0, math.inf, math.nan):
        with pytest.raises(ValueError, match="sigma"):
            M.rbf_mmd2(x, y, sigma)
        with pytest.raises(ValueError, match="sigma"):
            M.cmmd_score(x, y, sigma=sigma)
    with pytest.raises(ValueError, match="two rows"):
        M.rbf_mmd2(x[:1], y, 10.0, unbiased=True)
    with pytest.raises(ValueError, match="two rows"):
        M.rbf_mmd2(x, y[:1], 10.0, unbiased=True)
    with pytest.raises(ValueError):
        M.rbf_mmd2(x[0], y, 10.0)                                   # not [n, F]
    assert on_host == []                                            # every one of them was refused before the kernel call
    assert math.isfinite(M.rbf_mmd2(x[:1], y, 10.0))                # one row is enough for the V-statistic


def test_cmmd_object_errors_and_bank_round_trip(on_host, tmp_path):
    vision = CLIPVisionTransformer(**TINY_VISION)
    m = M.CMMD(vision, device="cpu", chunk=5)
    assert m.dims == TINY_VISION["projection_dim"] and m.chunk == 5 and len(m.fake) == 0 and len(m.real) == 0
    with pytest.raises(ValueError, match="both sets"):
        m.compute()
    g = torch.Generator().manual_seed(3)
    fake, real = torch.randn(7, m.dims, generator=g), torch.randn(9, m.dims, generator=g) + 0.1
    m.update_features(fake)
    with pytest.raises(ValueError, match="both sets"):
        m.compute()                                                 # no real embeddings yet
    with pytest.raises(ValueError):
        m.update_features(torch.zeros(2, m.dims + 1))               # width mismatch
    m.update_features(real[:4], real=True)
    m.update_features(real[4:], real=True)
    assert len(m.fake) == 7 and len(m.real) == 9
    score = m.compute()
    assert score == M.cmmd_score(fake, real) and on_host[-1] == ((7, m.dims), (9, m.dims), 1.0 / 200.0, True)
    path = str(tmp_path / "real.npz")
    m.save(path)
    with np.load(path) as f:
        assert f["features"].dtype == np.float32 and np.array_equal(f["features"], real.numpy())
    m.reset()
    assert len(m.fake) == 0 and len(m.real) == 0
    m.load(path)
    m.update_features(fake)
    assert m.compute() == score
    m.reset(real=False)
    assert len(m.fake) == 0 and len(m.real) == 9
    other = M.CMMD(CLIPVisionTransformer(**dict(TINY_VISION, projection_dim=32)), device="cpu")
    with pytest.raises(ValueError, match="width"):
        other.load(path)
    with pytest.raises(Exception):
        m.update(torch.zeros(1, 3, 64, 64))                         # images on the host: there is no CPU path


def test_given_paths_accepts_banks_in_either_position(on_host, tmp_path):
    x, y = _sets()
    px, py = str(tmp_path / "x.npz"), str(tmp_path / "y.npz")
    FeatureBank.from_features(x).save(px)
    FeatureBank.from_features(y).save(py)
    ref = C.ref_of(C.CASES[3], 1)
    a = M.calculate_cmmd_given_paths((px, py), None, device="cpu")
    b = M.calculate_cmmd_given_paths((py, px), None, device="cpu")
    assert a == pytest.approx(ref["score"], abs=ref["bound"]) and b == pytest.approx(ref["score"], abs=ref["bound"])
    assert on_host[0][:2] == ((130, 67), (17, 67)) and on_host[1][:2] == ((17, 67), (130, 67))      # paths[0] real, paths[1] generated
    with pytest.raises(RuntimeError, match="Invalid path"):
        M.calculate_cmmd_given_paths((px, str(tmp_path / "missing")), None, device="cpu")
    (tmp_path / "folder").mkdir()
    with pytest.raises(ValueError, match="vision tower"):
        M.calculate_cmmd_given_paths((px, str(tmp_path / "folder")), None, device="cpu")


def test_exports_and_defaults():
    import inspect
    for name in ("CMMD", "rbf_mmd2", "cmmd_score", "calculate_cmmd_given_paths"):
        assert name in M.__all__ and callable(getattr(M, name))
    sig = inspect.signature(M.cmmd_score).parameters
    assert sig["sigma"].default == 10.0 and sig["scale"].default == 1000.0
    sig = inspect.signature(M.rbf_mmd2).parameters
    assert sig["normalize"].default is True and sig["unbiased"].default is False
    sig = inspect.signature(M.CMMD.from_pretrained).parameters
    assert sig["version"].default == "openai/clip-vit-large-patch14-336"
    sig = inspect.signature(M.calculate_cmmd_given_paths).parameters
    assert list(sig)[:4] == ["paths", "vision", "device", "batch_size"] and sig["batch_size"].default == 50
