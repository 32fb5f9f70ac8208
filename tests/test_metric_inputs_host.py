"""The host plumbing the metric tools share (uspace_amd/tools/_inputs.py) and the accumulators built over arbitrary features
(``FIDStatistics.of_width`` / ``FeatureBank.of_width``): no GPU."""
import numpy as np
import pytest
import torch

from uspace_amd.tools import _inputs


def _save_image_rounding(x):
    return x.mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8).float() / 255


def test_quantize_is_save_images_rounding_and_the_identity_on_decoded_bytes():
    q = torch.arange(256, dtype=torch.float32)
    x = torch.cat([torch.tensor([0.0, 1.0, -0.25, -1e-9, 1.0 + 1e-6, 1.5, 0.3, 0.999999]), q / 255, (q + 0.5) / 255])
    keep = x.clone()
    got = _inputs.quantize(x)
    assert got.dtype == torch.float32 and torch.equal(got.view(torch.int32), _save_image_rounding(x).view(torch.int32))
    assert torch.equal(x.view(torch.int32), keep.view(torch.int32))                      # the argument is left as it was
    # decoded bytes come back as the bytes they were, all 256 levels, whether the level is the division q / 255 or the product
    # with fl(1 / 255) a device computes: fl(255 level) + 0.5 floors to q
    levels, by_reciprocal = q / 255, q * torch.tensor(1 / 255, dtype=torch.float32)
    for lv in (levels, by_reciprocal):
        assert torch.equal((lv * 255 + 0.5).floor(), q)
        assert torch.equal(_inputs.quantize(lv).view(torch.int32), levels.view(torch.int32))
        assert torch.equal((_inputs.quantize(lv) * 255).round(), q)
    # the plain product does not: it gives q for every division here, and misses q by an ulp for some of the reciprocal levels
    assert torch.equal(levels * 255, q)
    assert not torch.equal(by_reciprocal * 255, q) and float((by_reciprocal * 255 - q).abs().max()) <= 2.0 ** -16
    # values outside [0, 1] clamp to the ends
    assert _inputs.quantize(torch.tensor([-3.0, 7.0])).tolist() == [0.0, 1.0]


def _folder(tmp_path, names, size=(4, 5)):
    from PIL import Image
    tmp_path.mkdir(parents=True, exist_ok=True)
    for i, nm in enumerate(names):
        Image.fromarray(np.full((size[0], size[1], 3), i * 30, np.uint8)).save(tmp_path / nm)
    return tmp_path


def test_image_files_sorts_the_concatenated_globs(tmp_path):
    _folder(tmp_path, ["10.png", "2.png", "1.jpg", "a.webp"])
    (tmp_path / "skip.txt").write_text("x")
    assert [f.name for f in _inputs.image_files(tmp_path)] == ["1.jpg", "10.png", "2.png", "a.webp"]
    assert _inputs.image_files(str(tmp_path)) == _inputs.image_files(tmp_path) and _inputs.image_files(tmp_path / "none") == []


def test_uint8_batches_keep_order_and_leave_the_last_batch_ragged(tmp_path):
    _folder(tmp_path, [f"{i}.png" for i in range(7)])
    files = _inputs.image_files(tmp_path)
    batches = list(_inputs.uint8_batches(files, 3))
    assert [tuple(b.shape) for b in batches] == [(3, 3, 4, 5), (3, 3, 4, 5), (1, 3, 4, 5)]
    assert all(b.dtype == torch.uint8 and not b.is_cuda for b in batches)
    assert [int(v) for v in torch.cat(batches)[:, 0, 0, 0]] == [i * 30 for i in range(7)]       # file i holds the value 30 i
    assert list(_inputs.uint8_batches([], 3)) == []


def test_paired_image_files_and_their_three_errors(tmp_path):
    a, b = _folder(tmp_path / "a", ["y.png", "x.png"], (16, 16)), _folder(tmp_path / "b", ["x.jpg", "y.png"], (16, 16))
    names, fa, fb = _inputs.paired_image_files(a, b)
    assert names == ["x", "y"] and [f.name for f in fa] == ["x.png", "y.png"] and [f.name for f in fb] == ["x.jpg", "y.png"]
    with pytest.raises(ValueError, match="do not pair up by file name"):
        _inputs.paired_image_files(a, _folder(tmp_path / "c", ["x.png", "z.png"], (16, 16)))
    with pytest.raises(ValueError, match="sizes differ"):
        _inputs.paired_image_files(a, _folder(tmp_path / "d", ["x.png", "y.png"], (24, 24)))
    for d in ("e", "f"):                                                                 # equal partners, unlike the first pair
        _folder(tmp_path / d, ["x.png"], (16, 16))
        _folder(tmp_path / d, ["y.png"], (24, 24))
    with pytest.raises(ValueError, match="sizes differ at 'y'"):
        _inputs.paired_image_files(tmp_path / "e", tmp_path / "f")
    with pytest.raises(ValueError, match="no images"):
        _inputs.paired_image_files(tmp_path / "none", tmp_path / "none")


def test_require_paths_and_rocm_device(tmp_path):
    from uspace_amd._hip import UspaceHipError
    _inputs.require_paths([tmp_path, str(tmp_path)])
    with pytest.raises(RuntimeError, match="Invalid path"):
        _inputs.require_paths([tmp_path, tmp_path / "missing"])
    assert _inputs.rocm_device("cpu", "x") == torch.device("cpu")
    assert _inputs.rocm_device(torch.device("cpu"), "x") == torch.device("cpu")
    if not torch.cuda.is_available():
        with pytest.raises(UspaceHipError, match="the thing needs a ROCm device"):
            _inputs.rocm_device(None, "the thing")


def test_accumulators_of_any_width_go_through_the_constructor():
    from uspace_amd.tools.feature_metrics import FeatureBank
    from uspace_amd.tools.fid_score import FIDStatistics
    st = FIDStatistics.of_width(1024, "cpu")
    assert type(st) is FIDStatistics and st.dims == 1024 and st.n == 0 and st.device == torch.device("cpu")
    with pytest.raises(ValueError, match="at least two samples"):
        st.mu
    bank = FeatureBank.of_width(768, "cpu")
    assert type(bank) is FeatureBank and bank.dims == 768 and bank.n == 0 and len(bank) == 0
    assert tuple(bank.features.shape) == (0, 768)
    for acc in (st, bank):
        with pytest.raises(ValueError, match="has no model: use update_features"):
            acc.update(torch.zeros(1, 3, 8, 8))
        with pytest.raises(ValueError, match="has no model: use update_features"):
            acc.model
    assert FeatureBank.from_features(torch.ones(4, 768)).dims == 768
    # the constructors keep their check
    for cls in (FIDStatistics, FeatureBank):
        with pytest.raises(ValueError, match="dims must be one of"):
            cls(dims=100, device="cpu")
        assert cls(dims=768, device="cpu", model=object()).block == 2


def test_vision_tower_from_an_hf_clip_model():
    """``CLIPVisionTransformer.from_hf``, the one builder behind ``CLIPScore.from_pretrained`` and ``CMMD.from_pretrained``, on a
    stand-in with an HF ``CLIPModel``'s ``config`` and ``state_dict()`` (text entries included: the tower drops them)."""
    from types import SimpleNamespace
    from tests import clip_vision_cases as V
    from uspace_amd.libs.clip import CLIPVisionTransformer
    cfg = dict(V.TINY_VISION, hidden_act="quick_gelu")
    proj = cfg.pop("projection_dim")
    sd = dict(V.vision_params("workflow", seed=3, **V.TINY_VISION), logit_scale=torch.zeros(()))
    sd["text_model.final_layer_norm.weight"] = torch.ones(128)
    hf = SimpleNamespace(config=SimpleNamespace(vision_config=SimpleNamespace(**cfg), projection_dim=proj), state_dict=lambda: sd)
    tower = CLIPVisionTransformer.from_hf(hf)
    assert tower.cfg == dict(image=56, patch=14, dim=128, heads=2, layers=2, ffn=512, proj_dim=64, eps=1e-5) and tower.tokens == 17
    got = tower.state_dict()
    assert len(got) == len(sd) - 2 and all(torch.equal(v, sd[k]) for k, v in got.items())
