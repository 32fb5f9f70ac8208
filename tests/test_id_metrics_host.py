"""CPU-only checks of the ArcFace identity tower and the ID similarity: the module's state dict against the published layout, the
library's parameter table, the loader's errors, the ABI rows, the conditioning of the seeded weights on the float64 restatement of
tests/arcface_stages.py, every planted fault against the bounds the GPU tests use, and ``PairMetrics`` left as it was."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import arcface_stages as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["uspace_idnet_num_params", "uspace_idnet_param_numel", "uspace_idnet_weight_bytes", "uspace_idnet_workspace_bytes",
               "uspace_idnet_pack_weights", "uspace_idnet_preprocess", "uspace_idnet_forward", "uspace_idnet_tap",
               "uspace_idnet_unit_workspace_bytes", "uspace_idnet_unit", "uspace_idnet_similarity_f64"]


@pytest.fixture(scope="module")
def ir_se50():
    from uspace_amd.libs.arcface import Backbone
    m = Backbone(seed=0)
    return m, m.state_dict()


@pytest.fixture(scope="module")
def tiny():
    from uspace_amd.libs.arcface import Backbone
    m = Backbone(input_size=32, blocks=R.TINY, seed=5)
    return m, m.state_dict()


@pytest.fixture(scope="module")
def units():
    from uspace_amd.libs.arcface import Backbone
    m = Backbone(input_size=32, blocks=R.UNIT_BLOCKS, seed=6)
    return m, m.state_dict()


# ------------------------------------------------------------------------------------------------- module and state dict
def test_ir_se50_state_dict_is_the_published_layout(ir_se50):
    from uspace_amd import _hip
    m, sd = ir_se50
    tensors = [k for k in sd if not k.endswith("num_batches_tracked")]
    assert len(sd) == 397 and len(tensors) == 343 and sum(p.numel() for p in m.parameters()) == 43_797_696
    assert len([k for k in sd if k.startswith("body.") and k.split(".")[1].isdigit()]) and max(int(k.split(".")[1]) for k in sd if k.startswith("body.")) == 23
    shapes = {k: tuple(v.shape) for k, v in sd.items()}
    assert shapes["input_layer.0.weight"] == (64, 3, 3, 3) and shapes["input_layer.2.weight"] == (64,)
    assert shapes["body.0.res_layer.1.weight"] == (64, 64, 3, 3) and "body.0.shortcut_layer.0.weight" not in shapes
    assert shapes["body.3.shortcut_layer.0.weight"] == (128, 64, 1, 1) and shapes["body.3.shortcut_layer.1.running_var"] == (128,)
    assert shapes["body.3.res_layer.0.weight"] == (64,) and shapes["body.3.res_layer.3.weight"] == (128, 128, 3, 3)
    assert shapes["body.3.res_layer.5.fc1.weight"] == (8, 128, 1, 1) and shapes["body.3.res_layer.5.fc2.weight"] == (128, 8, 1, 1)
    assert shapes["body.23.res_layer.4.num_batches_tracked"] == ()
    assert shapes["output_layer.0.weight"] == (512,) and shapes["output_layer.3.weight"] == (512, 512 * 7 * 7)
    assert shapes["output_layer.3.bias"] == (512,) and shapes["output_layer.4.running_mean"] == (512,)
    # the library's parameter table is the state dict without num_batches_tracked, in order
    L = _hip.lib()
    r = ctypes.byref(m.cfg)
    assert L.uspace_idnet_num_params(r) == 343
    assert [L.uspace_idnet_param_numel(r, i) for i in range(343)] == [sd[k].numel() for k in tensors]
    assert L.uspace_idnet_weight_bytes(r) >= 4 * (43_797_696 - 54 * 2 * 512)      # batch norms are folded or stored as two vectors
    assert 0 < L.uspace_idnet_workspace_bytes(r, 1) < L.uspace_idnet_workspace_bytes(r, 4)
    assert not m.training and not m.train().training


@pytest.mark.parametrize("num_layers,mode,units_,keys", [(100, "ir_se", 49, None), (152, "ir_se", 50, None), (50, "ir", 24, 343 - 48)])
def test_variants(num_layers, mode, units_, keys):
    from uspace_amd import _hip
    from uspace_amd.libs.arcface import BLOCKS, Backbone, unit_specs
    m = Backbone(input_size=32, num_layers=num_layers, mode=mode)       # a small head: the walk is what is checked
    sd = m.state_dict()
    assert len(m.body) == units_ == len(unit_specs(BLOCKS[num_layers]))
    assert ("body.0.res_layer.5.fc1.weight" in sd) == (mode == "ir_se")
    tensors = [k for k in sd if not k.endswith("num_batches_tracked")]
    if keys is not None:
        assert len(tensors) == keys
    L = _hip.lib()
    r = ctypes.byref(m.cfg)
    assert L.uspace_idnet_num_params(r) == len(tensors)
    assert [L.uspace_idnet_param_numel(r, i) for i in range(len(tensors))] == [sd[k].numel() for k in tensors]


def test_refused_configurations():
    from uspace_amd.libs.arcface import Backbone
    for kw in (dict(num_layers=34), dict(mode="se_ir"), dict(affine=False), dict(input_size=100), dict(input_size=0)):
        with pytest.raises(NotImplementedError):
            Backbone(**kw)


def test_loader_is_strict_and_never_downloads(tiny, tmp_path):
    from uspace_amd import _hip
    from uspace_amd.libs.arcface import Backbone
    m, sd = tiny
    with pytest.raises(FileNotFoundError, match="never downloads"):
        Backbone(input_size=32, blocks=R.TINY, weights=str(tmp_path / "absent.pth"))
    path = tmp_path / "tiny.pth"
    torch.save(sd, path)
    again = Backbone(input_size=32, blocks=R.TINY, weights=str(path))
    assert all(torch.equal(v, again.state_dict()[k]) for k, v in sd.items())
    empty = Backbone(input_size=32, blocks=R.TINY)
    assert "weights=" in empty._missing
    for bad in ({k: v for k, v in sd.items() if k != "body.1.res_layer.2.weight"}, dict(sd, extra=torch.zeros(1)),
                dict(sd, **{"output_layer.3.bias": torch.zeros(511)})):
        with pytest.raises(RuntimeError):
            empty.load_state_dict(bad)
        assert empty._missing
    empty.load_state_dict(sd)
    assert empty._missing is None
    with pytest.raises(_hip.UspaceHipError):       # there is no CPU path
        m(torch.zeros(1, 3, 32, 32))


# ------------------------------------------------------------------------------------------------------------------- ABI
def test_abi_rows():
    from uspace_amd import _hip
    hdr = open(os.path.join(ROOT, "include", "uspace_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    declared = set(re.findall(r"USPACE_API\s+[\w\s\*]+?\b(uspace_\w+)\s*\(", hdr))
    L = _hip.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _hip.SIGNATURES and hasattr(L, name), name
    assert {n for n in declared if n.startswith("uspace_idnet_")} == set(NEW_SYMBOLS)
    for name in ("uspace_idnet_forward", "uspace_idnet_preprocess", "uspace_idnet_similarity_f64", "uspace_idnet_config"):
        assert name in doc, name
    assert declared == set(_hip.SIGNATURES)
    assert "#define USPACE_ABI_VERSION 11" in hdr and L.uspace_abi_version() == _hip.ABI_VERSION == 11
    assert len(_hip.SIGNATURES["uspace_idnet_preprocess"][1]) == 9 and len(_hip.SIGNATURES["uspace_idnet_forward"][1]) == 8
    assert len(_hip.SIGNATURES["uspace_idnet_tap"][1]) == 9 and len(_hip.SIGNATURES["uspace_idnet_similarity_f64"][1]) == 5
    fields = re.search(r"struct uspace_idnet_config \{(.*?)\};", hdr, re.S).group(1)
    assert re.findall(r"int\s+(\w+)(?:\[4\])?;", fields) == [f for f, _ in _hip.IdnetConfig._fields_] == ["input_size", "blocks", "se"]
    assert ctypes.sizeof(_hip.IdnetConfig) == 24
    # the generated stub lists the `typedef struct {` configs only and is still what the generator prints
    import importlib.util
    spec = importlib.util.spec_from_file_location("abi_stub", os.path.join(ROOT, "tools", "abi_stub.py"))
    abi = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(abi)
    block = doc[doc.index(abi.BEGIN) + len(abi.BEGIN):doc.index(abi.END)]
    assert block.split("```python", 1)[1].rsplit("```", 1)[0].strip() == abi.stub().strip()


def test_python_stage_shapes_match_the_restatement(tiny):
    from uspace_amd.libs.arcface import stage_shapes, unit_specs
    _, sd = tiny
    assert unit_specs(R.UNIT_BLOCKS) == R.unit_specs(R.UNIT_BLOCKS)
    x = torch.zeros(1, 3, 32, 32, dtype=torch.float64)
    for s, (h, w, c) in enumerate(stage_shapes(32, R.TINY)):
        x = R.stage(sd, R.TINY, True, s, x)
        assert tuple(x.shape) == (1, c, h, w)
    assert tuple(R.stage(sd, R.TINY, True, 5, x).shape) == (1, 512)


def test_adaptive_pool_restatement_is_torchs():
    x = torch.rand(2, 3, 188, 188, dtype=torch.float64)
    assert torch.allclose(R.adaptive_pool(x, 112), torch.nn.functional.adaptive_avg_pool2d(x, 112), rtol=0, atol=1e-14)
    y = torch.rand(1, 3, 300, 300, dtype=torch.float64)
    assert torch.allclose(R.adaptive_pool(y, 256), torch.nn.functional.adaptive_avg_pool2d(y, 256), rtol=0, atol=1e-14)
    widths = {int((row > 0).sum()) for row in R._pool_matrix(188, 112)}
    assert widths == {2, 3}


def test_restatement_is_torchs_own_modules(tiny):
    """The restatement against the module's own torch layers run eagerly in float64 (they only hold tensors for the kernels, but
    they are the published layers in the published nesting)."""
    m, sd = tiny
    import copy
    ref = copy.deepcopy(m).double()
    x = (R.smooth_images(2, 32, 32, 3) * 2 - 1).double()
    y = ref.input_layer(x)
    for u in ref.body:
        r = u.res_layer[:5](y)
        se = u.res_layer[5]
        r = r * se.sigmoid(se.fc2(se.relu(se.fc1(se.avg_pool(r)))))
        y = r + u.shortcut_layer(y)
    y = ref.output_layer(y)
    want = y / y.norm(dim=1, keepdim=True)
    assert float(R.rel_l2(R.embed(sd, R.TINY, True, x), want).max()) < 1e-12


# ---------------------------------------------------------------------------------------------------------- conditioning
def test_seeded_weights_are_well_conditioned(ir_se50):
    m, sd = ir_se50
    a = R.smooth_images(3, 256, 256, 11)
    e = lambda t: R.embed(sd, m.blocks, True, R.preprocess(t, True, True, 112))
    ea = e(a)
    cos = {amp: (ea * e(R.perturbed(a, amp, 12))).sum(1) for amp in (0.001, 0.1, 1.0)}
    assert bool((cos[0.001] > cos[0.1]).all()) and bool((cos[0.1] > cos[1.0]).all())
    assert float(cos[0.001].min()) > 0.9999 and float(cos[1.0].max()) < 0.95
    unrelated = (ea @ ea.T)[~torch.eye(3, dtype=torch.bool)]
    assert float(unrelated.max()) < 0.9


# ------------------------------------------------------------------------------------------------------ bounds and faults
def _unit_deviation(sd, fault, index, size, B=2):
    cin, depth, stride = R.unit_specs(R.UNIT_BLOCKS)[index]
    x = R.unit_input(B, size[0], size[1], cin, 31 + index).double()
    true = R.unit(sd, f"body.{index}", x, cin, depth, stride, True)
    return R.rel_l2_split(R.unit(sd, f"body.{index}", x, cin, depth, stride, True, (fault,)), true)


def test_every_bound_separates_every_planted_fault(tiny, units):
    """A condition on the bounds, not a measurement: each bound of TOL lies at least 10 x below the smallest deviation (over the
    samples of the cases meant to expose it) of every fault that bound is to catch."""
    (tm, tsd), (_, usd) = tiny, units
    seen = {}

    def note(bound, fault, dev):
        dev = float(torch.as_tensor(dev).min())
        seen.setdefault(bound, []).append((fault, dev))
        print(f"ID-FAULT {bound} {fault}: {dev:.3e}")
        assert R.TOL[bound] * 10 <= dev, (bound, fault, dev)

    # the preprocess: the crop and the window rule, on the ragged and the integer windows
    for B, H, W, crop in R.PREPROCESS_CASES:
        x = R.smooth_images(B, H, W, 21)
        true = R.preprocess(x, True, crop, 112)
        note("preprocess", "pool_floor_windows", R.rel_l2(R.preprocess(x, True, crop, 112, ("pool_floor_windows",)), true))
        if crop:
            note("preprocess", "crop_shifted", R.rel_l2(R.preprocess(x, True, crop, 112, ("crop_shifted",)), true))
    # single units: the border ring judges the padding, the interior the rest
    for index, size in R.UNIT_CASES:
        note("unit_border", "bn_through_padding", _unit_deviation(usd, "bn_through_padding", index, size)[1])
        for fault in ("prelu_as_relu", "no_se"):
            inner, border = _unit_deviation(usd, fault, index, size)
            note("unit_border", fault, border)
            if inner.any():      # the map has an interior
                note("unit_interior", fault, inner)
        if size[0] * size[1] > 4 or R.unit_specs(R.UNIT_BLOCKS)[index][2] == 1:      # more than one output pixel
            note("unit_border", "se_mean_over_window", _unit_deviation(usd, "se_mean_over_window", index, size)[1])
    inner, border = _unit_deviation(usd, "shortcut_offset", 0, (8, 8))
    note("unit_interior", "shortcut_offset", inner)
    note("unit_border", "shortcut_offset", border)
    # the input layer, the head and the whole tower on the tiny configuration
    x = (R.smooth_images(3, 32, 32, 41) * 2 - 1).double()
    s0 = R.stage(tsd, R.TINY, True, 0, x)
    note("input_layer", "prelu_as_relu", R.rel_l2(R.stage(tsd, R.TINY, True, 0, x, ("prelu_as_relu",)), s0))
    s4 = x
    for s in range(5):
        s4 = R.stage(tsd, R.TINY, True, s, s4)
    h = R.head(tsd, s4)
    note("head", "flatten_hwc", R.rel_l2(R.head(tsd, s4, ("flatten_hwc",)), h))
    e = R.embed(tsd, R.TINY, True, x)
    y = (x + 0.3 * (R.smooth_images(3, 32, 32, 42) * 2 - 1).double()).clamp(-1, 1)
    sim = (e * R.embed(tsd, R.TINY, True, y)).sum(1)
    for fault in ("bn_through_padding", "prelu_as_relu", "flatten_hwc", "no_se", "se_mean_over_window", "shortcut_offset", "no_l2norm"):
        ef = R.embed(tsd, R.TINY, True, x, (fault,))
        note("embedding", fault, R.rel_l2(ef, e))
        print(f"ID-FAULT similarity shift of {fault}: {float(((ef * R.embed(tsd, R.TINY, True, y, (fault,))).sum(1) - sim).abs().min()):.3e}")
        if fault == "no_l2norm":     # the similarity is the embeddings' dot product: it answers for the normalisation
            note("similarity", fault, ((ef * R.embed(tsd, R.TINY, True, y, (fault,))).sum(1) - sim).abs())
    # a wrong eps shows where the variances are small: the low-variance copy of the tiny tower, stage by stage and whole
    lsd = R.low_variance(tsd)
    prev = x
    for s in range(6):
        true = R.stage(lsd, R.TINY, True, s, prev)
        wrong = R.stage(lsd, R.TINY, True, s, prev, ("bn_eps_0",))
        if s in (0, 5):
            note("input_layer" if s == 0 else "head", "bn_eps_0", R.rel_l2(wrong, true))
        else:
            inner, border = R.rel_l2_split(wrong, true)
            note("unit_border", "bn_eps_0", border)
            if inner.any():
                note("unit_interior", "bn_eps_0", inner)
        prev = true
    note("embedding", "bn_eps_0", R.rel_l2(R.embed(lsd, R.TINY, True, x, ("bn_eps_0",)), R.embed(lsd, R.TINY, True, x)))
    # the metric end to end: the preprocess faults reach the similarity
    a = R.smooth_images(2, 96, 96, 81)
    b = R.perturbed(a, 0.3, 82)
    true_sim, true_a, _ = R.id_similarity(tsd, R.TINY, True, a, b, input_size=32)
    for fault in ("crop_shifted", "pool_floor_windows"):
        fs, fa, _ = R.id_similarity(tsd, R.TINY, True, a, b, input_size=32, faults=(fault,))
        note("embedding", fault, R.rel_l2(fa, true_a))
    assert set(seen) == set(R.TOL)
    assert {f for v in seen.values() for f, _ in v} == set(R.FAULTS)
    for bound, v in sorted(seen.items()):
        fault, dev = min(v, key=lambda t: t[1])
        print(f"ID-FAULT {bound}: bound {R.TOL[bound]:.1e}, smallest deviation {dev:.3e} ({fault})")


def test_published_fault_deviations_on_ir_se50(ir_se50):
    """The four deviations the feature was specified with, recomputed: the minimum embedding rel-L2 shift over four images."""
    m, sd = ir_se50
    x = (R.smooth_images(4, 112, 112, 51) * 2 - 1).double()
    e = R.embed(sd, m.blocks, True, x)
    for fault, least in (("bn_through_padding", 2e-2), ("flatten_hwc", 1.0)):
        dev = float(R.rel_l2(R.embed(sd, m.blocks, True, x, (fault,)), e).min())
        print(f"ID-FAULT ir_se50 {fault}: {dev:.3e}")
        assert dev >= least and R.TOL["embedding"] * 10 <= dev


# ------------------------------------------------------------------------------------------------------------ PairMetrics
class _StubTower:
    """Stands in for a Backbone: embeddings from the image means, no kernels."""
    input_size = 8

    def preprocess(self, images, normalize=False, crop=True):
        return images

    def embed_nhwc(self, x, chunk=32):
        e = torch.stack([x.mean((1, 2, 3)), x.amax((1, 2, 3)), x.amin((1, 2, 3))], 1)
        return torch.nn.functional.pad(e / e.norm(dim=1, keepdim=True), (0, 509)).contiguous()


def test_pair_metrics_without_identity_is_unchanged_and_gains_the_column_with_it(monkeypatch):
    from uspace_amd import _hip
    from uspace_amd.libs import arcface
    from uspace_amd.tools import id_metrics, pair_metrics
    from uspace_amd.tools.pair_metrics import PairMetrics
    sig = inspect.signature(PairMetrics.__init__)
    assert list(sig.parameters) == ["self", "device", "lpips", "net", "structure", "identity"]
    assert sig.parameters["structure"].default is None
    assert sig.parameters["identity"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["identity"].default is None
    assert PairMetrics(device="cpu")._identity is None and PairMetrics("cpu", None, "alex", None, identity=None)._identity is None
    with pytest.raises(TypeError):
        PairMetrics(device="cpu", identitee=object())
    pm = PairMetrics(device="cpu")
    assert list(pm._parts) == ["lpips", "ssim", "psnr"] and list(pm.values) == ["lpips", "ssim", "psnr"] and pm.n == 0
    assert list(PairMetrics(device="cpu", structure=object()).values) == ["lpips", "ssim", "psnr", "structure"]
    assert list(PairMetrics(device="cpu", identity=object()).values) == ["lpips", "ssim", "psnr", "identity"]
    assert list(PairMetrics(device="cpu", structure=object(), identity=object()).values) == ["lpips", "ssim", "psnr", "structure", "identity"]
    # the kernels stubbed on the host: the column is the fp64 dot product of the tower's embeddings of the quantised images
    monkeypatch.setattr(_hip, "require_device", lambda t, name="tensor": None)
    monkeypatch.setattr(id_metrics, "similarity", lambda ea, eb: (ea.double() * eb.double()).sum(1))
    for name in ("ssim", "psnr"):
        monkeypatch.setattr(pair_metrics, name, lambda x, y, r: torch.zeros(x.shape[0], dtype=torch.float64))
    calls = []

    def fake_lpips(x, y, normalize=False):
        calls.append((x.clone(), y.clone()))
        return torch.zeros(x.shape[0], dtype=torch.float64)

    pm = PairMetrics(device="cpu", lpips=fake_lpips, identity=_StubTower())
    monkeypatch.setattr(PairMetrics, "lpips", property(lambda self: self._lpips))
    a, b = R.smooth_images(3, 8, 8, 1), R.smooth_images(3, 8, 8, 2)
    pm.update(a, b)
    qa, qb = calls[0]
    assert torch.equal(qa, (a * 255 + 0.5).clamp(0, 255).to(torch.uint8).float() / 255)
    t = _StubTower()
    want = (t.embed_nhwc(qa).double() * t.embed_nhwc(qb).double()).sum(1)
    out = pm.compute()
    assert np.array_equal(pm.values["identity"], want.numpy()) and out["identity"] == float(np.mean(want.numpy())) and out["n"] == 3
    assert arcface.IR_SE50 == dict(input_size=112, num_layers=50, mode="ir_se")


def test_folder_pairing_errors(tmp_path):
    from PIL import Image
    from uspace_amd.tools.id_metrics import calculate_id_similarity_given_paths
    for d in ("a", "b", "c"):
        (tmp_path / d).mkdir()
    img = lambda s: Image.fromarray(np.zeros((s, s, 3), dtype=np.uint8))
    img(16).save(tmp_path / "a" / "x.png")
    img(16).save(tmp_path / "b" / "y.png")
    img(24).save(tmp_path / "c" / "x.png")
    with pytest.raises(ValueError, match="pair up"):
        calculate_id_similarity_given_paths(tmp_path / "a", tmp_path / "b", None, device="cpu")
    with pytest.raises(ValueError, match="sizes differ"):
        calculate_id_similarity_given_paths(tmp_path / "a", tmp_path / "c", None, device="cpu")
    with pytest.raises(ValueError, match="no images"):
        calculate_id_similarity_given_paths(tmp_path / "a" / "none", tmp_path / "b" / "none", None, device="cpu")
