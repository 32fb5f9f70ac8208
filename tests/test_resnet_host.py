"""CPU-only checks of the attribute-classifier tower and the attribute-effect metric: the float64 stage model of
tests/resnet_stages.py against what Hugging Face computed (tests/golden/resnet_tiny.npz), every planted fault against the bounds
the GPU tests use, those bounds against a float32 restatement, the module's state dict against torchvision's layout and the
library's parameter table, ``from_hf``, the ABI rows, the effect columns on hand-made logits, ``PairMetrics`` left as it was,
argument errors and the conditioning of the seeded weights."""
import ctypes
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import resnet_cases as C
from tests import resnet_stages as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["uspace_resnet_num_params", "uspace_resnet_param_numel", "uspace_resnet_weight_bytes", "uspace_resnet_workspace_bytes",
               "uspace_resnet_pack_weights", "uspace_resnet_preprocess", "uspace_resnet_forward", "uspace_resnet_tap",
               "uspace_attr_effect_f64"]


# ------------------------------------------------------------------------------------------------------- the stage model
@pytest.mark.parametrize("name", ["bottleneck", "basic"])
def test_stage_model_reproduces_the_hf_golden(name):
    """Hidden states, pooled vector and logits of ``ResNetForImageClassification`` in float64, to float64 rounding; the weights
    are stored under torchvision's names, so the key mapping is judged with them."""
    arch, sd, z = R.golden(name)
    x = torch.from_numpy(z["images"])
    assert x.shape == (3, 3, 40, 56)
    logits, outs = R.forward(sd, arch, x)
    ends = np.cumsum(arch.layers)
    worst = float(R.rel_l2(outs[0], z[f"{name}_hidden_states_0"]).max())
    for i, e in enumerate(ends):
        want = z[f"{name}_hidden_states_{i + 1}"]
        assert tuple(outs[e].shape) == want.shape
        worst = max(worst, float(R.rel_l2(outs[e], want).max()))
    worst = max(worst, float(R.rel_l2(outs[-1], z[f"{name}_pooled"]).max()), float(R.rel_l2(logits, z[f"{name}_logits"]).max()))
    print(f"RESNET-GOLDEN {name}: worst rel-L2 {worst:.3e}")
    assert worst < 1e-13
    assert tuple(outs[ends[-1]].shape[2:]) == (2, 2) and tuple(outs[ends[1]].shape[2:]) == (5, 7)      # odd sides further down
    again, outs2 = R.forward(sd, arch, x, fault=None)
    assert torch.equal(again, logits) and all(torch.equal(a, b) for a, b in zip(outs, outs2))


def _fault_deviation(fault, kind, case, pick):
    """The smallest deviation (over the samples and the tied stages) of one fault on one case."""
    name, H, W, B = case
    arch, sd = C.net(name)
    x, z, outs = C.reference(name, H, W, B)
    if kind == "tower":
        return float(R.rel_l2(R.forward(sd, arch, x, fault)[0], z).min())
    if kind == "logits":
        return float(R.rel_l2(R.logits(sd, outs[-1], fault), z).min())
    devs = []
    specs = R.block_specs(arch)
    for s in range(R.n_stages(arch)):
        if R.stage_kind(arch, s) != kind or (pick is not None and not pick(specs[s - 1])):
            continue
        prev = x if s == 0 else outs[s - 1]
        devs.append(float(R.rel_l2(R.stage(sd, arch, s, prev, fault), outs[s]).min()))
    assert devs, (fault, case)
    return min(devs)


def test_every_fault_is_tied_to_a_bound_that_catches_it():
    """A condition on the bounds, not a measurement: each fault moves the stage it is tied to by at least 10 x that stage's GPU
    bound, on every case of its tie and for every sample.  Ends with the check that no fault lacks a tie."""
    seen = {}
    for fault, kind, cases, pick in C.FAULT_TIES:
        assert R.FAULTS[fault][0] == kind
        for case in cases:
            dev = _fault_deviation(fault, kind, case, pick)
            print(f"RESNET-FAULT {kind} {fault} {case}: {dev:.3e} (bound {C.TOL[kind]:.1e})")
            assert C.TOL[kind] * 10 <= dev, (fault, kind, case, dev)
            seen.setdefault(fault, []).append(dev)
    assert set(seen) == set(R.FAULTS), set(R.FAULTS) - set(seen)
    assert {k for k, _ in R.FAULTS.values()} <= set(C.TOL)


def test_max_pool_faults_change_the_map_not_only_its_values():
    arch, sd = C.net("golden_basic")
    x = C.images(1, 40, 56)
    true = R.stage(sd, arch, 0, x)
    assert tuple(true.shape[2:]) == (10, 14)
    assert tuple(R.stage(sd, arch, 0, x, "maxpool_pad_0").shape[2:]) == (9, 13)
    ceil = R.stage(sd, arch, 0, x, "maxpool_ceil")
    assert tuple(ceil.shape[2:]) == (11, 15) and torch.equal(ceil[:, :, :10, :14], true)


def test_float32_restatement_stays_inside_every_bound():
    """The same statements in fp32 on the CPU, stage by stage from the float64 model's previous stage: the bounds are reachable
    by fp32 arithmetic."""
    worst = {k: 0.0 for k in C.TOL}
    for name in C.NETS:
        arch, sd = C.net(name)
        for H, W in C.SIZES:
            x, z, outs = C.reference(name, H, W, 3)
            for s in range(R.n_stages(arch)):
                prev = x if s == 0 else outs[s - 1]
                k = R.stage_kind(arch, s)
                worst[k] = max(worst[k], float(R.rel_l2(R.stage(sd, arch, s, prev, dtype=torch.float32), outs[s]).max()))
            worst["logits"] = max(worst["logits"], float(R.rel_l2(R.logits(sd, outs[-1].float()), z).max()))
            z32 = R.forward(sd, arch, x, dtype=torch.float32)[0]
            worst["tower"] = max(worst["tower"], float(R.rel_l2(z32, z).max()))
            a, b = C.effect_pairs(3, H, W)
            tgt, sg = np.array([31, 20, 15]), np.array([1.0, -1.0, 1.0])
            za, zb = (R.forward(sd, arch, t)[0] for t in (a, b))
            za32, zb32 = (R.forward(sd, arch, t, dtype=torch.float32)[0] for t in (a, b))
            d = np.abs(R.effect_columns(za32.numpy(), zb32.numpy(), tgt, sg) - R.effect_columns(za.numpy(), zb.numpy(), tgt, sg))
            worst["effect"] = max(worst["effect"], float(d[:, [0, 2, 3]].max()))
    for k, v in worst.items():
        print(f"RESNET-FP32 {k}: {v:.3e} (bound {C.TOL[k]:.1e})")
        assert v <= C.TOL[k], (k, v)


# ------------------------------------------------------------------------------------------------- module and state dict
def test_resnet50_state_dict_is_torchvisions_layout():
    from uspace_amd import _hip
    from uspace_amd.libs.resnet import RESNET50, ResNet
    m = ResNet(**RESNET50)
    sd = m.state_dict()
    params = [k for k, _ in m.named_parameters()]
    stats = [k for k in sd if k.endswith(("running_mean", "running_var"))]
    counters = [k for k in sd if k.endswith("num_batches_tracked")]
    assert len(sd) == 320 and len(params) == 161 and len(stats) == 106 and len(counters) == 53
    shapes = {k: tuple(v.shape) for k, v in sd.items()}
    assert shapes["conv1.weight"] == (64, 3, 7, 7) and shapes["bn1.running_mean"] == (64,)
    assert shapes["layer1.0.conv1.weight"] == (64, 64, 1, 1) and shapes["layer1.0.conv3.weight"] == (256, 64, 1, 1)
    assert shapes["layer1.0.downsample.0.weight"] == (256, 64, 1, 1) and "layer1.1.downsample.0.weight" not in shapes
    assert shapes["layer2.0.conv2.weight"] == (128, 128, 3, 3) and m.layer2[0].conv2.stride == (2, 2) and m.layer2[0].conv1.stride == (1, 1)
    assert shapes["layer2.0.downsample.1.running_var"] == (512,) and shapes["layer3.5.bn3.weight"] == (1024,)
    assert shapes["layer4.2.bn3.num_batches_tracked"] == () and shapes["fc.weight"] == (40, 2048) and shapes["fc.bias"] == (40,)
    assert list(sd)[:6] == ["conv1.weight", "bn1.weight", "bn1.bias", "bn1.running_mean", "bn1.running_var", "bn1.num_batches_tracked"]
    assert list(sd)[-2:] == ["fc.weight", "fc.bias"]
    # the library's parameter table is the state dict without num_batches_tracked, in order
    tensors = [k for k in sd if not k.endswith("num_batches_tracked")]
    L = _hip.lib()
    r = ctypes.byref(m.cfg)
    assert L.uspace_resnet_num_params(r) == 267 == len(tensors)
    assert [L.uspace_resnet_param_numel(r, i) for i in range(267)] == [sd[k].numel() for k in tensors]
    assert L.uspace_resnet_param_numel(r, 267) == -1 and L.uspace_resnet_param_numel(r, -1) == -1
    assert L.uspace_resnet_weight_bytes(r) >= 4 * (sum(p.numel() for p in m.parameters()) - 2 * 26560)      # one shift per batch norm stays
    assert 0 < L.uspace_resnet_workspace_bytes(r, 1, 224, 224) < L.uspace_resnet_workspace_bytes(r, 4, 224, 224)
    assert L.uspace_resnet_workspace_bytes(r, 1, 224, 224) < L.uspace_resnet_workspace_bytes(r, 1, 224, 320)
    assert not m.training and not m.train().training


@pytest.mark.parametrize("preset,n_blocks,n_tensors", [("RESNET18", 8, 102), ("RESNET34", 16, 182), ("RESNET101", 33, 522)])
def test_presets(preset, n_blocks, n_tensors):
    from uspace_amd import _hip
    from uspace_amd.libs import resnet
    m = resnet.ResNet(**getattr(resnet, preset))
    sd = m.state_dict()
    tensors = [k for k in sd if not k.endswith("num_batches_tracked")]
    assert sum(m.layers) == n_blocks and len(tensors) == n_tensors
    assert ("layer1.0.conv3.weight" in sd) == (m.block == "bottleneck") and ("layer1.0.downsample.0.weight" in sd) == (m.block == "bottleneck")
    L = _hip.lib()
    r = ctypes.byref(m.cfg)
    assert L.uspace_resnet_num_params(r) == len(tensors)
    assert [L.uspace_resnet_param_numel(r, i) for i in range(len(tensors))] == [sd[k].numel() for k in tensors]


def test_python_stage_shapes_match_the_stage_model():
    from uspace_amd.libs.resnet import block_specs
    for name in C.NETS:
        arch, sd = C.net(name)
        m = C.module(name)
        assert [s[1:] for s in R.block_specs(arch)] == block_specs(m.block, m.layers, m.planes, m.stem)
        for H, W in C.SIZES + ((32, 32), (224, 320)):
            x = torch.zeros(1, 3, H, W)
            shapes = m.stage_shapes(H, W)
            assert len(shapes) == R.n_stages(arch) - 1
            for s, (h, w, c) in enumerate(shapes):
                x = R.stage(sd, arch, s, x)
                assert tuple(x.shape) == (1, c, h, w)
    assert C.module("seeded").stage_shapes(32, 32)[-1][:2] == (1, 1) and C.module("seeded").stage_shapes(224, 320)[-1][:2] == (7, 10)


def test_loader_is_strict_and_never_downloads(tmp_path):
    from uspace_amd import _hip
    from uspace_amd.libs.resnet import ResNet
    arch, sd = C.net("seeded")
    kw = dict(block=arch.block, layers=arch.layers, planes=arch.planes, stem=arch.stem)
    with pytest.raises(FileNotFoundError, match="never downloads"):
        ResNet(**kw, weights=str(tmp_path / "absent.pth"))
    path = tmp_path / "seeded.pth"
    torch.save(sd, path)
    again = ResNet(**kw, weights=str(path))
    assert all(torch.equal(v, again.state_dict()[k]) for k, v in sd.items())
    empty = ResNet(**kw)
    assert "weights=" in empty._missing and "never downloads" in empty._missing
    for bad in ({k: v for k, v in sd.items() if k != "layer2.0.downsample.1.running_var"}, dict(sd, extra=torch.zeros(1)),
                {k: v for k, v in sd.items() if k != "fc.weight"}, dict(sd, **{"fc.bias": torch.zeros(39)})):
        with pytest.raises(RuntimeError):
            empty.load_state_dict(bad)
        assert empty._missing
    empty.load_state_dict(sd)
    assert empty._missing is None
    with pytest.raises(_hip.UspaceHipError):       # there is no CPU path
        again(torch.zeros(1, 3, 32, 32))


def test_refused_configurations():
    from uspace_amd.libs.resnet import ResNet
    for kw in (dict(block="resnext"), dict(layers=(2, 2, 2)), dict(layers=(2, 0, 2, 2)), dict(planes=(64, 128, 256, 1024)),
               dict(planes=(64, 130, 256, 512)), dict(stem=30), dict(num_classes=0)):
        with pytest.raises(NotImplementedError):
            ResNet(**kw)
    with pytest.raises(ValueError):
        ResNet(std=(0.2, 0.0, 0.2))


class _HFStandIn:
    """What ``from_hf`` reads of a ``ResNetForImageClassification``: ``config`` and ``state_dict()``."""

    def __init__(self, cfg, sd):
        self.config = type("Config", (), cfg)()
        self._sd = sd

    def state_dict(self):
        return self._sd


def _hf_name(key):
    """The inverse of ``hf_key`` on torchvision's names."""
    if key.startswith("conv1."):
        return "resnet.embedder.embedder.convolution." + key[6:]
    if key.startswith("bn1."):
        return "resnet.embedder.embedder.normalization." + key[4:]
    if key.startswith("fc."):
        return "classifier.1." + key[3:]
    layer, i, what, *rest = key.split(".")
    head = f"resnet.encoder.stages.{int(layer[5:]) - 1}.layers.{i}."
    if what == "downsample":
        return head + "shortcut." + ("convolution." if rest[0] == "0" else "normalization.") + ".".join(rest[1:])
    return head + f"layer.{int(what[-1]) - 1}." + ("convolution." if what.startswith("conv") else "normalization.") + ".".join(rest)


@pytest.mark.parametrize("name", ["bottleneck", "basic"])
def test_from_hf_round_trip(name):
    """The golden's weights renamed to Hugging Face's keys and converted back: the same module, tensor for tensor."""
    from uspace_amd.libs.resnet import ResNet, hf_key
    arch, sd, z = R.golden(name)
    cfg = json.loads(str(z[f"{name}_config"]))
    hf_sd = {_hf_name(k): v for k, v in sd.items()}
    assert "resnet.encoder.stages.1.layers.0.shortcut.normalization.running_var" in hf_sd and "classifier.1.bias" in hf_sd
    assert [hf_key(k) for k in hf_sd] == list(sd)
    m = ResNet.from_hf(_HFStandIn(cfg, hf_sd))
    assert (m.block, m.layers, m.planes, m.stem, m.num_classes) == (arch.block, arch.layers, arch.planes, arch.stem, 40)
    got = m.state_dict()
    assert set(got) == set(sd) and all(torch.equal(got[k].double(), sd[k].double()) for k in sd)      # (HF lists a shortcut first)
    assert got["bn1.num_batches_tracked"].dtype == torch.long
    for bad in (dict(cfg, hidden_act="gelu"), dict(cfg, downsample_in_bottleneck=True), dict(cfg, downsample_in_first_stage=True)):
        with pytest.raises(NotImplementedError):
            ResNet.from_hf(_HFStandIn(bad, hf_sd))
    with pytest.raises(KeyError):
        hf_key("resnet.pooler.weight")


def test_from_hf_on_a_transformers_model():
    """The real class, built offline from a config: its keys convert strictly and the float64 stage model on the converted state
    dict gives the logits Hugging Face computes."""
    transformers = pytest.importorskip("transformers")
    from uspace_amd.libs.resnet import ResNet
    cfg = transformers.ResNetConfig(num_channels=3, embedding_size=8, hidden_sizes=[16, 32, 48, 64], depths=[1, 1, 2, 1],
                                    layer_type="bottleneck", hidden_act="relu", downsample_in_first_stage=False,
                                    downsample_in_bottleneck=False, num_labels=5)
    torch.manual_seed(4)
    hf = transformers.ResNetForImageClassification(cfg).eval()
    for mod in hf.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.running_mean.normal_(0, 0.2)
            mod.running_var.uniform_(0.5, 1.5)
            mod.weight.data.uniform_(0.7, 1.3)
            mod.bias.data.normal_(0, 0.2)
    m = ResNet.from_hf(hf)
    assert (m.block, m.layers, m.planes, m.stem, m.num_classes) == ("bottleneck", (1, 1, 2, 1), (4, 8, 12, 16), 8, 5)
    x = R.smooth_images(2, 40, 56, 5)
    arch = R.Arch(m.block, m.layers, m.planes, m.stem)
    with torch.no_grad():
        want = hf.double()(pixel_values=R.normalize(arch, x.double())).logits
    got = R.forward(m.state_dict(), arch, x)[0]
    assert float(R.rel_l2(got, want).max()) < 1e-12


# ------------------------------------------------------------------------------------------------------------------- ABI
def test_abi_rows():
    from uspace_amd import _hip
    hdr = open(os.path.join(ROOT, "include", "uspace_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    declared = set(re.findall(r"USPACE_API\s+[\w\s\*]+?\b(uspace_\w+)\s*\(", hdr))
    L = _hip.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _hip.SIGNATURES and hasattr(L, name), name
    assert {n for n in declared if n.startswith(("uspace_resnet_", "uspace_attr_"))} == set(NEW_SYMBOLS)
    for name in ("uspace_resnet_forward", "uspace_resnet_preprocess", "uspace_attr_effect_f64", "uspace_resnet_config"):
        assert name in doc, name
    assert declared == set(_hip.SIGNATURES)
    assert "#define USPACE_ABI_VERSION 11" in hdr and L.uspace_abi_version() == _hip.ABI_VERSION == 11
    assert len(_hip.SIGNATURES["uspace_resnet_workspace_bytes"][1]) == 4 and len(_hip.SIGNATURES["uspace_resnet_preprocess"][1]) == 8
    assert len(_hip.SIGNATURES["uspace_resnet_forward"][1]) == 11 and len(_hip.SIGNATURES["uspace_resnet_tap"][1]) == 11
    assert len(_hip.SIGNATURES["uspace_attr_effect_f64"][1]) == 9
    fields = re.search(r"struct uspace_resnet_config \{(.*?)\};", hdr, re.S).group(1)
    assert re.findall(r"int\s+(\w+)(?:\[4\])?;", fields) == [f for f, _ in _hip.ResnetConfig._fields_] == \
        ["stem", "planes", "blocks", "bottleneck", "num_outputs"]
    assert ctypes.sizeof(_hip.ResnetConfig) == 44


def _cfg(stem=16, planes=(16, 32, 48, 64), blocks=(1, 1, 1, 1), bottleneck=1, num_outputs=40):
    from uspace_amd import _hip
    return _hip.ResnetConfig(stem, (ctypes.c_int * 4)(*planes), (ctypes.c_int * 4)(*blocks), bottleneck, num_outputs)


def test_invalid_configs_report_no_parameters_and_no_bytes():
    from uspace_amd import _hip
    L = _hip.lib()
    good = ctypes.byref(_cfg())
    assert L.uspace_resnet_num_params(good) == 5 + 4 * 20 + 2 and L.uspace_resnet_weight_bytes(good) > 0
    assert L.uspace_resnet_workspace_bytes(good, 2, 32, 32) > 0 and L.uspace_resnet_workspace_bytes(good, 2, 33, 47) > 0
    for bad in (_cfg(planes=(16, 30, 48, 64)), _cfg(stem=18), _cfg(blocks=(1, 0, 1, 1)), _cfg(num_outputs=0), _cfg(bottleneck=2),
                _cfg(planes=(16, 32, 48, 1024)), _cfg(planes=(16, 32, 48, 4096), bottleneck=0), _cfg(stem=0)):
        r = ctypes.byref(bad)
        assert L.uspace_resnet_num_params(r) == -1 and L.uspace_resnet_param_numel(r, 0) == -1
        assert L.uspace_resnet_weight_bytes(r) == 0 and L.uspace_resnet_workspace_bytes(r, 1, 64, 64) == 0
    for B, H, W in ((1, 31, 64), (1, 64, 31), (0, 64, 64), (40000, 64, 64), (1, 20000, 64), (32767, 4096, 4096)):
        assert L.uspace_resnet_workspace_bytes(good, B, H, W) == 0, (B, H, W)
    assert L.uspace_resnet_workspace_bytes(None, 1, 64, 64) == 0 and L.uspace_resnet_num_params(None) == -1


# ---------------------------------------------------------------------------------------------------------- the effect
class _StubTower:
    """Stands in for a ResNet: the logits are the first row of the first channel, no kernels."""

    def __init__(self, A):
        self.num_classes = A

    def __call__(self, images, chunk=32):
        return images[:, 0, 0, :self.num_classes].contiguous()


def _as_images(z):
    z = torch.as_tensor(z, dtype=torch.float32)
    return z[:, None, None, :].repeat(1, 3, 1, 1)


ZA, ZB, HAND, SIGMA, HAND_SIGMA = C.HAND_ZA, C.HAND_ZB, C.HAND, C.HAND_SIGMA_VALUES, C.HAND_WITH_SIGMA


def _host_effect(monkeypatch):
    """The effect kernel replaced by the numpy statement of tests/resnet_stages.py, so that the surface runs on the host."""
    from uspace_amd import _hip
    from uspace_amd.tools import attr_metrics
    monkeypatch.setattr(_hip, "require_device", lambda t, name="tensor": None)
    seen = []

    def columns(za, zb, target, sign, sigma=None):
        seen.append((target.clone(), sign.clone(), None if sigma is None else sigma.clone()))
        assert target.dtype == torch.int32 and sign.dtype == torch.float32 and za.dtype == torch.float32
        return torch.from_numpy(R.effect_columns(za.numpy(), zb.numpy(), target.numpy(), sign.numpy(), None if sigma is None else sigma.numpy()))

    monkeypatch.setattr(attr_metrics, "effect_columns", columns)
    return attr_metrics, seen


def test_effect_columns_on_hand_made_logits(monkeypatch):
    A, seen = _host_effect(monkeypatch)
    clf = A.AttributeClassifier(_StubTower(4), names=["a", "b", "c", "d"])
    a, b = _as_images(ZA), _as_images(ZB)
    # one target per pair, names and an index mixed; one sign per pair
    out = A.attribute_effect(clf, a, b, ["a", 1, "d"], sign=[1, 1, -1], quantize=False)
    assert list(out) == list(A.COLUMNS) == ["target_shift", "target_hit", "off_target", "selectivity"]
    got = np.stack([out[k] for k in A.COLUMNS], 1)
    assert got.dtype == np.float64 and np.allclose(got, HAND, rtol=0, atol=1e-15)
    assert seen[-1][0].tolist() == [0, 1, 3] and seen[-1][1].tolist() == [1.0, 1.0, -1.0] and seen[-1][2] is None
    assert out["selectivity"][1] == 0.0 and out["off_target"][1] == 0.0       # nothing moved
    # sigma
    out = A.attribute_effect(clf, a, b, ["a", "b", "d"], sign=[1, 1, -1], sigma=SIGMA, quantize=False)
    assert np.allclose(np.stack([out[k] for k in A.COLUMNS], 1), HAND_SIGMA, rtol=0, atol=1e-15)
    assert seen[-1][2].tolist() == SIGMA
    # one target by name and sign -1 for all pairs
    out = A.attribute_effect(clf, a, b, "d", sign=-1, quantize=False)
    assert np.allclose(out["target_shift"], [0.5, 0.0, 2.0]) and out["target_hit"].tolist() == [1.0, 0.0, 1.0]
    assert np.allclose(out["off_target"], [1.5 / 3, 0.0, 2.0 / 3]) and np.allclose(out["selectivity"], [0.25, 0.0, 0.5])
    # the same through the bound callable and through the index
    eff = A.AttributeEffect(clf, 3, sign=-1)
    again = eff(a, b, quantize=False)
    assert all(np.array_equal(again[k], out[k]) for k in A.COLUMNS)
    assert np.array_equal(eff.columns(a, b, quantize=False).numpy()[:, 0], out["target_shift"])
    # quantize=True rounds the images as save_image does before the tower sees them
    x = torch.full((1, 3, 1, 4), 0.5012)
    assert torch.equal(clf.logits(x), torch.full((1, 4), 128 / 255)) and torch.equal(clf.logits(x, quantize=False), torch.full((1, 4), 0.5012))


def test_default_names_are_the_celeba_table():
    from uspace_amd.tools.attr_metrics import AttributeClassifier
    from uspace_amd.tools.utils_attr import get_attr_name_from_attr_id
    clf = AttributeClassifier(_StubTower(40))
    assert clf.names == [get_attr_name_from_attr_id(i, "celeba") for i in range(40)] and len(clf.names) == 40
    assert clf.index("Smiling") == 31 and clf.index("Male") == 20 and clf.index("Eyeglasses") == 15 and clf.index(7) == 7
    for bad in ("Smile", 40, -1, 1.5, True):
        with pytest.raises(ValueError):
            clf.index(bad)
    with pytest.raises(ValueError):
        AttributeClassifier(_StubTower(11))
    with pytest.raises(ValueError):
        AttributeClassifier(_StubTower(2), names=["a", "a"])


def test_effect_argument_errors(monkeypatch):
    A, _ = _host_effect(monkeypatch)
    clf = A.AttributeClassifier(_StubTower(4), names=["a", "b", "c", "d"])
    a, b = _as_images(ZA), _as_images(ZB)
    for kw in (dict(target="e"), dict(target=["a", "b"]), dict(target="a", sign=0), dict(target="a", sign=[1, -1]),
               dict(target="a", sign=2.0), dict(target="a", sigma=[1, 1, 1]), dict(target="a", sigma=[1, 1, 0, 1]),
               dict(target="a", sigma=[1, 1, float("nan"), 1])):
        with pytest.raises(ValueError):
            A.attribute_effect(clf, a, b, **kw)
    with pytest.raises(ValueError):
        A.attribute_effect(clf, a, b[:2], "a")
    with pytest.raises(ValueError):
        A.AttributeEffect(clf, "e")
    with pytest.raises(ValueError):
        clf.logits(torch.zeros(3, 1, 4))
    with pytest.raises(ValueError):
        clf.logit_std(_as_images(ZA[:1]), quantize=False)
    assert np.allclose(clf.logit_std(_as_images(ZB), quantize=False), np.asarray(ZB).std(axis=0))


def test_attribute_response_slopes(monkeypatch):
    A, _ = _host_effect(monkeypatch)
    clf = A.AttributeClassifier(_StubTower(4), names=["a", "b", "c", "d"])
    scales = [-2.0, 0.0, 1.0, 3.0]
    base = np.array([[0.1, 0.2, 0.3, 0.4], [0.5, 0.1, 0.0, 0.2]])
    slope = np.array([[0.25, 0.0, -0.125, 0.0625], [0.5, 0.03125, 0.0, -0.25]])
    z = np.stack([base + s * slope for s in scales])                      # [S, B, A], exactly linear in the scale
    z[2, 1, 3] += 0.125                                                   # but for one point
    sweep = torch.stack([_as_images(z[s]) for s in range(4)])
    out = A.attribute_response(clf, sweep, scales, "a", quantize=False)
    assert out["logits"].shape == (4, 2, 4) and out["logits"].dtype == np.float64 and out["slopes"].shape == (2, 4)
    want = np.stack([[np.polyfit(scales, np.float32(z[:, b, a]).astype(np.float64), 1)[0] for a in range(4)] for b in range(2)])
    assert np.allclose(out["slopes"], want, rtol=0, atol=1e-12) and np.array_equal(out["target_slope"], out["slopes"][:, 0])
    assert np.allclose(out["slopes"][0], slope[0], atol=1e-7) and abs(out["slopes"][1, 3] - slope[1, 3]) > 1e-3
    for bad_scales in ([1.0, 1.0, 1.0, 1.0], [0.0, 1.0]):
        with pytest.raises(ValueError):
            A.attribute_response(clf, sweep, bad_scales, "a")
    with pytest.raises(ValueError):
        A.attribute_response(clf, sweep[0], scales, "a")


# ------------------------------------------------------------------------------------------------------------ PairMetrics
def test_pair_metrics_is_unchanged_until_attributes_are_set(monkeypatch):
    A, _ = _host_effect(monkeypatch)
    from uspace_amd.tools import pair_metrics
    from uspace_amd.tools.pair_metrics import PairMetrics
    sig = inspect.signature(PairMetrics.__init__)
    assert list(sig.parameters) == ["self", "device", "lpips", "net", "structure", "identity"]      # as it was
    pm = PairMetrics(device="cpu")
    assert pm.attributes is None
    assert list(pm._parts) == ["lpips", "ssim", "psnr"] and list(pm.values) == ["lpips", "ssim", "psnr"] and pm.n == 0
    pm.attributes = None
    assert list(pm.values) == ["lpips", "ssim", "psnr"]
    assert list(PairMetrics(device="cpu", structure=object(), identity=object()).values) == ["lpips", "ssim", "psnr", "structure", "identity"]
    # with the kernels stubbed on the host: the four columns are attribute_effect of the quantised images
    for name in ("ssim", "psnr"):
        monkeypatch.setattr(pair_metrics, name, lambda x, y, r: torch.zeros(x.shape[0], dtype=torch.float64))
    monkeypatch.setattr(PairMetrics, "lpips", property(lambda self: self._lpips))
    clf = A.AttributeClassifier(_StubTower(4), names=["a", "b", "c", "d"])
    pm = PairMetrics(device="cpu", lpips=lambda x, y, normalize=False: torch.zeros(x.shape[0], dtype=torch.float64))
    pm.attributes = A.AttributeEffect(clf, "c", sign=+1, sigma=SIGMA)
    assert list(pm.values) == ["lpips", "ssim", "psnr"] + list(A.COLUMNS)
    a, b = R.smooth_images(3, 8, 8, 1), R.smooth_images(3, 8, 8, 2)
    pm.update(a[:2], b[:2])
    pm.update(a[2:], b[2:])
    want = A.attribute_effect(clf, C.quantized(a), C.quantized(b), "c", +1, SIGMA, quantize=False)
    direct = A.attribute_effect(clf, a, b, "c", +1, SIGMA)
    out = pm.compute()
    for k in A.COLUMNS:
        assert np.array_equal(pm.values[k], want[k]) and np.array_equal(want[k], direct[k]) and out[k] == float(np.mean(want[k]))
    assert out["n"] == 3 and pm.values["target_shift"].dtype == np.float64
    with pytest.raises(ValueError, match="before the first update"):
        pm.attributes = None
    pm.reset()
    pm.attributes = None
    assert list(pm.values) == ["lpips", "ssim", "psnr"]


def test_folder_pairing_errors(tmp_path):
    from PIL import Image
    from uspace_amd.tools.attr_metrics import calculate_attribute_effect_given_paths
    for d in ("a", "b", "c"):
        (tmp_path / d).mkdir()
    img = lambda s: Image.fromarray(np.zeros((s, s, 3), dtype=np.uint8))
    img(32).save(tmp_path / "a" / "x.png")
    img(32).save(tmp_path / "b" / "y.png")
    img(48).save(tmp_path / "c" / "x.png")
    with pytest.raises(ValueError, match="pair up"):
        calculate_attribute_effect_given_paths(tmp_path / "a", tmp_path / "b", None, "Smiling", device="cpu")
    with pytest.raises(ValueError, match="sizes differ"):
        calculate_attribute_effect_given_paths(tmp_path / "a", tmp_path / "c", None, "Smiling", device="cpu")


# ---------------------------------------------------------------------------------------------------------- conditioning
def test_seeded_weights_are_well_conditioned():
    """The figures of the libs/resnet.py docstring, recomputed on the float64 model: unrelated images give different logits, and
    a perturbation moves them in proportion."""
    from uspace_amd.libs.resnet import RESNET50, ResNet
    m = ResNet(**RESNET50, seed=0)
    sd = m.state_dict()
    arch = R.Arch(m.block, m.layers, m.planes, m.stem)
    a = R.smooth_images(8, 64, 64, 11)
    za = R.forward(sd, arch, a)[0]
    std = za.std(0, unbiased=False)
    spread = torch.cdist(za, za)[~torch.eye(8, dtype=torch.bool)].mean()
    moved = {amp: float(((R.forward(sd, arch, R.perturbed(a, amp, 12))[0] - za).norm(dim=1) / spread).mean()) for amp in (0.001, 0.1, 1.0)}
    print(f"RESNET-SEED std {float(std.min()):.3f} .. {float(std.max()):.3f}, mean |z| {float(za.abs().mean()):.2f}, moved {moved}")
    assert float(std.min()) > 0.1 and float(za.abs().max()) < 50
    assert moved[0.001] < 0.01 and 0.02 < moved[0.1] < 0.5 and 0.5 < moved[1.0] < 5
