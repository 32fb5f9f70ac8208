"""No GPU: the float64 restatement of SegFormer (tests/segformer_stages.py) against ``transformers``' own float64 run in
tests/golden/segformer_tiny.npz, the module's keys against that model's, the library's parameter table against the module, every
bound of ``segformer_cases.TOL`` bracketed between the working-precision restatement and the planted faults, the seeded nets' label
maps, and the refusals."""
import ctypes

import numpy as np
import pytest
import torch

from tests import segformer_cases as C
from tests import segformer_stages as R
from uspace_amd.libs import segformer as _feature  # noqa: F401  (every test here is about the tower: none passes without it)


@pytest.fixture(scope="module")
def golden():
    g = np.load(C.GOLDEN)
    arch, sd = C.net("golden")
    m = C.module("golden")
    x = R.normalise(C.images(2, *C.GOLDEN_SIZE), m.mean, m.std)
    return g, arch, sd, x, R.forward(sd, arch, x)


def test_restatement_meets_transformers_float64(golden):
    g, arch, sd, x, taps = golden
    idx = R.stage_index(arch)
    norms = [taps[n] for n, e in enumerate(idx) if e[0] == "norm"]
    assert str(g["images_sha256"]) == C.sha256(C.images(2, *C.GOLDEN_SIZE).numpy())
    for i in range(4):                          # stored rounded to float32 (2^-24 relative per element)
        assert g[f"hidden_{i}"].dtype == np.float32 and R.rel_l2(norms[i].permute(0, 3, 1, 2).numpy(), g[f"hidden_{i}"]) < 6e-8, i
    assert g["logits"].dtype == np.float64 and g["logits"].shape == (2, 6, 25, 33)
    assert R.rel_l2(taps[-1].permute(0, 3, 1, 2).numpy(), g["logits"]) < 1e-13


def test_keys_shapes_and_epsilons_are_the_models(golden):
    g = golden[0]
    m = C.module("golden")
    sd = m.state_dict()
    assert sorted(sd) == list(g["keys"])
    assert [",".join(str(d) for d in sd[k].shape) for k in g["keys"]] == list(g["shapes"])
    mine = {n: float(mod.eps) for n, mod in m.named_modules() if isinstance(mod, (torch.nn.LayerNorm, torch.nn.BatchNorm2d))}
    assert sorted(mine) == list(g["eps_names"]) and [mine[k] for k in sorted(mine)] == list(g["eps_values"])
    bad = dict(sd)
    bad.pop("decode_head.classifier.bias")
    with pytest.raises(RuntimeError):
        m.load_state_dict(bad)
    assert m.training is False and m.train().training is False


def test_library_parameter_table_matches_the_module():
    from uspace_amd import _hip
    from uspace_amd.libs.segformer import MIT_B1, MIT_B2, MIT_B5, SegFormer
    L = _hip.lib()
    for m in (C.module("golden"), C.module("seeded19"), SegFormer(**MIT_B1), SegFormer(**MIT_B2, num_labels=150), SegFormer(**MIT_B5)):
        cfg = m._c_cfg()
        ps = m._canonical_params()
        assert L.uspace_segformer_num_params(ctypes.byref(cfg)) == len(ps)
        assert [L.uspace_segformer_param_numel(ctypes.byref(cfg), i) for i in range(len(ps))] == [p.numel() for p in ps]
        assert L.uspace_segformer_num_stages(ctypes.byref(cfg)) == len(m.stage_shapes(64, 64)) == len(R.stage_index(C.arch_of(m)))
        assert L.uspace_segformer_weight_bytes(ctypes.byref(cfg)) > 2 * sum(p.numel() for p in ps if p.dim() == 2)
        assert L.uspace_segformer_workspace_bytes(ctypes.byref(cfg), 1, 64, 64) > 0
        assert L.uspace_segformer_workspace_bytes(ctypes.byref(cfg), 1, 576, 576) > 0
        for B, H, W in ((1, 608, 608), (1, 31, 64), (0, 64, 64), (1, 64, 16385)):
            assert L.uspace_segformer_workspace_bytes(ctypes.byref(cfg), B, H, W) == 0, (B, H, W)


def _stage_bound(kind):
    return C.TOL["block_tight"] if kind == "block" else C.TOL[{"embed": "embed", "norm": "norm"}.get(kind, "head")]


def _acts(arch, sd, x, taps, fault):
    """[(kind, i, j, error, bound)] of the tap stages a fault moves, each from that stage's own exact inputs (blocks: the
    working-precision model on both sides)."""
    seen = []
    for k, (kind, i, j) in enumerate(R.stage_index(arch)):
        ref = R.step(sd, arch, k, x, taps, rnd=kind == "block")
        e = R.rel_l2(R.step(sd, arch, k, x, taps, rnd=kind == "block", fault=fault), ref)
        if e > 0:
            seen.append((kind, i, j, e, _stage_bound(kind)))
    return seen


@pytest.fixture(scope="module")
def eps5():
    arch, sd = C.net("eps5")
    m = C.module("eps5")
    assert arch["eps"] == C.EPS5 and len(set(C.EPS5.values())) == 5
    x = R.normalise(C.images(2, *C.GOLDEN_SIZE), m.mean, m.std)
    return arch, sd, x, R.forward(sd, arch, x)


@pytest.mark.parametrize("name", ["golden", "eps5"])
def test_every_bound_lies_above_the_working_precision_restatement(name, golden, eps5):
    arch, sd, x, taps = golden[1:] if name == "golden" else eps5
    idx = R.stage_index(arch)
    # the same statements in fp32 (convolutions, LayerNorms, the head; a block: bf16 where the kernels round, fp32 elsewhere)
    sd32, x32, t32 = R.as_f32(sd), x.float(), [t.float() for t in taps]
    worst = {}
    for k, (kind, i, j) in enumerate(idx):
        if kind == "block":
            key, e = "block_tight", R.rel_l2(R.step(sd32, arch, k, x32, t32, rnd=True).double(), R.step(sd, arch, k, x, taps, rnd=True))
        else:
            key, e = {"embed": "embed", "norm": "norm"}.get(kind, "head"), R.rel_l2(R.step(sd32, arch, k, x32, t32).double(), taps[k])
        worst[key] = max(worst.get(key, 0.0), e)
    print(f"SEGF-HOST fp32 restatement {name}: " + ", ".join(f"{k} {v:.2e}/{C.TOL[k]:.1e}" for k, v in worst.items()))
    assert set(worst) == {"embed", "block_tight", "norm", "head"}
    for k, v in worst.items():
        assert 0 < v < C.TOL[k], (k, v)
    # bf16 GEMM operands against plain float64: stage by stage from exact inputs, and end to end
    blocks = [R.rel_l2(R.step(sd, arch, k, x, taps, rnd=True), taps[k]) for k, e in enumerate(idx) if e[0] == "block"]
    tw = R.forward(sd, arch, x, rnd=True)
    lab, margin = R.labels(taps[-1], *C.GOLDEN_SIZE)
    labw, _ = R.labels(tw[-1], *C.GOLDEN_SIZE)
    print(f"SEGF-HOST working precision {name}: block {max(blocks):.3e}, logits {R.rel_l2(tw[-1], taps[-1]):.3e}, labels {np.mean(lab != labw):.3e}")
    assert C.TOL["block_loose"] > max(blocks) and C.TOL["logits"] > R.rel_l2(tw[-1], taps[-1])
    assert C.TOL["label_share"] > float(np.mean(lab != labw))


def test_every_fault_lies_ten_times_above_its_bounds(golden, eps5):
    g, arch, sd, x, taps = golden
    for f in R.FAULTS:
        if C.FAULT_BOUND[f] == "labels":
            continue
        seen = _acts(*eps5, f) if f == "eps_swapped" else _acts(arch, sd, x, taps, f)
        print(f"SEGF-HOST fault {f}: " + ", ".join(f"{k}{i}.{j} {e:.2e}/{b:.1e}" for k, i, j, e, b in seen))
        assert seen and all(e >= 10 * b for _k, _i, _j, e, b in seen), (f, seen)
    assert set(R.FAULTS) == set(C.FAULT_BOUND)
    # the swap acts in every patch embedding and every block, and nowhere on a net with one epsilon
    assert {k for k, *_ in _acts(*eps5, "eps_swapped")} == {"embed", "block"} and not _acts(arch, sd, x, taps, "eps_swapped")
    # any of the five epsilon fields reaching another kind of norm: at least 2 x the bound of every stage it moves
    for a in R.EPS_KINDS:
        for b in R.EPS_KINDS:
            if a != b:
                seen = _acts(*eps5, f"eps:{a}>{b}")
                assert seen and all(e >= 2 * bd for _k, _i, _j, e, bd in seen), (a, b, seen)
    # argmax_highest moves only exact ties: planted by a duplicated channel, as the label kernel's own test plants them
    # (interpolated with segops_cases.bilinear_f64, whose arithmetic is the same statement for every channel: torch's vectorised
    # interpolate does not keep two equal channels bit-equal)
    from tests import segops_cases as S
    z = taps[-1].numpy().copy()
    z[..., 5] = z[..., 1]
    up = S.bilinear_f64(z, *C.GOLDEN_SIZE)
    lo, hi = np.argmax(up, axis=-1), up.shape[-1] - 1 - np.argmax(up[..., ::-1], axis=-1)
    assert not (lo == 5).any() and (hi == 5).any() and not (hi == 1).any() and np.mean(lo != hi) > 0.02
    assert np.array_equal(lo, S.labels_f64(z, *C.GOLDEN_SIZE)[0])


@pytest.mark.parametrize("name", ["golden", "seeded19"])
def test_seeded_label_maps_are_not_degenerate(name):
    arch, sd = C.net(name)
    m = C.module(name)
    for H, W in ((96, 160), (100, 132)):
        x = R.normalise(C.images(2, H, W), m.mean, m.std)
        lab, _ = R.labels(R.forward(sd, arch, x)[-1], H, W)
        share = np.array([np.mean(lab == l) for l in range(arch["L"])])
        print(f"SEGF-HOST labels {name} {H}x{W}: {np.round(np.sort(share)[::-1][:6], 3)}")
        assert int((share >= 0.02).sum()) >= 4


def test_weights_file(tmp_path):
    from uspace_amd.libs.segformer import SegFormer
    m = C.module("golden")
    path = tmp_path / "tiny.pt"
    torch.save(m.state_dict(), path)
    again = SegFormer(**C.TINY, num_labels=6, weights=str(path))
    assert all(torch.equal(v, again.state_dict()[k]) for k, v in m.state_dict().items()) and again._missing is None
    assert SegFormer(**C.TINY, num_labels=6)._missing and SegFormer(**C.TINY, num_labels=6, seed=1)._missing is None


def test_from_hf_takes_keys_values_and_epsilons():
    tr = pytest.importorskip("transformers")
    from uspace_amd.libs.segformer import SegFormer
    cfg = tr.SegformerConfig(**{k: list(v) if isinstance(v, tuple) else v for k, v in C.TINY.items()}, num_labels=6)
    hf = tr.SegformerForSemanticSegmentation(cfg).eval()
    hf.decode_head.batch_norm.eps = 2e-5
    got = SegFormer.from_hf(hf)
    assert list(got.state_dict()) == list(hf.state_dict())
    assert all(torch.equal(v, got.state_dict()[k]) for k, v in hf.state_dict().items())
    assert got._eps() == (1e-5, 1e-5, 1e-5, 1e-5, 2e-5) and abs(got._cfg().eps_bn - 2e-5) < 1e-12
    got.segformer.stages[1].layer_norm.eps = 1e-3                   # set afterwards: one kind, two values
    with pytest.raises(NotImplementedError, match="different epsilons"):
        got._cfg()
    for st in got.segformer.stages:
        st.layer_norm.eps = 1e-3
    assert abs(got._cfg().eps_stage - 1e-3) < 1e-9 and got._packed._held is None
    with pytest.raises(NotImplementedError):
        SegFormer.from_hf(tr.SegformerForSemanticSegmentation(tr.SegformerConfig()))      # MiT-B0: head dim 32


def test_config_refusals():
    from uspace_amd import _hip
    from uspace_amd.libs.segformer import MIT_B1, SegFormer
    b0 = dict(MIT_B1, hidden_sizes=(32, 64, 160, 256))
    with pytest.raises(NotImplementedError, match="head dim"):
        SegFormer(**b0)
    with pytest.raises(NotImplementedError, match="head dim"):
        SegFormer(**dict(MIT_B1, hidden_sizes=(64, 128, 320, 500)))
    with pytest.raises(NotImplementedError, match="num_labels"):
        SegFormer(**MIT_B1, num_labels=257)
    with pytest.raises(NotImplementedError):
        SegFormer(**dict(MIT_B1, depths=(2, 2, 2)))
    with pytest.raises(FileNotFoundError):
        SegFormer(**MIT_B1, weights="/nonexistent/segformer.pt")
    L = _hip.lib()
    i4 = ctypes.c_int * 4
    good = [i4(64, 128, 320, 512), i4(2, 2, 2, 2), i4(1, 2, 5, 8), i4(8, 4, 2, 1), i4(4, 4, 4, 4), 256, 19, 1e-5, 1e-5, 1e-5, 1e-5, 1e-5]
    assert L.uspace_segformer_num_params(ctypes.byref(_hip.SegformerConfig(*good))) > 0
    for pos, val in ((0, i4(32, 64, 160, 256)), (2, i4(2, 2, 5, 8)), (0, i4(64, 128, 320, 500)), (6, 257), (6, 0), (5, 130), (1, i4(2, 0, 2, 2)),
                     (3, i4(8, 4, 2, 17)), (7, 0.0)):
        bad = list(good)
        bad[pos] = val
        cfg = _hip.SegformerConfig(*bad)
        assert L.uspace_segformer_num_params(ctypes.byref(cfg)) == -1 and L.uspace_segformer_weight_bytes(ctypes.byref(cfg)) == 0, (pos,)
    assert L.uspace_segformer_num_params(None) == -1
