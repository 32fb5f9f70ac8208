"""The attribute-effect metric (tools/attr_metrics.py, ``uspace_attr_effect_f64``) on the GPU: the effect kernel against numpy
fp64 on hand-made logits and on the GPU's own logits, the metric end to end against the float64 stage model of
tests/resnet_stages.py, ``logit_std``, ``attribute_response``, ``PairMetrics`` with ``attributes`` set, and two folders of PNGs.
Every figure is printed before it is judged; the bounds are ``resnet_cases.TOL``."""
import numpy as np
import pytest
import torch

from tests import resnet_cases as C
from tests import resnet_stages as R

pytestmark = pytest.mark.gpu

_CLF = {}


def classifier(name):
    """(AttributeClassifier on the device, arch, state dict on the host), built once."""
    if name not in _CLF:
        from uspace_amd.tools.attr_metrics import AttributeClassifier
        arch, sd = C.net(name)
        _CLF[name] = (AttributeClassifier(C.module(name).cuda()), arch, sd)
    return _CLF[name]


def _stack(out):
    from uspace_amd.tools.attr_metrics import COLUMNS
    return np.stack([out[k] for k in COLUMNS], 1)


def test_effect_kernel_on_hand_made_logits():
    from uspace_amd.tools.attr_metrics import effect_columns
    za, zb = (torch.tensor(t, dtype=torch.float32).cuda() for t in (C.HAND_ZA, C.HAND_ZB))
    tgt, sg = torch.tensor(C.HAND_TARGET, dtype=torch.int32).cuda(), torch.tensor(C.HAND_SIGN).cuda()
    got = effect_columns(za, zb, tgt, sg).cpu().numpy()
    assert got.dtype == np.float64 and got.shape == (3, 4)
    assert np.allclose(got, C.HAND, rtol=0, atol=1e-15)
    assert got[1, 3] == 0.0 and got[1, 2] == 0.0           # nothing moved
    sigma = torch.tensor(C.HAND_SIGMA_VALUES).cuda()
    assert np.allclose(effect_columns(za, zb, tgt, sg, sigma).cpu().numpy(), C.HAND_WITH_SIGMA, rtol=0, atol=1e-15)
    # one attribute: no off-target terms; a target outside the attributes: four NaNs for that pair alone
    one = effect_columns(za[:, :1].contiguous(), zb[:, :1].contiguous(), torch.zeros(3, dtype=torch.int32).cuda(), sg).cpu().numpy()
    assert np.array_equal(one[0], [1.0, 1.0, 0.0, 1.0]) and np.array_equal(one[1], [0.0, 1.0, 0.0, 0.0])
    bad = effect_columns(za, zb, torch.tensor([0, 4, -1], dtype=torch.int32).cuda(), sg).cpu().numpy()
    assert np.allclose(bad[0], C.HAND[0], rtol=0, atol=1e-15) and np.isnan(bad[1:]).all()


@pytest.mark.parametrize("B,A", [(1, 40), (64, 40), (65, 11), (130, 3)])
def test_effect_kernel_against_numpy(B, A):
    """Random logits, more pairs than one 64-thread workgroup: exact to float64 rounding."""
    from uspace_amd.tools.attr_metrics import effect_columns
    g = torch.Generator().manual_seed(B * 100 + A)
    za = torch.randn(B, A, generator=g)
    zb = za + torch.randn(B, A, generator=g) * (torch.rand(B, A, generator=g) < 0.7)
    zb[B // 2] = za[B // 2]
    tgt = torch.randint(0, A, (B,), generator=g).to(torch.int32)
    sg = torch.where(torch.rand(B, generator=g) < 0.5, -1.0, 1.0)
    sigma = 0.25 + torch.rand(A, generator=g)
    for s in (None, sigma):
        got = effect_columns(za.cuda(), zb.cuda(), tgt.cuda(), sg.cuda(), None if s is None else s.cuda()).cpu().numpy()
        want = R.effect_columns(za.numpy(), zb.numpy(), tgt.numpy(), sg.numpy(), None if s is None else s.numpy())
        err = float(np.abs(got - want).max())
        print(f"RESNET-MEASURE effect-kernel {(B, A, s is not None)}: {err:.3e}")
        assert err <= 4e-16 * max(1.0, float(np.abs(want).max())) and np.array_equal(got[:, 1], want[:, 1])
        assert got[B // 2, 3] == 0.0


@pytest.mark.parametrize("name,H,W", [("golden_bottleneck", 40, 56), ("golden_basic", 33, 47), ("seeded", 64, 64)])
def test_attribute_effect_end_to_end(name, H, W):
    from uspace_amd.tools.attr_metrics import attribute_effect
    clf, arch, sd = classifier(name)
    a, b = C.effect_pairs(3, H, W)
    targets, signs = ["Smiling", 20, "Eyeglasses"], [1, -1, 1]
    tgt, sg = np.array([31, 20, 15]), np.array([1.0, -1.0, 1.0])
    za, zb = clf.logits(a.cuda()), clf.logits(b.cuda())
    sigma = clf.logit_std(torch.cat([a, b]).cuda())
    assert sigma.dtype == np.float64 and sigma.shape == (40,)
    assert np.allclose(sigma, torch.cat([za, zb]).double().cpu().numpy().std(axis=0), rtol=1e-13, atol=0)
    wa, wb = (R.forward(sd, arch, C.quantized(t))[0].numpy() for t in (a, b))      # the images through the float64 model
    errs = []
    for s in (None, sigma):
        got = _stack(attribute_effect(clf, a.cuda(), b.cuda(), targets, signs, s))
        # from the GPU's own logits: exact to float64 rounding
        s32 = None if s is None else s.astype(np.float32)
        own = R.effect_columns(za.cpu().numpy(), zb.cpu().numpy(), tgt, sg, s32)
        assert float(np.abs(got - own).max()) <= 4e-16 * max(1.0, float(np.abs(own).max()))
        want = R.effect_columns(wa, wb, tgt, sg, s32)
        errs.append(float(np.abs(got - want)[:, [0, 2, 3]].max()))
        print(f"RESNET-MEASURE effect {(name, H, W, s is not None)}: {errs[-1]:.3e} (bound {C.TOL['effect']:.1e})")
        assert np.array_equal(got[:, 1], want[:, 1])
        assert np.array_equal(got[0], [0.0, want[0, 1], 0.0, 0.0])      # pair 0 was left unmoved
        assert got[1, 3] > 0 and got[2, 2] > 0
    assert max(errs) <= C.TOL["effect"], errs


def test_attribute_response_on_a_sweep():
    from uspace_amd.tools.attr_metrics import attribute_response
    clf, arch, sd = classifier("seeded")
    a = C.images(2, 40, 56)
    scales = [-2.0, 0.0, 1.5]
    sweep = torch.stack([R.perturbed(a, 0.1 * s, 78) for s in scales]).cuda()
    out = attribute_response(clf, sweep, scales, "Smiling")
    assert out["logits"].shape == (3, 2, 40) and out["logits"].dtype == np.float64
    for i in range(3):
        assert np.array_equal(out["logits"][i], clf.logits(sweep[i]).double().cpu().numpy())
    want = np.stack([[np.polyfit(scales, out["logits"][:, b, j], 1)[0] for j in range(40)] for b in range(2)])
    assert np.allclose(out["slopes"], want, rtol=1e-9, atol=1e-12) and np.array_equal(out["target_slope"], out["slopes"][:, 31])
    assert float(np.abs(out["slopes"]).max()) > 0


def test_pair_metrics_attributes_and_folders(tmp_path):
    from PIL import Image
    from uspace_amd.tools.attr_metrics import COLUMNS, AttributeEffect, attribute_effect, calculate_attribute_effect_given_paths
    from uspace_amd.tools.lpips import LPIPS
    from uspace_amd.tools.pair_metrics import PairMetrics
    clf, arch, sd = classifier("seeded")
    a, b = C.effect_pairs(4, 96, 96)
    qa, qb = ((t * 255 + 0.5).clamp(0, 255).to(torch.uint8) for t in (a, b))
    for d, q in (("a", qa), ("b", qb)):
        (tmp_path / d).mkdir()
        for i in range(4):
            Image.fromarray(q[i].permute(1, 2, 0).numpy()).save(tmp_path / d / f"{i:03d}.png")
    direct = attribute_effect(clf, a.cuda(), b.cuda(), "Male", -1)
    out = calculate_attribute_effect_given_paths(tmp_path / "a", tmp_path / "b", clf, "Male", -1, device="cuda", batch_size=3)
    assert out["n"] == 4 and set(out["values"]) == set(COLUMNS)
    for k in COLUMNS:                                            # the written PNGs hold the quantised numbers
        assert out["values"][k].dtype == np.float64 and np.array_equal(out["values"][k], direct[k]), k
        assert out[k] == float(np.mean(direct[k]))
    wa, wb = (R.forward(sd, arch, q.float() / 255)[0].numpy() for q in (qa, qb))
    want = R.effect_columns(wa, wb, np.full(4, 20), np.full(4, -1.0))
    err = float(np.abs(_stack(direct) - want)[:, [0, 2, 3]].max())
    print(f"RESNET-MEASURE effect ('seeded', 96, 96, 'folders'): {err:.3e} (bound {C.TOL['effect']:.1e})")
    assert err <= C.TOL["effect"] and np.array_equal(direct["target_hit"], want[:, 1])

    lp = LPIPS("alex", seed=3).cuda()
    plain, with_attr = PairMetrics(device="cuda", lpips=lp), PairMetrics(device="cuda", lpips=lp)
    assert with_attr.attributes is None
    with_attr.attributes = AttributeEffect(clf, "Male", -1)
    for pm in (plain, with_attr):
        pm.update(a[:3], b[:3])
        pm.update(a[3:], b[3:])
    v0, v1 = plain.values, with_attr.values
    assert list(v0) == ["lpips", "ssim", "psnr"] and list(v1) == list(v0) + list(COLUMNS)
    for k in v0:
        assert np.array_equal(v0[k], v1[k]), k
    for k in COLUMNS:
        assert np.array_equal(v1[k], direct[k]), k
    res = with_attr.compute()
    assert res["n"] == 4 and res["selectivity"] == float(np.mean(direct["selectivity"])) and "selectivity" not in plain.compute()

    (tmp_path / "b" / "extra.png").write_bytes((tmp_path / "b" / "000.png").read_bytes())
    with pytest.raises(ValueError, match="pair up"):
        calculate_attribute_effect_given_paths(tmp_path / "a", tmp_path / "b", clf, "Male", device="cuda")


def test_device_and_shape_refusals():
    from uspace_amd import _hip
    from uspace_amd.tools.attr_metrics import attribute_effect, effect_columns
    clf, _, _ = classifier("seeded")
    a = C.images(2, 40, 56)
    with pytest.raises(_hip.UspaceHipError):
        attribute_effect(clf, a, a, "Male")
    with pytest.raises(ValueError):
        attribute_effect(clf, a.cuda(), a[:1].cuda(), "Male")
    z = torch.zeros(2, 40).cuda()
    tgt, sg = torch.zeros(2, dtype=torch.int32).cuda(), torch.ones(2).cuda()
    for args in ((z, z[:1], tgt, sg), (z, z, tgt.long(), sg), (z, z, tgt, sg.double()), (z, z, tgt[:1], sg), (z.double(), z, tgt, sg),
                 (z, z, tgt, sg, torch.ones(39).cuda())):
        with pytest.raises(_hip.UspaceHipError):
            effect_columns(*args)
