"""The SegFormer tower (libs/segformer.py; csrc/segformer.hip, csrc/attention_kv.hip) on the GPU against the float64 model of
tests/segformer_stages.py, on the golden net, a 19-label seeded net and one with a different epsilon in every kind of norm (each of
the five config fields has to reach its own norms), at 64 x 64, 96 x 160 and 100 x 132, B 1 and 3:

* every tap stage from the GPU's own previous stages (blocks against the working-precision model and against plain float64);
* the logits from the images, end to end, and against ``transformers``' own float64 logits of the golden file;
* the label map: the share of differing pixels, and no pixel differing whose float64 margin exceeds 4 x the worst logit error;
* bit-identity across batch size, position, ``chunk`` and a workspace filled with NaN patterns;
* MiT-B2 at 256^2 runs whole and repeats; the refusals; the consistency metric on the tower.

Every figure is printed before it is judged; the bounds are ``segformer_cases.TOL``."""
import numpy as np
import pytest
import torch

from tests import segformer_cases as C
from tests import segformer_stages as R

pytestmark = pytest.mark.gpu

_DEV = {}


def tower(name):
    if name not in _DEV:
        _DEV[name] = C.build(name).cuda()
    return _DEV[name]


def _check(kind, value, what):
    print(f"SEGF-MEASURE {kind} {what}: {value:.3e} (bound {C.TOL[kind]:.1e})")
    assert value <= C.TOL[kind], (kind, what, value)


_KIND = {"embed": "embed", "norm": "norm", "concat": "head", "fused": "head", "logits": "head"}


@pytest.mark.parametrize("B", C.BATCHES)
@pytest.mark.parametrize("size", C.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", ["golden", "seeded19", "eps5"])
def test_stages_logits_and_labels_against_float64(name, size, B):
    m = tower(name)
    arch, sd = C.net(name)
    H, W = size
    x = C.images(B, H, W)
    xn = R.normalise(x, m.mean, m.std)
    idx = R.stage_index(arch)
    shapes = m.stage_shapes(H, W)
    assert len(shapes) == len(idx)
    got = [m.tap(x.cuda(), k).cpu() for k in range(len(idx))]
    worst = {}
    for k, (kind, i, j) in enumerate(idx):
        assert got[k].shape == (B,) + shapes[k] and bool(torch.isfinite(got[k]).all())
        prev = [g.double() for g in got[:k]]
        if kind == "block":
            worst["block_tight"] = max(worst.get("block_tight", 0), R.rel_l2(got[k], R.step(sd, arch, k, xn, prev, rnd=True)))
            worst["block_loose"] = max(worst.get("block_loose", 0), R.rel_l2(got[k], R.step(sd, arch, k, xn, prev)))
        else:
            worst[_KIND[kind]] = max(worst.get(_KIND[kind], 0), R.rel_l2(got[k], R.step(sd, arch, k, xn, prev)))
    for kind, v in worst.items():
        _check(kind, v, (name, size, B))
    # end to end
    ref = R.forward(sd, arch, xn)[-1]
    z = m.logits_nhwc(x.cuda()).cpu()
    assert torch.equal(z, got[-1]) and torch.equal(m.logits(x.cuda()).cpu(), z.permute(0, 3, 1, 2))
    _check("logits", R.rel_l2(z, ref), (name, size, B))
    lab = m.labels(x.cuda()).cpu().numpy()
    want, margin = R.labels(ref, H, W)
    assert lab.dtype == np.uint8 and lab.shape == (B, H, W)
    _check("label_share", float(np.mean(lab != want)), (name, size, B))
    err = float((z.double() - ref).abs().max())
    far = (lab != want) & (margin > 4 * err)
    print(f"SEGF-MEASURE label-margin {(name, size, B)}: worst |logit error| {err:.3e}, {int(far.sum())} differing pixels beyond 4 x it")
    assert not far.any()
    assert sum(np.mean(lab == l) >= 0.02 for l in range(arch["L"])) >= 3


def test_golden_logits_against_transformers_float64():
    g = np.load(C.GOLDEN)
    m = tower("golden")
    x = C.images(2, *C.GOLDEN_SIZE)
    assert str(g["images_sha256"]) == C.sha256(x.numpy())
    z = m.logits(x.cuda()).cpu().numpy()
    _check("logits", R.rel_l2(z, g["logits"]), ("golden file", C.GOLDEN_SIZE, 2))


@pytest.mark.parametrize("size", [(64, 64), (100, 132)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_bits_do_not_depend_on_batch_position_chunk_or_workspace(size):
    m = tower("seeded19")
    x = C.images(5, *size).cuda()
    whole = m.logits_nhwc(x, chunk=5)
    for chunk in (1, 2, 3):
        assert torch.equal(m.logits_nhwc(x, chunk=chunk), whole), chunk
    order = [3, 0, 4, 1, 2]
    assert torch.equal(m.logits_nhwc(x[order].contiguous(), chunk=5), whole[order])
    assert torch.equal(m.logits_nhwc(x[2:3].contiguous()), whole[2:3])
    for fill in (0xFF, 0x7F):                                       # fp32 / bf16 NaN patterns
        assert torch.equal(m.logits_nhwc(x, chunk=5, ws_fill=fill), whole), fill
    k = len(m.stage_shapes(*size)) - 4
    assert torch.equal(m.tap(x[1:4].contiguous(), k)[1], m.tap(x, k)[2])
    assert torch.equal(m.labels(x, chunk=2), m.labels(x[order].contiguous())[[1, 3, 4, 0, 2]])


def test_mit_b2_at_256_runs_whole_and_repeats():
    from uspace_amd.libs.segformer import MIT_B2, SegFormer
    m = SegFormer(**MIT_B2, num_labels=19, seed=3).cuda()
    x = C.images(2, 256, 256).cuda()
    z = m.logits(x)
    assert z.shape == (2, 19, 64, 64) and bool(torch.isfinite(z).all()) and float(z.std()) > 0.05
    assert torch.equal(m.logits(x), z)
    lab = m.labels(x)
    assert lab.shape == (2, 256, 256) and torch.equal(lab, m.labels(x)) and len(torch.unique(lab)) >= 3


def test_refusals():
    from uspace_amd.libs.segformer import MIT_B1, SegFormer
    m = tower("seeded19")
    with pytest.raises(NotImplementedError, match="336"):
        m.logits(torch.zeros(1, 3, 608, 608).cuda())                # stage 0: 19 x 19 = 361 keys
    with pytest.raises(NotImplementedError):
        m.logits(torch.zeros(1, 3, 24, 64).cuda())
    with pytest.raises(ValueError):
        m.logits(torch.zeros(1, 1, 64, 64).cuda())
    with pytest.raises(Exception):
        m.logits(torch.zeros(1, 3, 64, 64))
    with pytest.raises(FileNotFoundError, match="no weights"):
        SegFormer(**MIT_B1).cuda().logits(torch.zeros(1, 3, 64, 64).cuda())
    assert m.logits(torch.zeros(1, 3, 576, 576).cuda()).shape == (1, 19, 144, 144)       # 18 x 18 = 324 keys: the largest square


def test_consistency_on_the_tower():
    from tests import segops_cases as S
    from uspace_amd.tools.seg_metrics import SegmentationConsistency, segmentation_consistency
    m = tower("seeded19")
    a, b = S.edit_pairs(3, 96, 160, 8)
    present = np.unique(m.labels(a.cuda()).cpu().numpy())
    region = [int(present[0])]
    out = segmentation_consistency(m, a.cuda(), b.cuda(), region=region)
    assert out["agreement"][0] == 1.0 and out["miou"][0] == 1.0 and out["outside_mse"][0] == 0.0
    assert np.all(out["agreement"][1:] < 1.0) and np.all(out["outside_share"] < 1.0) and out["iou"].shape == (3, 19)
    acc = SegmentationConsistency(m, region)
    acc.update(a.cuda(), b.cuda())
    assert acc.compute()["n"] == 3 and np.array_equal(acc.values["miou"], out["miou"])
