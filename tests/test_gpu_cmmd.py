"""GPU checks of the RBF-kernel MMD and CMMD (uspace_metric_rbf_sums of uspace_amd/csrc/metrics.hip, uspace_amd/tools/cmmd.py)
against the float64 reference, cases and bounds of tests/cmmd_cases.py."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import clip_vision_cases as V
from tests import cmmd_cases as C

pytestmark = pytest.mark.gpu

GAMMA = 1.0 / (2.0 * C.SIGMA * C.SIGMA)
RUNS = [(case, nz) for case in C.CASES for nz in C.NORMALIZE]
_ids = lambda v: str(v).replace(" ", "")


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()                # (a copy: the cached cases are read-only)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.cpu().view(torch.int64), b.cpu().view(torch.int64))


@functools.lru_cache(maxsize=None)
def _gpu_sums(case, normalize):
    from uspace_amd import _hip
    x, y = C.sets_of(case)
    return _hip.metric_rbf_sums(_dev(x), _dev(y), GAMMA, normalize=bool(normalize))


# ------------------------------------------------------------------------------------------- sums and scores
@pytest.mark.parametrize("case,normalize", RUNS, ids=_ids)
def test_sums_and_scores(case, normalize):
    from uspace_amd.tools.cmmd import cmmd_score, rbf_mmd2
    x, y = C.sets_of(case)
    ref = C.ref_of(case, normalize)
    got = _gpu_sums(case, normalize)
    assert got.dtype == torch.float64 and got.shape == (3,) and got.is_cuda
    got = got.cpu().numpy()
    err = np.abs(got - ref["sums"])
    ratios = [float(e / b) if b > 0 else 0.0 for e, b in zip(err, ref["sum_bounds"])]
    v = C.SCALE * rbf_mmd2(_dev(x), _dev(y), C.SIGMA, normalize=bool(normalize))
    line = (f"case {case} normalize {normalize}: smallest K {ref['kmin']:.3g}; sums / bound {['%.2e' % r for r in ratios]}; "
            f"V score {v:.9g} (ref {ref['score']:.9g}), error / bound {abs(v - ref['score']) / ref['bound']:.2e}")
    if min(case[1], case[2]) >= 2:
        ru = C.ref_of(case, normalize, True)
        u = C.SCALE * rbf_mmd2(_dev(x), _dev(y), C.SIGMA, normalize=bool(normalize), unbiased=True)
        line += f"; U score {u:.9g}, error / bound {abs(u - ru['score']) / ru['bound']:.2e}"
    print(line)
    assert np.isfinite(got).all() and np.all(err <= ref["sum_bounds"]), (got, ref["sums"], ref["sum_bounds"])
    assert abs(v - ref["score"]) <= ref["bound"]
    if min(case[1], case[2]) >= 2:
        assert abs(u - ru["score"]) <= ru["bound"]
    else:
        assert got[0] == 0.0                                   # a one-row set: no off-diagonal pair, exactly
        with pytest.raises(ValueError):
            rbf_mmd2(_dev(x), _dev(y), C.SIGMA, normalize=bool(normalize), unbiased=True)
    if normalize:
        assert cmmd_score(_dev(y), _dev(x)) == pytest.approx(ref["score"], abs=ref["bound"])     # (fake, real): V is symmetric


@pytest.mark.parametrize("case,normalize", [(c, nz) for c in C.CASES[:4] for nz in C.NORMALIZE], ids=_ids)
def test_a_set_against_itself(case, normalize):
    from uspace_amd.tools.cmmd import rbf_mmd2
    x, _ = C.sets_of(case)
    rv = C.ref_score(x, x, C.SIGMA, bool(normalize), unbiased=False)
    ru = C.ref_score(x, x, C.SIGMA, bool(normalize), unbiased=True)
    v = C.SCALE * rbf_mmd2(_dev(x), _dev(x), C.SIGMA, normalize=bool(normalize))
    u = C.SCALE * rbf_mmd2(_dev(x), _dev(x), C.SIGMA, normalize=bool(normalize), unbiased=True)
    print(f"case {case} normalize {normalize}: V {v:.3e} (bound {rv['bound']:.3e}), U {u:.6g} (ref {ru['score']:.6g}, bound {ru['bound']:.3e})")
    assert abs(v) <= rv["bound"]
    assert u <= ru["bound"] and abs(u - ru["score"]) <= ru["bound"]


# ------------------------------------------------------------------------------------------- bits
@pytest.mark.parametrize("case,normalize", RUNS, ids=_ids)
def test_bits(case, normalize):
    """Run to run, on a workspace of 0xFF bytes, and with the sets swapped: Sxx <-> Syy bit for bit, Sxy within its bound (its
    summation order changes with the roles of rows and columns)."""
    from uspace_amd import _hip
    x, y = (_dev(a) for a in C.sets_of(case))
    first = _gpu_sums(case, normalize)
    assert _same_bits(first, _hip.metric_rbf_sums(x, y, GAMMA, normalize=bool(normalize)))
    ws = _hip.metric_workspace(len(x), len(y), 1, max(len(x), len(y)), device=x.device, fill=0xFF)
    assert _same_bits(first, _hip.metric_rbf_sums(x, y, GAMMA, normalize=bool(normalize), ws=ws))
    swapped = _hip.metric_rbf_sums(y, x, GAMMA, normalize=bool(normalize))
    assert _same_bits(first[0:1], swapped[1:2]) and _same_bits(first[1:2], swapped[0:1])
    assert abs(float(first[2]) - float(swapped[2])) <= C.ref_of(case, normalize)["sum_bounds"][2]


@pytest.mark.parametrize("normalize", C.NORMALIZE)
def test_batch_independence(normalize):
    """Rows appended to y, far away, leave Sxx's bits alone: also where they add row blocks to the launch (129 rows of x, 257 -> 400
    of y), whose partial sums for the x pair are zeros."""
    from uspace_amd import _hip
    case = C.CASES[0]
    x, y = C.sets_of(case)
    far = np.concatenate([y, (y[:143] + 1000.0).astype(np.float32)])
    more = _hip.metric_rbf_sums(_dev(x), _dev(far), GAMMA, normalize=bool(normalize))
    assert _same_bits(_gpu_sums(case, normalize)[0:1], more[0:1])
    fewer = _hip.metric_rbf_sums(_dev(x), _dev(y[:5]), GAMMA, normalize=bool(normalize))
    assert _same_bits(_gpu_sums(case, normalize)[0:1], fewer[0:1])


def test_wrapper_errors():
    from uspace_amd import _hip
    x = torch.zeros(17, 64, device="cuda")
    with pytest.raises(_hip.UspaceHipError):
        _hip.metric_rbf_sums(x, x[:, :32].contiguous(), GAMMA)
    with pytest.raises(_hip.UspaceHipError):
        _hip.metric_rbf_sums(x, x[:, ::2], GAMMA)                       # not contiguous
    with pytest.raises(_hip.UspaceHipError):
        _hip.metric_rbf_sums(x.double(), x.double(), GAMMA)
    with pytest.raises(_hip.UspaceHipError):
        _hip.metric_rbf_sums(x, x, -1.0)
    with pytest.raises(_hip.UspaceHipError):
        _hip.metric_rbf_sums(x, x, GAMMA, ws=torch.empty(8, dtype=torch.uint8, device="cuda"))
    # zero rows under normalisation count as the zero vector: D2 = 0 between two of them, 1 against a unit vector
    y = torch.zeros(3, 64, device="cuda")
    y[2, 5] = 7.0
    s = _hip.metric_rbf_sums(y, y, 0.5, normalize=True).cpu().numpy()
    k = float(np.exp(-0.5))
    assert np.allclose(s, [2.0 + 4.0 * k, 2.0 + 4.0 * k, 5.0 + 4.0 * k], rtol=1e-14, atol=0)


# ------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def rig():
    from uspace_amd.libs.clip import CLIPVisionTransformer
    from uspace_amd.tools.cmmd import CMMD
    vision = CLIPVisionTransformer(**V.TINY_VISION)
    vision.load_state_dict(V.vision_params("workflow", seed=41, **V.TINY_VISION))
    fake, real = V.make_images(12, 64, seed=21, kind="mixed").cuda(), V.make_images(9, 64, seed=22, kind="mixed").cuda()
    metric = CMMD(vision, device="cuda")
    metric.update(fake)
    metric.update_real(real)
    return dict(vision=metric.vision, metric=metric, fake=fake, real=real, score=metric.compute())


def test_end_to_end_from_images(rig):
    from uspace_amd.tools.cmmd import CMMD, cmmd_score
    vision, metric = rig["vision"], rig["metric"]
    e_fake, e_real = (vision(vision.preprocess(rig[k])) for k in ("fake", "real"))
    assert len(metric.fake) == 12 and len(metric.real) == 9 and e_fake.shape == (12, V.TINY_VISION["projection_dim"])
    assert torch.equal(metric.fake.features, e_fake) and torch.equal(metric.real.features, e_real)      # banked unnormalised
    assert rig["score"] == cmmd_score(e_fake, e_real)
    ref = C.ref_score(e_fake.cpu().numpy(), e_real.cpu().numpy())
    print(f"CMMD of 12 + 9 images through the tiny tower: {rig['score']:.9g} (float64 reference on the same embeddings {ref['score']:.9g}, "
          f"error / bound {abs(rig['score'] - ref['score']) / ref['bound']:.2e})")
    assert abs(rig["score"] - ref["score"]) <= ref["bound"] and rig["score"] > 0
    chunked = CMMD(vision, device="cuda", chunk=5)
    chunked.update(rig["fake"])
    chunked.update_real(rig["real"][:4])
    chunked.update_real(rig["real"][4:])
    assert torch.equal(chunked.fake.features, e_fake) and chunked.compute() == rig["score"]
    other = CMMD(vision, device="cuda")
    other.update_features(e_fake)
    other.update_features(e_real, real=True)
    assert other.compute() == rig["score"]


def test_end_to_end_from_folders(rig, tmp_path):
    from uspace_amd.tools.cmmd import calculate_cmmd_given_paths
    from uspace_amd.tools.utils_uvit import save_image
    for name in ("real", "fake"):
        os.makedirs(tmp_path / name)
        for i, img in enumerate(rig[name]):
            save_image(img, str(tmp_path / name / f"{i:02d}.png"))
    paths = (str(tmp_path / "real"), str(tmp_path / "fake"))
    assert calculate_cmmd_given_paths(paths, rig["vision"], device="cuda", batch_size=5) == rig["score"]
    bank = str(tmp_path / "real.npz")
    rig["metric"].save(bank)
    assert calculate_cmmd_given_paths((bank, paths[1]), rig["vision"], device="cuda") == rig["score"]
    rig["metric"].fake.save(str(tmp_path / "fake.npz"))
    assert calculate_cmmd_given_paths((paths[0], str(tmp_path / "fake.npz")), rig["vision"], device="cuda") == rig["score"]
    assert calculate_cmmd_given_paths((bank, str(tmp_path / "fake.npz")), None, device="cuda") == rig["score"]


def test_577_token_tower_through_cmmd():
    """One forward of a two-layer tower at image_size 336, patch 14 (the streaming attention kernel's length): finite embeddings of the
    right shape through CMMD.  The tower's numerics at that length are the business of tests/test_gpu_clip_vision.py."""
    from uspace_amd.libs.clip import CLIPVisionTransformer
    from uspace_amd.tools.cmmd import CMMD
    cfg = dict(V.TINY_VISION, image_size=336)
    vision = CLIPVisionTransformer(**cfg)
    vision.load_state_dict(V.vision_params("workflow", seed=43, **cfg))
    assert vision.tokens == 577
    metric = CMMD(vision, device="cuda")
    metric.update(V.make_images(2, 256, seed=23, kind="mixed").cuda())
    feat = metric.fake.features
    assert feat.shape == (2, cfg["projection_dim"]) and feat.dtype == torch.float32 and bool(torch.isfinite(feat).all())
    assert float(feat.norm(dim=1).min()) > 0 and not torch.equal(feat[0], feat[1])
