"""Inception Score, sFID and EvalSuite on the GPU: the one-pass entry point against the two existing calls bit for bit, the
spatial features and the logits against float64, the fp64 score statistics against the float64 reference of
tests/eval_suite_cases.py, the sFID path against numpy statistics, and EvalSuite against the single-metric tools.  All weights
are seeded (the pretrained file is not available here).

The bounds are tests/test_gpu_inception.py:TOL's (stage 2.5e-6, stats 1e-10, fid_path 1.6e-6), taken over unchanged; every test
prints what it measured before it asserts.  Measured on one MI355X: spatial features against float64 2.43e-6 (little room: the
whole path from the raw input held to one stage's bound; deterministic; 4.0e-7 for stage 14 alone), logits 1.2e-7 to 1.1e-6, split scores 1.3e-15 at the most,
spatial statistics 1.8e-16, sFID against numpy statistics 3.5e-11."""
import numpy as np
import pytest
import torch

from tests import eval_suite_cases as EC

pytestmark = pytest.mark.gpu
TOL = EC.TOL


def _images(n, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, 3, h, w, generator=g)


@pytest.fixture(scope="module")
def model():
    from uspace_amd.tools.inception import InceptionV3
    return InceptionV3([3], seed=0).cuda()


@pytest.fixture(scope="module")
def head():
    from uspace_amd.tools.inception import InceptionHead
    return InceptionHead(seed=1).cuda()


# ------------------------------------------------------------------------------------------------ 1. one pass
def _suite_raw(model, x, nan_fill):
    """The entry point itself on one chunk, with the workspace and both outputs filled with NaN first."""
    from uspace_amd import _hip
    B, _, H, W = x.shape
    ws = model._workspace(B, H, W, x.device)
    pool = torch.empty(B, 2048, dtype=torch.float32, device=x.device)
    sp = torch.empty(B, 2023, dtype=torch.float32, device=x.device)
    if nan_fill:
        ws.view(torch.float32).fill_(float("nan"))
        pool.fill_(float("nan"))
        sp.fill_(float("nan"))
    _hip.check(_hip.lib().uspace_inception_forward_suite(_hip.ptr(model._blob(x.device)), _hip.ptr(ws), ws.numel(), _hip.ptr(x), B, H,
                                                         W, _hip.ptr(pool), _hip.ptr(sp), 14, 7, _hip.stream_ptr()), "suite")
    return pool, sp


@pytest.mark.parametrize("size", [(137, 201), (299, 299)], ids=str)
def test_one_pass_equals_the_two_existing_calls_bit_for_bit(model, size):
    B = 5
    x = _images(B, size[0], size[1], seed=size[0]).cuda()
    want_pool = model.features(x, 3)
    want_sp = model.tap(x, 14)[..., :7].contiguous()
    pool, sp = model.suite(x, chunk=2)                              # ragged last chunk
    assert tuple(pool.shape) == (B, 2048) and tuple(sp.shape) == (B, 2023)
    assert torch.equal(pool, want_pool)
    assert torch.equal(sp.view(B, 17, 17, 7), want_sp)
    pool2, none = model.suite(x, spatial=False, chunk=2)
    assert none is None and torch.equal(pool2, want_pool)
    p3, s3 = _suite_raw(model, x[:2].contiguous(), nan_fill=True)
    assert torch.equal(p3, want_pool[:2]) and torch.equal(s3.view(2, 17, 17, 7), want_sp[:2])
    # the existing calls still give what they gave before the walk learnt to gather
    assert torch.equal(model.features(x, 3), want_pool) and torch.equal(model.tap(x, 14)[..., :7], want_sp)
    # other stages and widths follow the same rule
    _p, s15 = model.suite(x[:2], spatial_stage=15, spatial_channels=768)
    assert torch.equal(s15.view(2, 17, 17, 768), model.tap(x[:2], 15))


def test_suite_argument_errors(model):
    from uspace_amd._hip import UspaceHipError
    x = _images(1, 32, 32, seed=0).cuda()
    for stage, ch in ((0, 7), (19, 7), (14, 0), (14, 769)):
        with pytest.raises(UspaceHipError):
            model.suite(x, spatial_stage=stage, spatial_channels=ch)
        with pytest.raises(UspaceHipError):
            model.suite(x, spatial=False, spatial_stage=stage, spatial_channels=ch)
    with pytest.raises(UspaceHipError):
        model.suite(x.cpu())


# ------------------------------------------------------------------------------------------------ 2. spatial vs float64
def test_spatial_features_against_float64(model):
    from tests import inception_stages as S
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    x = _images(2, 137, 201, seed=3)
    ref = EC.ref_spatial(S.forward(sd, x.double(), last=14).numpy())
    _pool, sp = model.suite(x.cuda())
    err = EC.rel_l2(sp.cpu().numpy(), ref)
    # ... and as tests/test_gpu_inception.py measures a stage: against the restatement fed the GPU's own stage 13, which leaves
    # the error of stage 14 alone
    prev = model.tap(x.cuda(), 13).permute(0, 3, 1, 2).double().cpu()
    err_stage = EC.rel_l2(sp.cpu().numpy(), EC.ref_spatial(S.stage(sd, 14, prev).numpy()))
    print(f"spatial features vs float64: rel-L2 {err:.3e} from the raw input, {err_stage:.3e} from the GPU's stage 13")
    assert err_stage <= TOL["stage"], err_stage
    assert err <= TOL["stage"], err


# ------------------------------------------------------------------------------------------------ 3. logits
def _head_of(W, b):
    from uspace_amd.tools.inception import InceptionHead
    h = InceptionHead(num_classes=1, seed=0)
    h.load_state_dict({"fc.weight": torch.from_numpy(W), "fc.bias": torch.from_numpy(b)})
    return h.cuda()


@pytest.mark.parametrize("case", EC.LOGIT_CASES, ids=str)
def test_logits_against_float64(case):
    pool, W, b = EC.logit_operands(case)
    h = _head_of(W, b)
    xp = torch.from_numpy(pool).cuda()
    for bias in (True, False):
        got = h.logits(xp, bias=bias)
        assert tuple(got.shape) == (case[0], case[2]) and got.dtype == torch.float32
        err = EC.worst_row_rel_l2(got.cpu().numpy(), EC.ref_logits(pool, W, b if bias else None))
        print(f"{case} bias={bias}: worst per-row rel-L2 {err:.3e}")
        assert err <= TOL["stage"], (case, bias, err)
    assert torch.equal(h(xp), h.logits(xp, bias=True))


def test_logit_rows_do_not_depend_on_the_batch():
    case = EC.LOGIT_CASES[2]
    assert case[0] == 130
    pool, W, b = EC.logit_operands(case)
    h = _head_of(W, b)
    xp = torch.from_numpy(pool).cuda()
    full = h.logits(xp)
    for i in (0, 31, 32, 127, 128, 129):
        assert torch.equal(h.logits(xp[i:i + 1]), full[i:i + 1]), i
    assert torch.equal(h.logits(xp[100:107]), full[100:107])


def test_logits_reject_k_not_a_multiple_of_16():
    from uspace_amd import _hip
    with pytest.raises(_hip.UspaceHipError):
        _hip.inception_logits(torch.zeros(2, 24, device="cuda"), torch.zeros(5, 24, device="cuda"))
    with pytest.raises(_hip.UspaceHipError):
        _hip.inception_logits(torch.zeros(2, 16), torch.zeros(5, 16))            # a CPU tensor fails loudly


# ------------------------------------------------------------------------------------------------ 4. score statistics
def _check_scores(x, splits, what):
    from uspace_amd import _hip
    from uspace_amd.tools.inception_score import inception_score, split_scores
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    ref = EC.ref_split_scores(x, splits)
    got = split_scores(xd, splits)
    assert got.dtype == np.float64 and got.shape == (splits,) and np.isfinite(got).all()
    rel = float(np.abs(got / ref - 1).max())
    mean, std = inception_score(xd, splits)
    rmean, rstd = float(np.mean(ref)), float(np.std(ref))
    print(f"{what}: split scores rel {rel:.3e}, mean rel {abs(mean / rmean - 1):.3e}, std abs / mean {abs(std - rstd) / rmean:.3e}"
          f"  (IS {mean:.4f} +- {std:.4f})")
    assert rel <= TOL["stats"], (what, rel)
    assert abs(mean / rmean - 1) <= TOL["stats"], (what, mean, rmean)
    assert abs(std - rstd) / rmean <= TOL["stats"], (what, std, rstd)
    # bit-equal from run to run, and nothing of the workspace is read before it is written
    assert np.array_equal(split_scores(xd, splits), got)
    ws = torch.empty(_hip.lib().uspace_inception_score_workspace_bytes(x.shape[0], x.shape[1], splits), dtype=torch.uint8,
                     device="cuda")
    ws.view(torch.float64).fill_(float("nan"))
    assert np.array_equal(_hip.inception_score_splits(xd, splits, ws=ws).cpu().numpy(), got)


@pytest.mark.parametrize("case", EC.IS_CASES, ids=str)
def test_inception_score_against_float64(case):
    _check_scores(EC.logits_of(case), case[2], str(case))


def test_inception_score_with_zero_probabilities():
    x = EC.logits_of(EC.ZERO_CASE, True)
    _check_scores(x, EC.ZERO_CASE[2], "p = 0 and pbar = 0")


def test_inception_score_needs_a_row_per_split():
    from uspace_amd.tools.inception_score import inception_score
    with pytest.raises(ValueError):
        inception_score(torch.zeros(9, 40, device="cuda"), splits=10)


# ------------------------------------------------------------------------------------------------ 5. and 6. the paths
BATCH = 7


def _two_sets():
    a = _images(12, 64, 64, seed=21)
    g = torch.Generator().manual_seed(22)
    b = (0.6 + 0.15 * torch.randn(12, 3, 64, 64, generator=g)).clamp(0, 1)
    return a, b


def _batches(x):
    return [x[lo:lo + BATCH] for lo in range(0, len(x), BATCH)]


@pytest.fixture(scope="module")
def spatial_stats(model):
    """SpatialFIDStatistics of the two seeded sets (fed in batches of 7) and their sFID: shared by tests 5 and 6.  Every Frechet
    distance over 2023 or 2048 dimensions costs a host sqrtm of seconds, so each is computed once."""
    from uspace_amd.tools.fid_score import calculate_frechet_distance
    from uspace_amd.tools.sfid_score import SpatialFIDStatistics
    sts = []
    for x in _two_sets():
        st = SpatialFIDStatistics(device="cuda", model=model)
        for part in _batches(x):
            st.update(part)
        sts.append(st)
    sfid = calculate_frechet_distance(sts[1].mu, sts[1].sigma, sts[0].mu, sts[0].sigma)      # set 1 is the generated side
    return sts, float(sfid)


def test_sfid_path_against_numpy_statistics(model, spatial_stats, tmp_path):
    from uspace_amd.tools.fid_score import calculate_frechet_distance
    from uspace_amd.tools.sfid_score import calculate_sfid_given_paths
    sts, sfid = spatial_stats
    ref = []
    for st, x in zip(sts, _two_sets()):
        assert st.n == 12 and st.dims == 2023
        q = x.cuda().mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8).float() / 255      # what update(quantize=True) feeds
        _pool, sp = model.suite(q)
        a = sp.cpu().numpy().astype(np.float64)
        mu, sigma = a.mean(0), np.cov(a, rowvar=False)
        e_mu = np.linalg.norm(st.mu - mu) / np.linalg.norm(mu)
        e_sig = np.linalg.norm(st.sigma - sigma) / np.linalg.norm(sigma)
        print(f"spatial statistics vs numpy: mu {e_mu:.3e}, sigma {e_sig:.3e}")
        assert e_mu <= TOL["stats"] and e_sig <= TOL["stats"]
        ref.append((mu, sigma))
    want = float(calculate_frechet_distance(*ref[1], *ref[0]))
    print(f"sFID {sfid:.6f} vs numpy statistics {want:.6f}: rel {abs(sfid - want) / abs(want):.3e}")
    assert sfid > 0 and abs(sfid - want) / abs(want) <= TOL["fid_path"]
    # the .npz round trip gives the same value
    paths = []
    for k, st in enumerate(sts):
        paths.append(str(tmp_path / f"{k}.npz"))
        st.save(paths[-1])
        with np.load(paths[-1]) as f:
            assert sorted(f.keys()) == ["mu_s", "sigma_s"]
    assert calculate_sfid_given_paths((paths[1], paths[0]), device="cuda") == sfid


KID = dict(subsets=4, subset_size=8)


@pytest.fixture(scope="module")
def suites(model, head):
    """Per set (0 real, 1 generated): an EvalSuite and the four single tools fed the same images in batches of 7, and what
    ``fake.compute(real)`` gave: shared by the in-memory and the saved-file test, each of which pays for its own host sqrtm only."""
    from uspace_amd.tools.eval_suite import EvalSuite
    from uspace_amd.tools.feature_metrics import FeatureBank
    from uspace_amd.tools.fid_score import FIDStatistics
    from uspace_amd.tools.inception_score import InceptionScore
    res = dict(suite=[], fid=[], score=[], bank=[])
    for x in _two_sets():
        s = EvalSuite(device="cuda", model=model, head=head, bank=True)
        f = FIDStatistics(2048, device="cuda", model=model)
        i = InceptionScore(device="cuda", model=model, head=head)
        b = FeatureBank(2048, device="cuda", model=model)
        for part in _batches(x):
            for acc in (s, f, i, b):
                acc.update(part)
        assert s.n == 12 and len(i) == 12 and len(b) == 12
        for k, v in zip(("suite", "fid", "score", "bank"), (s, f, i, b)):
            res[k].append(v)
    res["out"] = res["suite"][1].compute(res["suite"][0], splits=3, kid=KID, nearest_k=3)
    return res


def test_eval_suite_equals_the_single_metric_tools(suites, spatial_stats):
    from uspace_amd.tools.feature_metrics import kid_score, prdc
    from uspace_amd.tools.fid_score import calculate_frechet_distance
    sts, sfid = spatial_stats
    ev, fids, scores, banks, out = (suites[k] for k in ("suite", "fid", "score", "bank", "out"))
    print({k: round(v, 6) for k, v in out.items()})
    assert sorted(out) == sorted(["fid", "sfid", "is_mean", "is_std", "kid_mean", "kid_std", "precision", "recall", "density",
                                  "coverage"])
    # the statistics are the single tools' bit for bit, and so are the numbers
    for k in (0, 1):
        assert np.array_equal(ev[k].fid.mu, fids[k].mu) and np.array_equal(ev[k].fid.sigma, fids[k].sigma)
        assert np.array_equal(ev[k].sfid.mu, sts[k].mu) and np.array_equal(ev[k].sfid.sigma, sts[k].sigma)
        assert torch.equal(ev[k].inception_score.logits, scores[k].logits)
        assert torch.equal(ev[k].bank.features, banks[k].features)
    # fid is the FIDStatistics.update path's number, sfid the very number test 5's objects gave
    assert out["fid"] == float(calculate_frechet_distance(fids[1].mu, fids[1].sigma, fids[0].mu, fids[0].sigma))
    assert out["fid"] > 0
    assert out["sfid"] == sfid
    assert (out["is_mean"], out["is_std"]) == scores[1].compute(splits=3)
    assert out["is_mean"] > 1.0 and out["is_std"] > 0.0
    assert (out["kid_mean"], out["kid_std"]) == kid_score(banks[1], banks[0], **KID)
    assert {k: out[k] for k in ("precision", "recall", "density", "coverage")} == prdc(banks[0], banks[1], nearest_k=3)


def test_eval_suite_against_a_saved_statistics_file(suites, tmp_path):
    """A saved statistics file stands in for the real side: no banks, so the two distances and the score, equal to the in-memory
    result."""
    real, fake = suites["suite"]
    p = str(tmp_path / "real.npz")
    real.save(p)
    with np.load(p) as f:
        assert sorted(f.keys()) == ["mu", "mu_s", "sigma", "sigma_s"]
    again = fake.compute(p, splits=3)
    assert sorted(again) == ["fid", "is_mean", "is_std", "sfid"]
    for k in again:
        assert again[k] == suites["out"][k], k


def test_eval_suite_reset(model, head):
    from uspace_amd.tools.eval_suite import EvalSuite
    s = EvalSuite(device="cuda", model=model, head=head, bank=True)
    s.update(_images(3, 32, 32, seed=1))
    assert s.n == 3 and len(s.inception_score) == 3 and len(s.bank) == 3 and s.sfid.n == 3
    s.reset()
    assert s.n == 0 and len(s.inception_score) == 0 and len(s.bank) == 0 and s.sfid.n == 0


def test_folder_paths_equal_the_in_memory_tools(model, head, tmp_path):
    """calculate_is_given_path, the spatial statistics of a folder and the four-array statistics file against the in-memory
    accumulators fed the same uint8 images in the same batches (no Frechet distance: the arrays decide it)."""
    import os
    from PIL import Image
    from uspace_amd.tools import sfid_score
    from uspace_amd.tools.fid_score import FIDStatistics
    from uspace_amd.tools.inception_score import InceptionScore, calculate_is_given_path
    rng = np.random.default_rng(5)
    imgs = rng.integers(0, 256, (9, 40, 48, 3), dtype=np.uint8)
    folder = str(tmp_path / "imgs")
    os.makedirs(folder)
    for i, a in enumerate(imgs):
        Image.fromarray(a).save(os.path.join(folder, f"{i}.png"))
    x = torch.from_numpy(imgs).permute(0, 3, 1, 2).float().cuda() / 255          # names 0 .. 8 sort as they are numbered
    acc, fid, sp = InceptionScore(device="cuda", model=model, head=head), FIDStatistics(2048, device="cuda", model=model), \
        sfid_score.SpatialFIDStatistics(device="cuda", model=model)
    for lo in range(0, 9, 4):
        for a in (acc, fid, sp):
            a.update(x[lo:lo + 4], quantize=False)
    got = calculate_is_given_path(folder, device="cuda", batch_size=4, num_workers=0, model=model, head=head, splits=3)
    assert got == acc.compute(splits=3)
    mu_s, sigma_s = sfid_score.compute_spatial_statistics_of_path(folder, model, 4, "cuda", 0)
    assert np.array_equal(mu_s, sp.mu) and np.array_equal(sigma_s, sp.sigma)
    out = str(tmp_path / "stats.npz")
    sfid_score.save_statistics_of_path(folder, out, device="cuda", batch_size=4, num_workers=0, model=model)
    with np.load(out) as f:
        assert sorted(f.keys()) == ["mu", "mu_s", "sigma", "sigma_s"]
        assert np.array_equal(f["mu"], fid.mu) and np.array_equal(f["sigma"], fid.sigma)
        assert np.array_equal(f["mu_s"], sp.mu) and np.array_equal(f["sigma_s"], sp.sigma)


def test_cpu_tensor_fails_loudly(model, head):
    from uspace_amd import _hip
    from uspace_amd.tools.eval_suite import EvalSuite
    from uspace_amd.tools.inception_score import inception_score
    with pytest.raises(_hip.UspaceHipError):
        model.suite(torch.rand(1, 3, 32, 32))
    with pytest.raises(_hip.UspaceHipError):
        head.logits(torch.rand(1, 2048))
    with pytest.raises(_hip.UspaceHipError):
        inception_score(torch.zeros(20, 40), splits=2)
    with pytest.raises(_hip.UspaceHipError):
        EvalSuite(device="cpu", model=model, head=head).update(torch.rand(1, 3, 32, 32))
