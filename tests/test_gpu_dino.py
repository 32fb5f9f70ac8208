"""The DINO towers and the structure distance on the GPU (uspace_amd/csrc/dino.hip) against the float64 restatement of
tests/dino_cases.py and the Hugging Face golden: both golden models stage by stage through the taps (native and interpolated
position table, with and without LayerScale), one shape at the ViT-L width, one long enough for the streaming attention kernel, the
structure kernel on its own at every tile count it distinguishes, bit-equality, and the two metrics end to end.

Bounds: ``C.TOL`` -- 3x what an MI355X measured, written beside each entry."""
import numpy as np
import pytest
import torch

from tests import clip_vision_cases as CV
from tests import dino_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def threads():
    n = CV.S.cpu_threads()
    yield
    torch.set_num_threads(n)


@pytest.fixture(scope="module")
def golden():
    return C.load_golden()


def _golden_module(model, side):
    from uspace_amd.libs.dino import DinoVisionTransformer
    m = DinoVisionTransformer(seed=0, **C.golden_module_config(model, side))
    m.load_state_dict(C.raw_golden_state_dict(model))
    return m.cuda()


def _stages(m, pv, sd, heads, eps):
    """Taps of the module against the tight model fed with the GPU's own previous tap -> (T, keys, pool, errors)."""
    nl = m.cfg["layers"]
    dev = pv.cuda()
    T = [m(dev, hidden_state=k).cpu() for k in range(nl + 1)]
    assert torch.equal(m(dev, hidden_state="embeddings").cpu(), T[0])
    upd, key_err = [], []
    for k in range(1, nl + 1):
        R, keys_ref, _q = C.layer(T[k - 1], sd, k - 1, "tight", heads, eps)
        upd.append(float((T[k].double() - R).norm() / (T[k].double() - T[k - 1].double()).norm()))
        key_err.append(C.rel(m.keys(dev, layer=k - 1).cpu().double(), keys_ref))
    pool = m(dev).cpu()
    keys = m.keys(dev).cpu()
    assert keys.dtype == torch.bfloat16 and tuple(keys.shape) == (pv.shape[0], m.tokens, m.cfg["dim"])
    assert torch.equal(m.keys(dev, layer=nl - 1).cpu(), keys)
    errs = dict(embeddings_tight=C.rel(T[0], C.embeddings(pv, sd, "tight")), update=max(upd), keys=max(key_err),
                pooler=C.rel(pool, C.pooled(T[nl], sd, eps)))
    # run to run: the same bits
    assert torch.equal(m(dev).cpu(), pool) and torch.equal(m(dev, hidden_state=nl).cpu(), T[nl]) and torch.equal(m.keys(dev).cpu(), keys)
    return T, keys, pool, errs


# ------------------------------------------------------------------------------------------------------------------ the tower
@pytest.mark.parametrize("run", list(C.GOLDEN_RUNS))
def test_tower_against_the_golden(threads, golden, run):
    from uspace_amd.tools.dino_metrics import self_similarity_mse
    z, sds = golden
    model, side = C.GOLDEN_RUNS[run]
    cfg = C.golden_module_config(model, side)
    m = _golden_module(model, side)
    pv = torch.from_numpy(z[f"{run}_pixel_values"])
    T, keys, pool, errs = _stages(m, pv, sds[model], cfg["num_attention_heads"], cfg["layer_norm_eps"])
    hs = z[f"{run}_hidden_states"]
    errs.update(embeddings=C.rel(T[0], z[f"{run}_embeddings"]), hidden=max(C.rel(T[k], hs[k]) for k in range(len(T))),
                pooler_e2e=C.rel(pool, z[f"{run}_pooler"]), keys_golden=C.rel(keys.double(), z[f"{run}_keys"]))
    pairs = z[f"{run}_pairs"]
    kd = keys.cuda()
    d = self_similarity_mse(kd[pairs[:, 0]], kd[pairs[:, 1]]).cpu().numpy()
    want = z[f"{run}_structure"]
    same = pairs[:, 0] == pairs[:, 1]
    errs["structure_e2e"] = float(np.max(np.abs(d[~same] - want[~same]) / want[~same]))
    print(f"tower {run}:", {n: "%.2e" % e for n, e in errs.items()})
    assert np.all(d[same] == 0.0)
    for n, e in errs.items():
        assert e < C.TOL[n], (n, e)


@pytest.mark.parametrize("name", list(C.SEEDED_CASES))
def test_tower_against_float64(threads, name):
    from uspace_amd import _hip
    from uspace_amd.libs.dino import DinoVisionTransformer
    cfg, _B = C.SEEDED_CASES[name]
    sd, pv = C.case_params(name), C.case_pixels(name)
    m = DinoVisionTransformer(seed=0, **cfg)
    m.load_state_dict(sd)
    m = m.cuda()
    heads, eps = cfg["num_attention_heads"], cfg["layer_norm_eps"]
    _hip.prof_all_begin()
    T, keys, pool, errs = _stages(m, pv, sd, heads, eps)
    recs = [r for r in _hip.prof_all_end() if r["kind"] == 1]
    # which attention kernel ran: the recorder's flag 2 marks the streaming form
    assert recs and all(r["N"] == m.tokens for r in recs)
    assert all(bool(r["flags"] & 2) == (m.tokens > 336) for r in recs), recs
    ref = C.tower_forward(pv, sd, heads, "loose", eps)
    errs.update(embeddings=C.rel(T[0], ref["embeddings"]), hidden=max(C.rel(T[k], ref["hidden"][k]) for k in range(len(T))),
                pooler_e2e=C.rel(pool, ref["pooler"]), keys_golden=C.rel(keys.double(), ref["last_keys"]))
    print(f"tower {name}:", {n: "%.2e" % e for n, e in errs.items()})
    for n, e in errs.items():
        assert e < C.TOL[n], (n, e)


def test_forward_refuses_what_it_cannot_do():
    m = _golden_module("dinov2", 42)
    pv = torch.zeros(1, 3, 42, 42, device="cuda")
    with pytest.raises(ValueError):
        m(torch.zeros(1, 3, 70, 70, device="cuda"))
    with pytest.raises(ValueError):
        m.keys(pv, layer=3)
    with pytest.raises(Exception):
        m(pv.cpu())
    assert tuple(m(pv[:0]).shape) == (0, 128) and tuple(m.keys(pv[:0]).shape) == (0, 10, 128)


# ------------------------------------------------------------------------------------------------------------------ the structure kernel
@pytest.mark.parametrize("B", C.STRUCTURE_B)
@pytest.mark.parametrize("D", C.STRUCTURE_D)
@pytest.mark.parametrize("T", C.STRUCTURE_T)
def test_structure_kernel_against_float64(threads, T, D, B):
    from uspace_amd.tools.dino_metrics import self_similarity_mse
    worst = {}
    for data in C.STRUCTURE_DATA:
        a, b = C.structure_keys(T, D, B, data)
        got = self_similarity_mse(a.cuda(), b.cuda()).cpu().numpy()
        ref = C.structure(a, b).numpy()
        assert got.shape == (B,) and np.all(np.isfinite(got))
        if data == "identical":
            assert np.all(got == 0.0), got
            continue
        if T == 1:            # one token: S = [[1]] on both sides up to the fp32 rounding of a unit cosine, (2^-22)^2 = 6e-14 squared
            assert np.all(ref < 1e-30) and np.all(got <= 1e-12), (data, got, ref)
            continue
        worst[data] = float(np.max(np.abs(got - ref) / ref))
    print(f"structure T={T} D={D} B={B}:", {n: "%.2e" % e for n, e in worst.items()})
    for data, e in worst.items():
        assert e < C.TOL["structure_near" if data == "near" else "structure"], (data, e)


def test_structure_kernel_bits_do_not_depend_on_batch_workspace_or_strides():
    from uspace_amd import _hip
    from uspace_amd.tools.dino_metrics import self_similarity_mse
    for T, D in ((17, 64), (257, 384), (785, 64)):
        a, b = (t.cuda() for t in C.structure_keys(T, D, 3, "random", seed=1))
        full = self_similarity_mse(a, b)
        assert torch.equal(self_similarity_mse(a, b), full)                                     # run to run
        for p in range(3):                                                                      # alone, and at another position
            assert torch.equal(self_similarity_mse(a[p:p + 1], b[p:p + 1])[0], full[p])
        perm = [2, 0, 1]
        assert torch.equal(self_similarity_mse(a[perm], b[perm]), full[perm])
        assert torch.equal(torch.cat([self_similarity_mse(a[:2], b[:2]), self_similarity_mse(a[2:], b[2:])]), full)   # chunks
        ws = torch.full((_hip.lib().uspace_self_similarity_mse_workspace_bytes(3, T),), 0xFF, dtype=torch.uint8, device="cuda")
        assert torch.equal(self_similarity_mse(a, b, ws=ws), full)                              # NaN-filled workspace
        # keys inside a q|k|v buffer: row stride 3 D
        qa, qb = (torch.randn(3, T, 3 * D, device="cuda").to(torch.bfloat16) for _ in range(2))
        qa[:, :, D:2 * D], qb[:, :, D:2 * D] = a, b
        assert torch.equal(self_similarity_mse(qa[:, :, D:2 * D], qb[:, :, D:2 * D]), full)
        assert torch.all(self_similarity_mse(a, a) == 0.0)


def test_structure_kernel_refuses_bad_arguments():
    from uspace_amd import _hip
    from uspace_amd.tools.dino_metrics import self_similarity_mse
    a = torch.zeros(1, 4, 96, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(_hip.UspaceHipError):
        self_similarity_mse(a, a)                        # D % 64
    with pytest.raises(_hip.UspaceHipError):
        self_similarity_mse(a.float(), a.float())
    with pytest.raises(_hip.UspaceHipError):
        self_similarity_mse(a, a[:, :2])


# ------------------------------------------------------------------------------------------------------------------ end to end
def test_structure_distance_and_fd_dino_end_to_end(threads, golden, tmp_path):
    from uspace_amd.libs.dino import IMAGENET_MEAN, IMAGENET_STD
    from uspace_amd.tools.dino_metrics import DinoFeatures, FDDino, fd, structure_distance
    from uspace_amd.tools.lpips import LPIPS
    from uspace_amd.tools.pair_metrics import PairMetrics
    _z, sds = golden
    sd = sds["dinov2"]
    m = _golden_module("dinov2", 42)
    g = torch.Generator().manual_seed(11)
    a = torch.rand(5, 3, 64, 64, generator=g)
    b = (a + 0.15 * torch.randn(5, 3, 64, 64, generator=g)).clamp(0, 1)
    b[4] = a[4]

    def model_keys(x):
        pv = CV.preprocess(x, 42, True, IMAGENET_MEAN, IMAGENET_STD)
        return C.tower_forward(pv, sd, 2, "loose")["last_keys"]
    ref = C.structure(model_keys(a), model_keys(b)).numpy()
    got = structure_distance(m, a.cuda(), b.cuda()).cpu().numpy()
    e_struct = float(np.max(np.abs(got[:4] - ref[:4]) / ref[:4]))
    assert got[4] == 0.0 and ref[4] == 0.0
    assert np.array_equal(structure_distance(m, a.cuda(), b.cuda(), chunk=2).cpu().numpy(), got)
    pm = PairMetrics(device="cuda", lpips=LPIPS("alex", seed=0).cuda(), structure=m)
    pm.update(a[:3], b[:3])
    pm.update(a[3:], b[3:])
    assert np.array_equal(pm.values["structure"], got) and abs(pm.compute()["structure"] - got.mean()) < 1e-15

    # FD: two sets of 160 small images (more samples than the 128 feature dimensions)
    xs = [torch.rand(160, 3, 32, 32, generator=g) * s + o for s, o in ((1.0, 0.0), (0.7, 0.2))]
    feats_ref = [C.tower_forward(CV.preprocess(x, 42, True, IMAGENET_MEAN, IMAGENET_STD), sd, 2, "loose")["pooler"].numpy() for x in xs]
    want = fd(*feats_ref)
    f = FDDino(m, device="cuda", chunk=64)
    f.update_real(xs[0][:100])
    f.update_real(xs[0][100:])
    f.update(xs[1])
    got_fd = f.compute()
    feats = [DinoFeatures(m, 64).features(x.cuda()).cpu().numpy() for x in xs]
    e_feat = max(C.rel(torch.from_numpy(p), torch.from_numpy(q)) for p, q in zip(feats, feats_ref))
    assert abs(got_fd - fd(feats[1], feats[0])) <= 1e-8 * abs(got_fd)          # the accumulated statistics = numpy's on the same features
    f.save(tmp_path / "real.npz")
    f2 = FDDino(m, device="cuda")
    f2.load(tmp_path / "real.npz")
    f2.update(xs[1])
    assert f2.compute() == got_fd
    e_fd = abs(got_fd - want) / want
    print(f"end to end: structure {e_struct:.2e} (values {got}), features {e_feat:.2e}, fd {e_fd:.2e} (value {got_fd:.4f})")
    assert e_struct < C.TOL["structure_e2e"] and e_feat < C.TOL["pooler_e2e"] and e_fd < C.TOL["fd"]
