"""The ArcFace identity tower and the ID similarity (csrc/idnet.hip, libs/arcface.py, tools/id_metrics.py) on the GPU against the
float64 restatement of tests/arcface_stages.py: the preprocess, single units at the sizes that reach every branch, the towers
stage by stage, whole towers, bit-identity across batch sizes and positions, the metric's entry points and the refusals.  Every
figure is printed before it is judged; the bounds are ``arcface_stages.TOL``."""
import ctypes

import numpy as np
import pytest
import torch

from tests import arcface_stages as R

pytestmark = pytest.mark.gpu

_TOWERS = {}


def tower(name):
    """Seeded towers, built once: tiny32 / tiny48 / tiny112 (one unit per level), lowvar32 (tiny32 with small batch norm variances),
    units (UNIT_BLOCKS), ir_se50, ir100."""
    if name not in _TOWERS:
        from uspace_amd.libs.arcface import Backbone
        if name == "lowvar32":
            m = Backbone(input_size=32, blocks=R.TINY)
            m.load_state_dict(R.low_variance(tower("tiny32")[1]))
        elif name.startswith("tiny"):
            m = Backbone(input_size=int(name[4:]), blocks=R.TINY, seed=5)
        elif name == "units":
            m = Backbone(input_size=32, blocks=R.UNIT_BLOCKS, seed=6)
        elif name == "ir_se50":
            m = Backbone(seed=0)
        else:
            m = Backbone(num_layers=100, seed=1)
        sd = {k: v.detach().clone() for k, v in m.state_dict().items()}      # the restatement's copy stays on the host
        _TOWERS[name] = (m.cuda(), sd)
    return _TOWERS[name]


def report(what, case, value, bound):
    value = float(value)
    print(f"ID-MEASURE {what} {case}: {value:.3e} (bound {bound:.1e})")
    return value


def signed_images(n, size, seed):
    """Aligned inputs of the tower: smooth images in [-1, 1], NCHW fp32."""
    return R.smooth_images(n, size, size, seed) * 2 - 1


# ----------------------------------------------------------------------------------------------------------- preprocess
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("B,H,W,crop", R.PREPROCESS_CASES)
def test_preprocess(B, H, W, crop, normalize):
    m, _ = tower("tiny112")
    x = R.smooth_images(B, H, W, 21)
    if not normalize:
        x = x * 2 - 1
    got = R.nchw(m.preprocess(x.cuda(), normalize=normalize, crop=crop).cpu())
    want = R.preprocess(x, normalize, crop, 112)
    assert got.shape == want.shape == (B, 3, 112, 112)
    worst = report("preprocess", (B, H, W, crop, normalize), R.rel_l2(got, want).max(), R.TOL["preprocess"])
    assert worst <= R.TOL["preprocess"]


# ---------------------------------------------------------------------------------------------------------------- units
def _judge_unit(got, want, case):
    inner, border = R.rel_l2_split(got, want)
    wi = report("unit_interior", case, inner.max(), R.TOL["unit_interior"])
    wb = report("unit_border", case, border.max(), R.TOL["unit_border"])
    assert wi <= R.TOL["unit_interior"] and wb <= R.TOL["unit_border"]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("index,size", R.UNIT_CASES)
def test_single_unit(index, size, B):
    """One unit alone (``uspace_idnet_unit``) on maps no valid input size reaches: odd sides, a stride-1 unit at 5 x 5."""
    m, sd = tower("units")
    cin, depth, stride = R.unit_specs(R.UNIT_BLOCKS)[index]
    x = R.unit_input(B, size[0], size[1], cin, 31 + index)
    got = R.nchw(m.unit(index, R.nhwc(x).cuda()).cpu())
    want = R.unit(sd, f"body.{index}", x.double(), cin, depth, stride, True)
    assert got.shape == want.shape
    _judge_unit(got, want, ((cin, depth, stride), size, B))


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name,size", [(f"tiny{s}", s) for s in R.TINY_SIZES] + [("lowvar32", 32)])
def test_tiny_tower_stage_by_stage(name, size, B):
    """blocks (1, 1, 1, 1) through ``uspace_idnet_tap``: every stage from the GPU's own previous stage; the last stage is the head
    alone (512 x 2 x 2 at 32, 512 x 7 x 7 at 112).  lowvar32: batch norm variances near eps, where a wrong eps would show."""
    m, sd = tower(name)
    x = signed_images(B, size, 41)
    prev = x.double()
    for s in range(6):
        got = m.tap(x.cuda(), s).cpu()
        got = R.nchw(got) if got.dim() == 4 else got
        want = R.stage(sd, R.TINY, True, s, prev)
        assert got.shape == want.shape
        if s == 0 or s == 5:
            key = "input_layer" if s == 0 else "head"
            worst = report(key, (name, B), R.rel_l2(got, want).max(), R.TOL[key])
            assert worst <= R.TOL[key]
        else:
            _judge_unit(got, want, (name, B, s))
        prev = got.double()


def test_mode_ir_stage_by_stage():
    """mode "ir": no SE module, out = res + shortcut."""
    from uspace_amd.libs.arcface import Backbone
    m = Backbone(input_size=32, mode="ir", blocks=R.TINY, seed=9)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m = m.cuda()
    x = signed_images(2, 32, 43)
    prev = R.nchw(m.tap(x.cuda(), 0).cpu()).double()
    for s in range(1, 5):
        got = R.nchw(m.tap(x.cuda(), s).cpu())
        _judge_unit(got, R.stage(sd, R.TINY, False, s, prev), ("ir", 32, 2, s))
        prev = got.double()


# --------------------------------------------------------------------------------------------------------------- towers
def _judge_tower(case, ea, eb, sim, want_sim, want_a, want_b):
    we = report("embedding", case, torch.cat([R.rel_l2(ea, want_a), R.rel_l2(eb, want_b)]).max(), R.TOL["embedding"])
    ws = report("similarity", case, (sim.double() - want_sim).abs().max(), R.TOL["similarity"])
    assert we <= R.TOL["embedding"] and ws <= R.TOL["similarity"]


@pytest.mark.parametrize("name,size,B", [("tiny32", 32, 3), ("lowvar32", 32, 3), ("ir_se50", 112, 2), ("ir100", 112, 1)])
def test_whole_tower(name, size, B):
    from uspace_amd.libs.arcface import similarity
    m, sd = tower(name)
    a = signed_images(B, size, 51)
    b = (a + 0.3 * signed_images(B, size, 52)).clamp(-1, 1)
    ea, eb = m(a.cuda()), m(b.cuda())
    assert ea.shape == (B, 512) and ea.dtype == torch.float32
    sim = similarity(ea, eb).cpu()
    want_a, want_b = R.embed(sd, m.blocks, True, a), R.embed(sd, m.blocks, True, b)
    _judge_tower((name, size, B), ea.cpu(), eb.cpu(), sim, (want_a * want_b).sum(1), want_a, want_b)
    assert float((ea.double().norm(dim=1) - 1).abs().max()) < 1e-6


def test_ir_se50_through_the_preprocess():
    """The metric as pSp / e4e compute it: 256 x 256 images in [0, 1] -> crop -> pool -> IR-SE50 -> dot product."""
    from uspace_amd.tools.id_metrics import IDSimilarity
    m, sd = tower("ir_se50")
    a = R.smooth_images(2, 256, 256, 61)
    b = R.perturbed(a, 0.3, 62)
    metric = IDSimilarity(m)
    sim = metric(a.cuda(), b.cuda(), quantize=False).cpu()
    ea, eb = metric.features(a.cuda(), quantize=False).cpu(), metric.features(b.cuda(), quantize=False).cpu()
    want_sim, want_a, want_b = R.id_similarity(sd, m.blocks, True, a, b)
    assert sim.dtype == torch.float64
    _judge_tower(("ir_se50", "256 -> 112", 2), ea, eb, sim, want_sim, want_a, want_b)


# --------------------------------------------------------------------------------------------------------- bit-identity
@pytest.mark.parametrize("name,size", [("tiny112", 112), ("ir_se50", 112)])
def test_bit_identical_across_batch_and_position(name, size):
    from uspace_amd.libs.arcface import similarity
    m, _ = tower(name)
    x = signed_images(5, size, 71).cuda()
    y = (x + 0.2 * signed_images(5, size, 72).cuda()).clamp(-1, 1)
    ex, ey = m(x), m(y)
    assert torch.equal(ex, m(x)) and torch.equal(ey, m(y, chunk=2))
    sims = similarity(ex, ey)
    for pos in (0, 2, 4):
        e1, f1 = m(x[pos:pos + 1]), m(y[pos:pos + 1])
        assert torch.equal(e1[0], ex[pos]) and torch.equal(f1[0], ey[pos]), pos
        assert torch.equal(similarity(e1, f1)[0], sims[pos]), pos
    assert torch.equal(sims, similarity(ex, ey))


# ------------------------------------------------------------------------------------------------- the metric's surface
def test_pair_metrics_identity_and_folders(tmp_path):
    from PIL import Image
    from uspace_amd.tools.id_metrics import calculate_id_similarity_given_paths
    from uspace_amd.tools.lpips import LPIPS
    from uspace_amd.tools.pair_metrics import PairMetrics
    m, sd = tower("tiny32")
    a = R.smooth_images(4, 96, 96, 81)
    b = R.perturbed(a, 0.3, 82)
    qa, qb = ((t * 255 + 0.5).clamp(0, 255).to(torch.uint8) for t in (a, b))
    for d, q in (("a", qa), ("b", qb)):
        (tmp_path / d).mkdir()
        for i in range(4):
            Image.fromarray(q[i].permute(1, 2, 0).numpy()).save(tmp_path / d / f"{i:03d}.png")
    want, _, _ = R.id_similarity(sd, m.blocks, True, qa.float() / 255, qb.float() / 255, input_size=32)
    out = calculate_id_similarity_given_paths(tmp_path / "a", tmp_path / "b", m, device="cuda", batch_size=3)
    assert out["n"] == 4 and out["values"].dtype == np.float64
    w1 = report("similarity", "folders, tiny32 from 96 x 96", np.abs(out["values"] - want.numpy()).max(), R.TOL["similarity"])
    assert w1 <= R.TOL["similarity"] and out["identity"] == float(np.mean(out["values"]))

    lp = LPIPS("alex", seed=3).cuda()
    plain, with_id = PairMetrics(device="cuda", lpips=lp), PairMetrics(device="cuda", lpips=lp, identity=m)
    for pm in (plain, with_id):
        pm.update(a[:3], b[:3])
        pm.update(a[3:], b[3:])
    v0, v1 = plain.values, with_id.values
    assert set(v0) == {"lpips", "ssim", "psnr"} and set(v1) == set(v0) | {"identity"}
    for k in v0:
        assert np.array_equal(v0[k], v1[k]), k
    assert np.array_equal(v1["identity"], out["values"])      # the written PNGs hold the quantised numbers
    res = with_id.compute()
    assert res["n"] == 4 and res["identity"] == float(np.mean(v1["identity"])) and "identity" not in plain.compute()

    (tmp_path / "b" / "extra.png").write_bytes((tmp_path / "b" / "000.png").read_bytes())
    with pytest.raises(ValueError, match="pair up"):
        calculate_id_similarity_given_paths(tmp_path / "a", tmp_path / "b", m, device="cuda")


def test_missing_weights_are_named_at_first_use():
    from uspace_amd.libs.arcface import Backbone
    m = Backbone(input_size=32, blocks=R.TINY).cuda()
    with pytest.raises(FileNotFoundError, match="weights="):
        m(torch.zeros(1, 3, 32, 32, device="cuda"))
    m.load_state_dict(tower("tiny32")[1])
    x = signed_images(1, 32, 91).cuda()
    assert torch.equal(m(x), tower("tiny32")[0](x))


# ------------------------------------------------------------------------------------------------------------ refusals
def test_argument_refusals():
    from uspace_amd import _hip
    from uspace_amd.libs.arcface import similarity
    L = _hip.lib()
    m, _ = tower("tiny32")
    cfg = m.cfg
    ERR_ARG, ERR_WS = -1, -3
    for bad in (_hip.IdnetConfig(100, (ctypes.c_int * 4)(1, 1, 1, 1), 1), _hip.IdnetConfig(0, (ctypes.c_int * 4)(1, 1, 1, 1), 1),
                _hip.IdnetConfig(32, (ctypes.c_int * 4)(1, 0, 1, 1), 1), _hip.IdnetConfig(32, (ctypes.c_int * 4)(1, 1, 1, 1), 2)):
        r = ctypes.byref(bad)
        assert L.uspace_idnet_num_params(r) == ERR_ARG and L.uspace_idnet_param_numel(r, 0) == -1
        assert L.uspace_idnet_weight_bytes(r) == 0 and L.uspace_idnet_workspace_bytes(r, 1) == 0
        assert L.uspace_idnet_unit_workspace_bytes(r, 0, 1, 8, 8) == 0
    r = ctypes.byref(cfg)
    n = L.uspace_idnet_num_params(r)
    assert L.uspace_idnet_param_numel(r, n) == -1 and L.uspace_idnet_param_numel(r, -1) == -1
    assert L.uspace_idnet_workspace_bytes(r, 0) == 0 and L.uspace_idnet_workspace_bytes(r, 40000) == 0
    assert L.uspace_idnet_unit_workspace_bytes(r, 4, 1, 8, 8) == 0 and L.uspace_idnet_unit_workspace_bytes(r, 0, 1, 0, 8) == 0
    dev = torch.device("cuda")
    blob = m._blob(dev)
    st = _hip.stream_ptr()
    arr = (ctypes.c_void_p * n)(*[t.data_ptr() for t in [p.float().contiguous() for p in m._canonical_params()]])
    assert L.uspace_idnet_pack_weights(r, arr, n - 1, _hip.ptr(blob), blob.numel(), st) == ERR_ARG
    assert L.uspace_idnet_pack_weights(r, arr, n, _hip.ptr(blob), blob.numel() - 1, st) == ERR_WS
    assert L.uspace_idnet_pack_weights(r, arr, n, None, blob.numel(), st) == ERR_ARG
    x = torch.zeros(1, 3, 40, 40, device=dev)
    xn = torch.zeros(1, 32, 32, 3, device=dev)
    out = torch.zeros(1, 32, 32, 3, device=dev)
    for args in ((None, 1, 40, 40, 1, 1, 32, _hip.ptr(out)), (_hip.ptr(x), 0, 40, 40, 1, 1, 32, _hip.ptr(out)),
                 (_hip.ptr(x), 1, 0, 40, 1, 1, 32, _hip.ptr(out)), (_hip.ptr(x), 1, 40, 40, 1, 1, 0, _hip.ptr(out)),
                 (_hip.ptr(x), 1, 40, 40, 1, 1, 32, None)):
        assert L.uspace_idnet_preprocess(*args, st) == ERR_ARG
    ws = m._workspace(1, dev)
    emb = torch.zeros(1, 512, device=dev)
    assert L.uspace_idnet_forward(r, _hip.ptr(blob), _hip.ptr(ws), ws.numel(), _hip.ptr(xn), 1, None, st) == ERR_ARG
    assert L.uspace_idnet_forward(r, None, _hip.ptr(ws), ws.numel(), _hip.ptr(xn), 1, _hip.ptr(emb), st) == ERR_ARG
    assert L.uspace_idnet_forward(r, _hip.ptr(blob), _hip.ptr(ws), ws.numel(), _hip.ptr(xn), 0, _hip.ptr(emb), st) == ERR_ARG
    assert L.uspace_idnet_forward(r, _hip.ptr(blob), _hip.ptr(ws), 1024, _hip.ptr(xn), 1, _hip.ptr(emb), st) == ERR_WS
    for stage in (-1, 6):
        assert L.uspace_idnet_tap(r, _hip.ptr(blob), _hip.ptr(ws), ws.numel(), _hip.ptr(xn), 1, stage, _hip.ptr(emb), st) == ERR_ARG
    assert L.uspace_idnet_tap(r, _hip.ptr(blob), _hip.ptr(ws), ws.numel(), _hip.ptr(xn), 1, 5, None, st) == ERR_ARG
    um = torch.zeros(1, 8, 8, 64, device=dev)
    uo = torch.zeros(1, 4, 4, 64, device=dev)
    assert L.uspace_idnet_unit(r, _hip.ptr(blob), _hip.ptr(ws), ws.numel(), 4, _hip.ptr(um), 1, 8, 8, _hip.ptr(uo), st) == ERR_ARG
    assert L.uspace_idnet_unit(r, _hip.ptr(blob), _hip.ptr(ws), 1024, 0, _hip.ptr(um), 1, 8, 8, _hip.ptr(uo), st) == ERR_WS
    assert L.uspace_idnet_unit(r, _hip.ptr(blob), _hip.ptr(ws), ws.numel(), 0, _hip.ptr(um), 1, 8, 8, None, st) == ERR_ARG
    sim = torch.zeros(1, dtype=torch.float64, device=dev)
    assert L.uspace_idnet_similarity_f64(_hip.ptr(emb), _hip.ptr(emb), 0, _hip.ptr(sim), st) == ERR_ARG
    assert L.uspace_idnet_similarity_f64(_hip.ptr(emb), None, 1, _hip.ptr(sim), st) == ERR_ARG
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        m(torch.zeros(1, 3, 48, 48, device=dev))
    with pytest.raises(_hip.UspaceHipError):
        m(torch.zeros(1, 3, 32, 32))
    with pytest.raises(_hip.UspaceHipError):
        similarity(emb, torch.zeros(2, 512, device=dev))
    with pytest.raises(ValueError):
        m.unit(9, um)
