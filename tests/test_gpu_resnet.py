"""The attribute-classifier tower (csrc/resnet.hip, libs/resnet.py) on the GPU against the float64 stage model of
tests/resnet_stages.py: every tap stage from the GPU's own previous stage, the logits from the GPU's own pooled vector and from the
images, on the two golden nets and the seeded net at the sizes of tests/resnet_cases.py; bit-identity across batch sizes,
positions and chunking; ResNet-50 whole; the refusals.  Every figure is printed before it is judged; the bounds are
``resnet_cases.TOL``."""
import ctypes

import pytest
import torch

from tests import resnet_cases as C
from tests import resnet_stages as R

pytestmark = pytest.mark.gpu

_TOWERS = {}


def tower(name):
    """(module on the device, arch, state dict on the host) of one of ``resnet_cases.NETS``, built once."""
    if name not in _TOWERS:
        arch, sd = C.net(name)
        _TOWERS[name] = (C.module(name).cuda(), arch, sd)
    return _TOWERS[name]


def report(kind, case, value):
    value = float(value)
    print(f"RESNET-MEASURE {kind} {case}: {value:.3e} (bound {C.TOL[kind]:.1e})")
    return value


# --------------------------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("name,H,W,B", C.PARITY_CASES + C.POOL_CASES)
def test_stage_parity(name, H, W, B):
    m, arch, sd = tower(name)
    x, z_ref, _ = C.reference(name, H, W, B)
    xd = x.cuda()
    worst = {k: 0.0 for k in ("stem", "block", "pooled")}
    prev = x.double()
    n = R.n_stages(arch)
    for s in range(n):
        got = m.tap(xd, s).cpu()
        got = R.nchw(got) if got.dim() == 4 else got
        want = R.stage(sd, arch, s, prev)
        assert got.shape == want.shape, (s, got.shape, want.shape)
        k = R.stage_kind(arch, s)
        worst[k] = max(worst[k], report(k, (name, H, W, B, s), R.rel_l2(got, want).max()))
        prev = got.double()
    logits, pooled = m(xd, return_pooled=True)
    assert logits.shape == (B, 40) and logits.dtype == torch.float32
    assert torch.equal(pooled.cpu().double(), prev)      # the forward's pooled vector is the tap's last stage
    worst["logits"] = report("logits", (name, H, W, B), R.rel_l2(logits.cpu(), R.logits(sd, prev)).max())
    worst["tower"] = report("tower", (name, H, W, B), R.rel_l2(logits.cpu(), z_ref).max())
    for k, v in worst.items():
        assert v <= C.TOL[k], (k, v)


def test_pool_cases_reach_one_pixel_and_seventy():
    m, _, _ = tower("seeded")
    assert [m.stage_shapes(h, w)[-1][:2] for _, h, w, _ in C.POOL_CASES] == [(1, 1), (7, 10)]


# --------------------------------------------------------------------------------------------------------- bit-identity
@pytest.mark.parametrize("name,H,W", [("golden_bottleneck", 40, 56), ("golden_basic", 33, 47), ("seeded", 64, 64)])
def test_bit_identical_across_batch_and_position(name, H, W):
    m, arch, _ = tower(name)
    x = C.images(5, H, W).cuda()
    n = R.n_stages(arch)
    taps = [m.tap(x, s) for s in range(n)]
    logits = m(x)
    assert torch.equal(logits, m(x)) and torch.equal(logits, m(x, chunk=2)) and torch.equal(logits, m(x, chunk=1))
    m._workspace(5, H, W, x.device).fill_(255)      # nothing of the workspace is read before it is written: NaN patterns change nothing
    assert torch.equal(m(x), logits)
    m._workspace(5, H, W, x.device).fill_(255)
    assert torch.equal(m.tap(x, n - 1), taps[n - 1])
    order = [4, 0, 2]
    shuffled = x[order].contiguous()
    assert torch.equal(m(shuffled), logits[order])
    for s in range(n):
        assert torch.equal(m.tap(shuffled, s), taps[s][order]), s
    for pos in (0, 2, 4):
        one = x[pos:pos + 1]
        assert torch.equal(m(one)[0], logits[pos]), pos
        for s in range(n):
            assert torch.equal(m.tap(one, s)[0], taps[s][pos]), (pos, s)


def test_resnet50_runs_whole_and_repeats():
    from uspace_amd.libs.resnet import RESNET50, ResNet
    m = ResNet(**RESNET50, seed=0).cuda()
    x = R.smooth_images(2, 224, 224, 7).cuda()
    z = m(x)
    assert z.shape == (2, 40) and bool(torch.isfinite(z).all()) and float(z.abs().max()) > 0
    assert torch.equal(z, m(x)) and torch.equal(z[1], m(x[1:2])[0])


def test_missing_weights_are_named_at_first_use():
    from uspace_amd.libs.resnet import ResNet
    arch, sd = C.net("seeded")
    m = ResNet(arch.block, arch.layers, 40, arch.planes, arch.stem).cuda()
    x = C.images(1, 32, 32).cuda()
    with pytest.raises(FileNotFoundError, match="weights="):
        m(x)
    m.load_state_dict(sd)
    assert torch.equal(m(x), tower("seeded")[0](x))


# ------------------------------------------------------------------------------------------------------------ refusals
def test_argument_refusals():
    from uspace_amd import _hip
    L = _hip.lib()
    m, _, _ = tower("seeded")
    r = ctypes.byref(m.cfg)
    ERR_ARG, ERR_WS = -1, -3
    dev = torch.device("cuda")
    blob = m._blob(dev)
    st = _hip.stream_ptr()
    n = L.uspace_resnet_num_params(r)
    arr = (ctypes.c_void_p * n)(*[t.data_ptr() for t in [p.float().contiguous() for p in m._canonical_params()]])
    assert L.uspace_resnet_pack_weights(r, arr, n - 1, _hip.ptr(blob), blob.numel(), st) == ERR_ARG
    assert L.uspace_resnet_pack_weights(r, arr, n, _hip.ptr(blob), blob.numel() - 1, st) == ERR_WS
    assert L.uspace_resnet_pack_weights(r, arr, n, None, blob.numel(), st) == ERR_ARG
    x = torch.zeros(1, 3, 40, 56, device=dev)
    xn = torch.zeros(1, 40, 56, 3, device=dev)
    mean, std = (ctypes.c_float * 3)(0.5, 0.5, 0.5), (ctypes.c_float * 3)(0.25, 0.25, 0.25)
    zero_std = (ctypes.c_float * 3)(0.25, 0.0, 0.25)
    for args in ((None, 1, 40, 56, mean, std, _hip.ptr(xn)), (_hip.ptr(x), 0, 40, 56, mean, std, _hip.ptr(xn)),
                 (_hip.ptr(x), 1, 0, 56, mean, std, _hip.ptr(xn)), (_hip.ptr(x), 1, 40, 56, None, std, _hip.ptr(xn)),
                 (_hip.ptr(x), 1, 40, 56, mean, zero_std, _hip.ptr(xn)), (_hip.ptr(x), 1, 40, 56, mean, std, None)):
        assert L.uspace_resnet_preprocess(*args, st) == ERR_ARG
    ws = m._workspace(1, 40, 56, dev)
    logits = torch.zeros(1, 40, device=dev)
    fwd = lambda *a: L.uspace_resnet_forward(r, *a, st)
    assert fwd(_hip.ptr(blob), _hip.ptr(ws), ws.numel(), _hip.ptr(xn), 1, 40, 56, None, None) == ERR_ARG
    assert fwd(None, _hip.ptr(ws), ws.numel(), _hip.ptr(xn), 1, 40, 56, None, _hip.ptr(logits)) == ERR_ARG
    assert fwd(_hip.ptr(blob), _hip.ptr(ws), ws.numel(), None, 1, 40, 56, None, _hip.ptr(logits)) == ERR_ARG
    assert fwd(_hip.ptr(blob), _hip.ptr(ws), ws.numel(), _hip.ptr(xn), 0, 40, 56, None, _hip.ptr(logits)) == ERR_ARG
    assert fwd(_hip.ptr(blob), _hip.ptr(ws), ws.numel(), _hip.ptr(xn), 1, 31, 56, None, _hip.ptr(logits)) == ERR_ARG
    assert fwd(_hip.ptr(blob), _hip.ptr(ws), 1024, _hip.ptr(xn), 1, 40, 56, None, _hip.ptr(logits)) == ERR_WS
    dump = torch.zeros(1, 64 * 4, device=dev)
    last = R.n_stages(C.SEEDED) - 1
    for stage in (-1, last + 1):
        assert L.uspace_resnet_tap(r, _hip.ptr(blob), _hip.ptr(ws), ws.numel(), _hip.ptr(xn), 1, 40, 56, stage, _hip.ptr(dump), st) == ERR_ARG
    assert L.uspace_resnet_tap(r, _hip.ptr(blob), _hip.ptr(ws), ws.numel(), _hip.ptr(xn), 1, 40, 56, last, None, st) == ERR_ARG
    z = torch.zeros(2, 4, device=dev)
    tgt, sg = torch.zeros(2, dtype=torch.int32, device=dev), torch.ones(2, device=dev)
    out = torch.zeros(2, 4, dtype=torch.float64, device=dev)
    eff = lambda *a: L.uspace_attr_effect_f64(*a, st)
    assert eff(None, _hip.ptr(z), _hip.ptr(tgt), _hip.ptr(sg), None, 2, 4, _hip.ptr(out)) == ERR_ARG
    assert eff(_hip.ptr(z), _hip.ptr(z), None, _hip.ptr(sg), None, 2, 4, _hip.ptr(out)) == ERR_ARG
    assert eff(_hip.ptr(z), _hip.ptr(z), _hip.ptr(tgt), None, None, 2, 4, _hip.ptr(out)) == ERR_ARG
    assert eff(_hip.ptr(z), _hip.ptr(z), _hip.ptr(tgt), _hip.ptr(sg), None, 0, 4, _hip.ptr(out)) == ERR_ARG
    assert eff(_hip.ptr(z), _hip.ptr(z), _hip.ptr(tgt), _hip.ptr(sg), None, 2, 0, _hip.ptr(out)) == ERR_ARG
    assert eff(_hip.ptr(z), _hip.ptr(z), _hip.ptr(tgt), _hip.ptr(sg), None, 2, 4, None) == ERR_ARG
    torch.cuda.synchronize()
    with pytest.raises(_hip.UspaceHipError):
        m(torch.zeros(1, 3, 31, 64, device=dev))
    with pytest.raises(_hip.UspaceHipError):
        m(torch.zeros(1, 3, 40, 56))
    with pytest.raises(ValueError):
        m(torch.zeros(1, 1, 40, 56, device=dev))
