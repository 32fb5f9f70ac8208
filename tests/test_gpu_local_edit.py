"""Local edits on the GPU (tests/local_edit_cases.py holds the cases, references and bounds): the three kernels of csrc/local_edit.hip
against their references, and the paired solve -- the outside of the mask bit-equal to the source under Euler, dopri5 and fixadp, the
two ends (mask 0, mask 1) against plain decodes, the CPU oracle's blended solve, the attention-word mask and the label-region mask."""
import functools
import json
import os
import tempfile

import numpy as np
import pytest
import torch

from tests import local_edit_cases as LE
from uspace_amd.tools import local_edit  # noqa: F401  (without the feature nothing in this file can run)

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.array(a, copy=True, order="C")).to("cuda")            # a copy: the shared inputs are read-only


def expand_t(tv, B):
    return torch.tensor(float(tv), dtype=torch.float32, device="cuda").expand(B)


@functools.lru_cache(maxsize=None)
def gpu_net(name):
    net = LE.make(name).to("cuda").eval()
    net.use_graph = False
    return net


def cnf_of(name):
    from uspace_amd import flow_matching, flow_matching_t2i
    return (flow_matching_t2i if LE.NETS[name][1] else flow_matching).CNF(gpu_net(name))


# ------------------------------------------------------------------------------------------------------------------ pair_blend
@pytest.mark.parametrize("shape", LE.BLEND_SHAPES, ids=str)
def test_pair_blend_matches_the_formula(shape):
    """Source rows unchanged; exact where the mask is 0, 1, NaN, below 0 or above 1; within 1 ulp of the float64 value on operands of one
    sign within a factor 2 (e - s exact, one rounding), within 2^-24 (m |e - s| + |ref|) on arbitrary ones (tests/local_edit_cases.py on
    why 1 ulp of the result is not derivable there); in place, out of place, and from a pointer offset by 4 bytes (the scalar form).
    Measured on an MI355X: at most 0.500 ulp on the near operands and 0.973 of the derived bound on the arbitrary ones, of which 951 of
    20 480 elements at (5, 4, 1024) lie beyond 1 ulp of their (cancelled) result."""
    from uspace_amd import _hip
    B, C, cells = shape
    worst_ulp = worst_general = 0.0
    beyond = 0
    for near in (True, False):
        pair, mask = LE.blend_inputs(shape, near=near)
        ref = LE.blend_reference(pair, mask)
        bound = LE.blend_general_bound(pair, mask)
        p, m = dev(pair), dev(mask)
        out = _hip.pair_blend(p, m, out=torch.empty_like(p))
        assert torch.equal(p, dev(pair))                                   # out of place: the input is left alone
        inplace = p.clone()
        assert _hip.pair_blend(inplace, m) is inplace and torch.equal(inplace, out)
        flat = torch.empty(pair.size + 1, dtype=torch.float32, device="cuda")
        shifted = flat[1:].view(p.shape)
        shifted.copy_(p)
        assert shifted.data_ptr() % 16 == 4 and torch.equal(_hip.pair_blend(shifted, m), out)
        got = out.cpu().numpy()
        np.testing.assert_array_equal(got[:B], pair[:B])
        mm = np.broadcast_to(mask.reshape(B, 1, cells), (B, C, cells))
        np.testing.assert_array_equal(got[B:][mm == 0], pair[:B][mm == 0])
        np.testing.assert_array_equal(got[B:][mm == 1], pair[B:][mm == 1])
        u = LE.ulps(got[B:], ref[B:])
        if near:
            worst_ulp = max(worst_ulp, float(u.max()))
            assert u.max() <= LE.TOL["blend_ulp"]
        else:
            beyond += int((u > 1).sum())
        ratio = np.abs(got[B:] - ref[B:]) / np.maximum(bound, 1e-300)
        worst_general = max(worst_general, float(ratio[np.abs(got[B:] - ref[B:]) > 0].max(initial=0.0)))
        assert np.all(np.abs(got[B:] - ref[B:]) <= bound * (1 + 1e-9))
    print(f"pair_blend {shape}: worst {worst_ulp:.3f} ulp (near operands), {worst_general:.3f} of the derived bound; "
          f"{beyond} general elements beyond 1 ulp of the result")
    # the special mask values, all of them exact
    pair, _ = LE.blend_inputs(shape)
    for mv in LE.BLEND_EXACT_M:
        got = _hip.pair_blend(dev(pair), torch.full((B, cells), mv, device="cuda"))
        want = pair[B:] if mv >= 1 else pair[:B]
        assert torch.equal(got[B:], dev(want)) and torch.equal(got[:B], dev(pair[:B])), mv


def test_pair_blend_wrapper_rejects_bad_operands():
    from uspace_amd import _hip
    with pytest.raises(ValueError):
        _hip.pair_blend(torch.zeros(3, 4, 8, device="cuda"), torch.zeros(1, 8, device="cuda"))
    with pytest.raises(ValueError):
        _hip.pair_blend(torch.zeros(4, 4, 8, device="cuda"), torch.zeros(2, 4, device="cuda"))
    with pytest.raises(ValueError):
        _hip.pair_blend(torch.zeros(4, 4, 8, device="cuda"), torch.zeros(2, 8, device="cuda"), out=torch.zeros(4, 4, 4, device="cuda"))
    with pytest.raises(_hip.UspaceHipError):
        _hip.pair_blend(torch.zeros(4, 4, 8), torch.zeros(2, 8))


# ------------------------------------------------------------------------------------------------------------------ mask_from_labels
@pytest.mark.parametrize("case", LE.LABEL_CASES, ids=str)
def test_mask_from_labels_is_exact(case):
    from uspace_amd import _hip
    B, H, W, S, dilate = case
    lab = LE.label_maps(case)
    members = {"region": LE.member_of(), "empty": np.zeros(256, np.uint8), "full": np.ones(256, np.uint8)}
    for name, member in members.items():
        for soft, thr in [(True, 0.0)] + [(False, t) for t in LE.LABEL_THRESHOLDS]:
            got = _hip.mask_from_labels(dev(lab), dev(member), S, dilate, thr, soft)
            assert got.shape == (B, S, S) and got.dtype == torch.float32
            want = LE.labels_mask_reference(lab, member, S, dilate, thr, soft)
            np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=f"{case} {name} soft={soft} thr={thr}")
    # a sample's mask does not depend on the batch it sits in
    whole = _hip.mask_from_labels(dev(lab), dev(members["region"]), S, dilate, 0.0, True)
    for b in range(B):
        assert torch.equal(_hip.mask_from_labels(dev(lab[b:b + 1]), dev(members["region"]), S, dilate, 0.0, True)[0], whole[b])


# ------------------------------------------------------------------------------------------------------------------ mask_from_maps
@pytest.mark.parametrize("case", LE.MAPS_CASES, ids=str)
def test_mask_from_maps_matches_the_float64_reference(case):
    """soft: max |got - ref64| <= TOL["maps_soft"] = 4.54e-7 (3 x the worst value measured on the MI355X, 1.511e-7 on MAPS_TOL_CASE; below
    its n_blocks nk 2^-24 = 7.8e-5; the other cases measured 0 to 7.1e-8).
    binary: equal to the reference wherever its normalised value is farther from the threshold than that bound, at most 1 % of the cells
    excused.  Bit-equal across runs and whatever R a row sits in."""
    from uspace_amd import _hip
    n_blocks, R, G, nk, patch = case
    maps, w, cols = LE.maps_inputs(case)
    dm, dw, dc = dev(maps), dev(w), dev(cols)
    soft = _hip.mask_from_maps(dm, dw, dc, G, patch, LE.MAPS_THR, True)
    assert soft.shape == (R, G * patch, G * patch)
    ref_soft, norm = LE.maps_mask_reference(maps, w, cols, G, patch, LE.MAPS_THR, True)
    err = float(np.abs(soft.cpu().numpy() - ref_soft).max())
    print(f"mask_from_maps {case}: max |soft - ref64| = {err:.3e} (bound {LE.TOL['maps_soft']:.2e}, a priori {LE.maps_apriori(case):.2e})")
    assert err <= LE.TOL["maps_soft"]
    hard = _hip.mask_from_maps(dm, dw, dc, G, patch, LE.MAPS_THR, False)
    ref_hard, _ = LE.maps_mask_reference(maps, w, cols, G, patch, LE.MAPS_THR, False)
    loose = LE.excused(norm, LE.MAPS_THR, LE.TOL["maps_soft"])
    assert loose.mean() <= LE.MAPS_EXCUSED_SHARE
    got = hard.cpu().numpy()
    np.testing.assert_array_equal(got[~loose], ref_hard[~loose])
    assert set(np.unique(got)) <= {0.0, 1.0}
    for r in range(R):
        if not cols[r].any():
            assert float(soft[r].abs().max()) == 0 and float(hard[r].max()) == 0
    assert torch.equal(_hip.mask_from_maps(dm, dw, dc, G, patch, LE.MAPS_THR, True), soft)
    for r in range(R):
        one = _hip.mask_from_maps(dm[:, r:r + 1].contiguous(), dw, dc[r:r + 1].contiguous(), G, patch, LE.MAPS_THR, True)
        assert torch.equal(one[0], soft[r]), r


# ------------------------------------------------------------------------------------------------------------------ solves
@pytest.fixture(scope="module")
def deltas():
    """Direction files for a write hook at every timestep digit, the same table under each (the field is continuous in t); image-shaped
    for head and tail."""
    with tempfile.TemporaryDirectory() as d:
        table = (0.5 * np.random.default_rng(5).standard_normal((3, 4, 16, 16))).astype(np.float32)
        for k in range(1, 101):
            np.save(os.path.join(d, f"delta_{k / 100:.2f}.npy"), table)
        yield d


def _outside(mask, like):
    return torch.from_numpy(np.broadcast_to(np.asarray(mask)[:, None] == 0, tuple(like.shape)).copy()).cuda()


def _assert_local(edited, source, mask):
    """Every latent cell where the mask is 0 is bit-equal to the source in all channels; every cell where it is 1 differs."""
    out = _outside(mask, edited)
    assert torch.equal(edited[out], source[out])
    differs = (edited != source).any(dim=1).cpu().numpy()
    assert differs[np.asarray(mask) == 1].all() and not differs[np.asarray(mask) == 0].any()


def test_mask_zero_and_mask_one_are_the_plain_solves(deltas):
    """(1) mask 0: edited == source.  (2) mask 1: both halves bit-equal to a plain decode on the concatenated 2B inputs with the same
    per-row keywords."""
    name, B = "tiny_u", 3
    cnf = cnf_of(name)
    z = dev(LE.solve_inputs(name, B)["z"])
    kw = LE.write_kwargs(deltas, "tail", [1.0, -1.0, 0.5])
    edited, source = cnf.decode_local(z, None, mask=np.zeros((16, 16), np.float32), solver_kwargs=LE.SOLVER, **kw)
    assert torch.equal(edited, source) and cnf.last_stats.nfe == 4
    edited, source = cnf.decode_local(z, None, mask=np.ones((B, 1, 16, 16), np.float32), solver_kwargs=LE.SOLVER, **kw)
    rows = np.array([0, 0, 0, 1.0, -1.0, 0.5], np.float32)
    plain = cnf.decode(torch.cat([z, z]), None, solver_kwargs=LE.SOLVER, **dict(kw, write_scale=rows))
    assert torch.equal(edited, plain[B:]) and torch.equal(source, plain[:B]) and not torch.equal(edited, source)
    unedited = cnf.decode(z, None, solver_kwargs=LE.SOLVER, dissect_name="none", edit_loc=None)
    assert LE.rel_l2(source.cpu().numpy(), unedited.cpu().numpy()) < 2e-3       # the source is the unedited decode (at batch 2B)


@pytest.mark.parametrize("mask_name", ["half_plane", "checkerboard"])
@pytest.mark.parametrize("edit", ["tail", "head", "p2p"])
def test_outside_the_mask_is_the_source_bit_for_bit(deltas, edit, mask_name):
    B = 2
    mask = getattr(LE, mask_name)(B)
    if edit == "p2p":
        name = "tiny_t2i"
        inp = LE.solve_inputs(name, B)
        kw = dict(dissect_name="p2p", t_edit=1.0, block_id="all", token_kwargs=dict(token_dissect="p2p_rescale", p2p_multiplier=8.0),
                  target_context_ids=[np.array([3, 5]), np.array([0, 76])])
        edited, source = cnf_of(name).decode_local(dev(inp["z"]), context=dev(inp["ctx"]), mask=mask, solver_kwargs=LE.SOLVER, **kw)
    else:
        name = "tiny_u"
        inp = LE.solve_inputs(name, B)
        edited, source = cnf_of(name).decode_local(dev(inp["z"]), None, mask=dev(mask), solver_kwargs=LE.SOLVER, **LE.write_kwargs(deltas, edit, 1.5))
    _assert_local(edited, source, mask)


@pytest.mark.parametrize("solver", ["dopri5", "fixadp"])
def test_outside_the_mask_under_error_controlled_solves(deltas, solver):
    name, B = "tiny_u", 2
    cnf = cnf_of(name)
    z = dev(LE.solve_inputs(name, B)["z"])
    mask = LE.checkerboard(B)
    if solver == "dopri5":
        sk, kw = dict(solver="adaptive", solver_adaptive="dopri5"), LE.write_kwargs(deltas, "tail", 1.5)
    else:
        sk = dict(solver="fixadp", solver_fix="euler", solver_fix_step=0.25, solver_adaptive="dopri5")
        kw = dict(LE.write_kwargs(deltas, "tail", 1.5), t_edit=0.5)
    edited, source = cnf.decode_local(z, None, mask=mask, solver_kwargs=sk, **kw)
    st = cnf.last_stats
    print(f"decode_local {solver}: nfe {st.nfe}, accepted {st.accepted}, rejected {st.rejected}")
    assert st.nfe > 4 and st.accepted >= 1
    _assert_local(edited, source, mask)


def test_euler_solve_matches_the_blended_oracle_solve(deltas):
    """SOLVE_CASE (a tail write, the soft mask of three bands): rel-L2 of ``edited`` against the CPU oracle's Euler solve over both
    branches with the float64 blend <= TOL["solve_rel_l2"] = 5.63e-4 = 3 x the value measured on the MI355X (1.874e-4), capped by 1e-2;
    blending the state instead misses by 3.06e-2 on the oracle."""
    name, B, loc, _ = LE.SOLVE_CASE
    cnf = cnf_of(name)
    z = LE.solve_inputs(name, B)["z"]
    with tempfile.TemporaryDirectory() as d:
        LE.write_deltas(d, z.shape[1:], LE.EULER_DIGITS)
        edited, source = cnf.decode_local(dev(z), None, mask=LE.soft_bands(B), solver_kwargs=LE.SOLVER, **LE.write_kwargs(d, loc))
    ref = LE.oracle_solve()
    r = LE.rel_l2(edited.cpu().numpy(), ref)
    print(f"euler-4 blended decode vs oracle: rel-L2 {r:.3e} (bound {LE.TOL['solve_rel_l2']:.2e}); "
          f"state-blend fault {LE.rel_l2(LE.oracle_solve('state_blended'), ref):.3e}")
    assert LE.TOL["solve_rel_l2"] <= LE.SOLVE_CAP and r <= LE.TOL["solve_rel_l2"]
    out = _outside(LE.soft_bands(B), edited)
    assert torch.equal(edited[out], source[out])


def test_local_prompt_pairs_two_contexts():
    name, B = "tiny_t2i", 3
    cnf = cnf_of(name)
    inp = LE.solve_inputs(name, B)
    z, ctx, ctx_src = dev(inp["z"]), dev(inp["ctx"]), dev(inp["ctx_src"])
    mask = LE.half_plane(B)
    kw = dict(dissect_name="local_prompt", t_edit=0.5, token_kwargs=dict(token_dissect="lp_replace"))
    edited, source = cnf.decode_local(z, context=ctx, mask=mask, source=dict(context=ctx_src), solver_kwargs=LE.SOLVER, **kw)
    plain = cnf.decode(torch.cat([z, z]), context=torch.cat([ctx_src, ctx]), solver_kwargs=LE.SOLVER, **kw)
    assert torch.equal(source, plain[:B]) and not torch.equal(edited, plain[B:])
    _assert_local(edited, source, mask)


def test_attention_word_mask():
    from uspace_amd import _hip
    from uspace_amd.odeint import HipStateOps
    from uspace_amd.tools.local_edit import AttentionWordMask
    name, B = "tiny_t2i", 2
    net, cnf = gpu_net(name), cnf_of(name)
    inp = LE.solve_inputs(name, B)
    z, ctx, ctx_src = dev(inp["z"]), dev(inp["ctx"]), dev(inp["ctx_src"])
    kw = dict(dissect_name="none", solver_kwargs=LE.SOLVER)
    ids = ([np.array([2]), np.array([4, 5])], np.array([3]))
    # the evaluation at t = 0.25 is the first one at or after from_t: its state is z + 0.25 v(0, z), the one at t = 0 being plain.
    # The threshold is the median of that evaluation's normalised values, so that the mask is neither empty nor full on this net,
    # whose attention (the module's own init) is close to uniform
    z2, ctx2 = torch.cat([z, z]), torch.cat([ctx_src, ctx])
    v0, _ = net(z2, expand_t(0.0, 2 * B), ctx2, _t_host=0.0)
    x1 = HipStateOps(z2).combine(z2, [v0], [0.25])
    maps = net.attention_maps(x1, expand_t(0.25, 2 * B), ctx2, _t_host=0.25)
    cols = np.zeros((2 * B, 77), np.float32)
    cols[0, 2] = cols[1, 4] = cols[1, 5] = cols[2, 3] = cols[3, 3] = 1.0
    ones = torch.ones(net.depth + 1, device="cuda")
    thr = float(_hip.mask_from_maps(maps, ones, dev(cols), 8, 2, 0.0, True).median())
    record = []
    wm = AttentionWordMask(token_ids=ids, blocks="all", threshold=thr, from_t=0.2, record=record)
    edited, source = cnf.decode_local(z, context=ctx, mask=wm, source=dict(context=ctx_src), **kw)
    assert [t for t, _ in record] == [0.25, 0.5, 0.75] and cnf.last_stats.nfe == 4
    both = _hip.mask_from_maps(maps, ones, dev(cols), 8, 2, thr, False)
    want = torch.maximum(both[:B], both[B:])
    print(f"attention-word mask at t = 0.25: threshold {thr:.4f}, share of open cells {float(want.mean()):.3f}")
    assert torch.equal(record[0][1], want) and 0 < float(want.mean()) < 1
    assert not torch.equal(edited, source) and all(m.shape == (B, 16, 16) for _, m in record)
    # below from_t the solve is the mask == 1 solve, bit for bit
    late = AttentionWordMask(token_ids=ids, from_t=2.0)
    e1, s1 = cnf.decode_local(z, context=ctx, mask=late, source=dict(context=ctx_src), **kw)
    e2, s2 = cnf.decode_local(z, context=ctx, mask=np.ones((16, 16), np.float32), source=dict(context=ctx_src), **kw)
    assert torch.equal(e1, e2) and torch.equal(s1, s2)
    # a caption without the word: no edit anywhere
    none = AttentionWordMask(token_ids=(np.array([], dtype=np.int64), np.array([], dtype=np.int64)), from_t=0.0)
    e0, s0 = cnf.decode_local(z, context=ctx, mask=none, source=dict(context=ctx_src), **kw)
    assert torch.equal(e0, s0) and not torch.equal(e2, s2)


def _tiny_vae(golden_dir):
    from uspace_amd.libs.autoencoder import FrozenAutoencoderKL
    meta = json.loads(bytes(np.load(os.path.join(golden_dir, "vae_decoder_tiny.npz"))["meta_json"]).decode())
    torch.manual_seed(meta["weight_seed"])
    return FrozenAutoencoderKL(meta["ddconfig"], 4).cuda()


def _toy_logits(images):
    """A hand-made parser: three labels from the red channel at half resolution -- label 1 where it lies above the image's mean, label 2
    where below."""
    red = torch.nn.functional.avg_pool2d(images[:, :1].float(), 2)
    d = red - red.mean(dim=(2, 3), keepdim=True)
    return torch.cat([torch.zeros_like(d), d, -d], dim=1)


def test_label_region_mask_and_edit_region(golden_dir, deltas):
    from uspace_amd.tools.local_edit import LabelRegionMask, edit_region
    from uspace_amd.tools.seg_metrics import LogitsParser
    name, B = "tiny_u", 2
    cnf, vae = cnf_of(name), _tiny_vae(golden_dir)
    z = dev(LE.solve_inputs(name, B)["z"])
    region = LabelRegionMask(LogitsParser(_toy_logits, 3), [1], dilate=1, threshold=0.25)
    g = torch.Generator().manual_seed(3)
    images = torch.rand(B, 3, 4, 4, generator=g).repeat_interleave(8, dim=2).repeat_interleave(8, dim=3).cuda()     # blocks of 8 x 8 pixels
    images[0, 0, :8, :8] = 1.0                                                    # label 1 in a corner: the region touches the border
    bound = region.of(images, 16)
    member = np.zeros(256, np.uint8)
    member[1] = 1
    want = LE.labels_mask_reference(bound.labels.cpu().numpy(), member, 16, 1, 0.25, False)
    np.testing.assert_array_equal(bound.mask.cpu().numpy(), want)
    assert region.mask is None and 0 < want.mean() < 1 and want[0, 0, 0] == 1
    soft = LabelRegionMask(LogitsParser(_toy_logits, 3), [1], dilate=0, soft=True).of(images, 16)
    np.testing.assert_array_equal(soft.mask.cpu().numpy(), LE.labels_mask_reference(bound.labels.cpu().numpy(), member, 16, 0, 0.0, True))
    # end to end: decode -> vae.decode -> mask of the source image -> decode_local
    kw = dict(LE.write_kwargs(deltas, "tail", 1.5), solver_kwargs=LE.SOLVER)
    region = LabelRegionMask(LogitsParser(_toy_logits, 3), [1], dilate=0, threshold=0.5)
    edited, source, mask = edit_region(cnf, vae, z, None, region, **kw)
    plain = cnf.decode(z, None, solver_kwargs=LE.SOLVER, dissect_name="none", edit_loc=None)
    img = vae.decode(plain).mul(0.5).add(0.5).clamp(0, 1)
    again = region.of(img, 16)
    assert torch.equal(mask, again.mask) and mask.shape == (B, 16, 16)
    m = mask.cpu().numpy()
    assert 0 < m.mean() < 1, "the toy parser's region is neither empty nor everything"
    _assert_local(edited, source, m)
    e2, s2 = cnf.decode_local(z, None, mask=again, **kw)
    assert torch.equal(e2, edited) and torch.equal(s2, source)
