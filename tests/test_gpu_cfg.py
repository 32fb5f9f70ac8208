"""Classifier-free guidance on the GPU (tests/cfg_cases.py holds the nets, inputs, references and bounds):
(A) the combine kernel against the float64 formula, (B) the paired forward's 2B predictions bit-equal to the plain forward on
concatenated inputs, (C) the modules against the CPU oracle's v_c + s (v_c - v_u); per-sample scales, the p2p edit and the u-space hooks
under guidance, an Euler solve, and the unguided path left as it was.
"""
import functools
import os
import tempfile

import numpy as np
import pytest
import torch

from tests import cfg_cases as CC
from tests.util import rel_l2

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def gpu_net(name):
    net = CC.make(name).to("cuda").eval()
    net.use_graph = False
    return net


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def expand_t(tv, B):
    return torch.tensor(float(tv), dtype=torch.float32, device="cuda").expand(B)     # stride 0, like the solver


def within_combine_bound(got, pair, s, rows=None):
    """(A) for ``got`` [B, ...] against ``pair`` [2B, ...] (tensors): the worst |got - ref| / bound, which has to be <= 1."""
    p = pair.double().cpu().numpy()
    B = p.shape[0] // 2
    rs = None if rows is None else rows.cpu().numpy()
    err = np.abs(got.double().cpu().numpy() - CC.guided_reference(p[:B], p[B:], s, rs))
    bound = CC.combine_bound(p[:B], p[B:], s, rs)
    return float((err / np.maximum(bound, 1e-300)).max()) if err.max() > 0 else 0.0


# ------------------------------------------------------------------------------------------------------------------ (A)
@pytest.mark.parametrize("per", [1, 3, 4, 1024, 4099])
def test_combine_kernel_matches_the_formula(per):
    """|got - ref64| <= 2^-22 (|s_b| |c - u| + |ref|) elementwise, and bit-equal to c at s = 0.  Measured on an MI355X: at most 0.25 of
    the bound (two roundings of 2^-24 each)."""
    from uspace_amd import _hip
    g = torch.Generator().manual_seed(per)
    worst = 0.0
    for B in (1, 5):
        pair = (torch.randn(2 * B, per, generator=g) * torch.exp(2.0 * torch.randn(2 * B, per, generator=g))).cuda()
        rows = (torch.rand(B, generator=g) * 3.0 - 1.0).cuda()
        for s in (0.0, 0.4, 7.5, -1.0):
            for rs in (None, rows):
                got = _hip.cfg_combine(pair, s, row_scale=rs)
                assert got.shape == (B, per) and got.dtype == torch.float32
                if s == 0.0:
                    assert torch.equal(got, pair[:B])
                w = within_combine_bound(got, pair, s, rs)
                worst = max(worst, w)
                assert w <= 1.0, (B, s, rs is not None, w)
        zero_rows = torch.zeros(B, device="cuda")
        assert torch.equal(_hip.cfg_combine(pair, 7.5, row_scale=zero_rows), pair[:B])
    print(f"combine per_sample={per}: worst error / bound = {worst:.3f}")


def test_combine_wrapper_rejects_bad_operands():
    from uspace_amd import _hip
    with pytest.raises(ValueError):
        _hip.cfg_combine(torch.zeros(3, 8, device="cuda"), 0.4)
    with pytest.raises(ValueError):
        _hip.cfg_combine(torch.zeros(4, 8, device="cuda"), 0.4, row_scale=torch.zeros(3, device="cuda"))
    with pytest.raises(_hip.UspaceHipError):
        _hip.cfg_combine(torch.zeros(4, 8), 0.4)


# ------------------------------------------------------------------------------------------------------------------ (B)
def _pair_operands(name, B, batched):
    """(net, x, cond context, unconditional context as the C entry takes it, the same expanded to [B, ...]) on the device."""
    net = gpu_net(name)
    inp = CC.inputs(name, B)
    x = dev(inp["x"])
    if CC.NETS[name][1]:
        ctx, one = dev(inp["ctx"]), dev(inp["empty"]) + 0.25          # not all zero here: a dropped or misplaced row would show
        full = one[None].expand(B, -1, -1).contiguous()
    else:
        w = net.label_emb.weight.detach()
        ctx, one = w[dev(inp["y"])].contiguous(), w[inp["empty"]].contiguous()
        full = one[None].expand(B, -1).contiguous()
    return net, x, ctx, (full if batched else one), full


@pytest.mark.parametrize("name,B,batched", [("tiny_t2i", 1, False), ("tiny_t2i", 3, False), ("tiny_t2i", 3, True), ("mid_t2i", 3, False),
                                            ("tiny_cls", 1, True), ("tiny_cls", 3, False), ("tiny_cls", 3, True), ("long_t2i", 1, False)])
def test_paired_forward_is_the_plain_forward_at_2B(name, B, batched):
    """pair_out is bit-equal to the plain forward on cat([x, x]), cat([t, t]), cat([ctx, empty]) in both LayerNorm modes, with a
    stride-0 and with per-row timesteps, and with a key-scale table whose second half is ones; io->out satisfies (A) on pair_out."""
    from uspace_amd import _hip
    net, x, ctx, uncond, full = _pair_operands(name, B, batched)
    L = _hip.lib()
    x2, ctx2 = torch.cat([x, x]), torch.cat([ctx, full])
    rows = dev(np.array(CC.SWEEP[-B:], np.float32))                  # B = 1: 7.5; B = 3: 0, 0.4, 7.5
    g = torch.Generator().manual_seed(3)
    ks = torch.cat([0.5 + 1.5 * torch.rand(net.depth + 1, B, net.seq_len, generator=g), torch.ones(net.depth + 1, B, net.seq_len)], 1).cuda()
    per_row = dev(np.array([0.1, 0.35, 0.9][:B], np.float32))
    seen = []
    try:
        for fold in (1, 0):
            _hip.check(L.uspace_uvit_set_ln_fold(fold), "set_ln_fold")
            for t, t2 in ((expand_t(CC.T_VAL, B), expand_t(CC.T_VAL, 2 * B)), (per_row, torch.cat([per_row, per_row]))):
                for key_scale in (None, ks):
                    out, pair = net._run(x, t, context=ctx, key_scale=key_scale, cfg=(uncond, batched, CC.S_CFG, rows, True))
                    plain = net._run(x2, t2, context=ctx2, key_scale=key_scale)
                    assert pair.shape == plain.shape and torch.equal(pair, plain), (fold, t.stride(0), key_scale is not None)
                    assert within_combine_bound(out, pair, CC.S_CFG, rows) <= 1.0
                    if B == 3:
                        assert torch.equal(out[0], pair[0])                              # SWEEP[0] = 0: the conditional row itself
                    seen.append(pair)
    finally:
        L.uspace_uvit_set_ln_fold(-1)
    assert not torch.equal(seen[0][:B], seen[0][B:])                                     # the two halves are two conditions
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[0], seen[2])       # the table and the timesteps are felt
    # without pair_out the predictions stay in the workspace: same guided result
    again = net._run(x, per_row, context=ctx, key_scale=ks, cfg=(uncond, batched, CC.S_CFG, rows, False))
    last, _ = net._run(x, per_row, context=ctx, key_scale=ks, cfg=(uncond, batched, CC.S_CFG, rows, True))
    assert torch.equal(again, last)


# ------------------------------------------------------------------------------------------------------------------ (C)
def test_t2i_module_matches_the_guided_oracle():
    """MID, the module's own init, all-zero empty context, s = 7.5: ||got - ref|| / max(||v_c||, ||v_u||) <= (1 + 2 s) 1e-2 = 0.16,
    where leaving the guidance out misses by 0.83.  Measured on an MI355X: 1.95e-2."""
    B = 3
    sd, inp, vc, vu = CC.oracle_case("mid_t2i", B)
    assert CC.guidance_is_visible(vc, vu, CC.S_BIG)
    net = gpu_net("mid_t2i")
    ref = CC.guided_reference(vc, vu, CC.S_BIG)
    for empty in (dev(inp["empty"]), inp["empty"], dev(np.broadcast_to(inp["empty"], (B, 77, 128)))):     # device, host, batched
        out, aux = net(dev(inp["x"]), expand_t(CC.T_VAL, B), dev(inp["ctx"]), cfg_scale=CC.S_BIG, empty_context=empty)
        assert aux is None and out.shape == (B, 4, 16, 16) and out.dtype == torch.float32
        err = CC.module_err(out.cpu().numpy(), ref, vc, vu)
        print(f"mid_t2i guided vs oracle: {err:.3e} (bound {CC.module_bound(CC.S_BIG):.2f})")
        assert err <= CC.module_bound(CC.S_BIG)
    plain, _ = net(dev(inp["x"]), expand_t(CC.T_VAL, B), dev(inp["ctx"]))
    assert CC.module_err(plain.cpu().numpy(), ref, vc, vu) > 3 * CC.module_bound(CC.S_BIG)
    zero, _ = net(dev(inp["x"]), expand_t(CC.T_VAL, B), dev(inp["ctx"]), cfg_scale=0.0, empty_context=dev(inp["empty"]))
    assert rel_l2(zero.cpu().numpy(), plain.cpu().numpy()) < 2e-3            # s = 0: the conditional prediction (of the 2B-row forward)
    half, _ = net(dev(inp["x"]).half(), expand_t(CC.T_VAL, B), dev(inp["ctx"]), cfg_scale=CC.S_CFG, empty_context=dev(inp["empty"]))
    assert half.dtype == torch.float16
    assert net(dev(inp["x"])[:0], expand_t(CC.T_VAL, 0), dev(inp["ctx"])[:0], cfg_scale=CC.S_CFG, empty_context=dev(inp["empty"]))[0].shape == (0, 4, 16, 16)


def test_per_sample_scales_are_the_scalar_calls_row_by_row():
    B = 3
    inp = CC.inputs("mid_t2i", B)
    net = gpu_net("mid_t2i")
    x, t, ctx, empty = dev(inp["x"]), expand_t(CC.T_VAL, B), dev(inp["ctx"]), dev(inp["empty"])
    for sweep in (list(CC.SWEEP), np.array(CC.SWEEP), torch.tensor(CC.SWEEP), torch.tensor(CC.SWEEP).cuda()):
        rows, _ = net(x, t, ctx, cfg_scale=sweep, empty_context=empty)
        for b, s in enumerate(CC.SWEEP):
            one, _ = net(x, t, ctx, cfg_scale=s, empty_context=empty)
            assert torch.equal(rows[b], one[b]), (type(sweep), b)
    assert not torch.equal(rows[1], rows[2]) and len(net._cfg_workspace) == 1


# ------------------------------------------------------------------------------------------------------------------ p2p
def test_p2p_edit_under_guidance_acts_on_the_conditional_branch():
    from uspace_amd import _hip
    from uspace_amd.tools import utils_t2i
    B, s = 3, CC.S_CFG
    inp = CC.inputs("mid_t2i", B)
    net = gpu_net("mid_t2i")
    x, ctx, empty = dev(inp["x"]), dev(inp["ctx"]), dev(inp["empty"])
    kw = dict(dissect_name="p2p", fm_direction="decode", t_edit=0.5, block_id="all",
              token_kwargs=dict(token_dissect="p2p_rescale", p2p_multiplier=8.0),
              target_context_ids=[np.array([3, 5]), np.array([], dtype=np.int64), np.array([0, 76])])
    edited, _ = net(x, expand_t(0.3, B), ctx, cfg_scale=s, empty_context=empty, _t_host=0.3, **kw)
    unedited, _ = net(x, expand_t(0.3, B), ctx, cfg_scale=s, empty_context=empty)
    # the composition of (B): the plain forward at 2B rows under the table extended with ones, then the combine kernel
    table = utils_t2i.key_scale_table(net.depth + 1, B, net.seq_len, "0.30", kw)
    assert table is not None and table.shape == (net.depth + 1, B, net.seq_len)
    ks = dev(np.concatenate([table, np.ones_like(table)], axis=1))
    pair = net._run(torch.cat([x, x]), expand_t(0.3, 2 * B), context=torch.cat([ctx, empty[None].expand(B, -1, -1)]), key_scale=ks)
    assert torch.equal(edited, _hip.cfg_combine(pair, s))
    r = rel_l2(edited.cpu().numpy(), unedited.cpu().numpy())
    print(f"p2p under guidance: rel-L2 to the unedited guided result {r:.3e}")
    assert r > 1e-4
    assert torch.equal(edited[1], unedited[1])                                # sample 1 edits no token
    # the unconditional branch is the unedited one's
    unc = net._run(x, expand_t(0.3, B), context=ctx, key_scale=ks, cfg=(empty, False, s, None, True))[1][B:]
    unc0 = net._run(x, expand_t(0.3, B), context=ctx, cfg=(empty, False, s, None, True))[1][B:]
    assert torch.equal(unc, unc0)
    late, _ = net(x, expand_t(0.7, B), ctx, cfg_scale=s, empty_context=empty, _t_host=0.7, **kw)      # t > t_edit
    late0, _ = net(x, expand_t(0.7, B), ctx, cfg_scale=s, empty_context=empty)
    assert torch.equal(late, late0)


# ------------------------------------------------------------------------------------------------------------------ class-conditional
def test_class_conditional_module_matches_the_guided_oracle():
    """TINY with 11 classes (label 10 the empty class, the default), s = 7.5.  Measured on an MI355X: 0.109 against the bound 0.16
    (the 16 times sharper attention of this net costs the bf16 forward more than the plain init does)."""
    B = 3
    sd, inp, vc, vu = CC.oracle_case("tiny_cls", B)
    assert CC.guidance_is_visible(vc, vu, CC.S_BIG)
    net = gpu_net("tiny_cls")
    x, t, y = dev(inp["x"]), expand_t(CC.T_VAL, B), dev(inp["y"])
    ref = CC.guided_reference(vc, vu, CC.S_BIG)
    out, aux = net(x, t, y, cfg_scale=CC.S_BIG, edit_loc=None)
    err = CC.module_err(out.cpu().numpy(), ref, vc, vu)
    print(f"tiny_cls guided vs oracle: {err:.3e} (bound {CC.module_bound(CC.S_BIG):.2f})")
    assert aux is None and err <= CC.module_bound(CC.S_BIG)
    explicit, _ = net(x, t, y, cfg_scale=CC.S_BIG, empty_label=10, edit_loc=None)
    assert torch.equal(out, explicit)
    other, _ = net(x, t, y, cfg_scale=CC.S_BIG, empty_label=3, edit_loc=None)
    assert not torch.equal(out, other)
    plain, _ = net(x, t, y, edit_loc=None)
    assert CC.module_err(plain.cpu().numpy(), ref, vc, vu) > 3 * CC.module_bound(CC.S_BIG)
    sweep, _ = net(x, t, y, cfg_scale=list(CC.SWEEP), edit_loc=None)
    assert torch.equal(sweep[2], out[2])


def test_class_conditional_hooks_under_guidance():
    """A mid write hook reaches both branches, with per-sample write scales on both rows of a sample; head edits x before it is
    paired; tail acts on the guided result; a mid read raises.  s = 0.4: bound (1 + 0.8) 1e-2.  Measured on an MI355X for the mid
    write: 1.54e-2 (a hook that reached the conditional branch only: 0.22 on the oracle)."""
    name, B, s, tv = "tiny_cls", 3, CC.S_CFG, 0.2
    sd, inp, _, _ = CC.oracle_case(name, B)
    net = gpu_net(name)
    x, t, y = dev(inp["x"]), expand_t(tv, B), dev(inp["y"])
    rng = np.random.default_rng(5)
    scales = [0.5, 1.0, -1.0]
    bound = CC.module_bound(s)
    with tempfile.TemporaryDirectory() as d:
        np.save(os.path.join(d, "delta_0.20.npy"), (0.5 * rng.standard_normal((3, net.seq_len, net.embed_dim))).astype(np.float32))
        base = dict(edit_loc="mid", dissect_task="uspace_uvit", dissect_name="write_attr", t_edit=0.4, write_path_root=d, ith_attr=1)
        c0, u0 = CC.oracle_pair_at(name, sd, inp, inp["x"], tv)
        # scalar write scale: the oracle with the hook on both branches
        c1, u1 = CC.oracle_pair_at(name, sd, inp, inp["x"], tv, write_scale=1.0, **base)
        ref = CC.guided_reference(c1, u1, s)
        assert CC.module_err(CC.guided_reference(c0, u0, s), ref, c1, u1) > 3 * bound        # the hook is visible ...
        assert CC.module_err(CC.guided_reference(c1, u0, s), ref, c1, u1) > 3 * bound        # ... and so is one that misses the unconditional branch
        out, _ = net(x, t, y, cfg_scale=s, write_scale=1.0, **base)
        err = CC.module_err(out.cpu().numpy(), ref, c1, u1)
        print(f"tiny_cls mid write under guidance: {err:.3e} (bound {bound:.3f})")
        assert err <= bound
        # one write scale per sample: each sample's two rows take its scale
        rows, _ = net(x, t, y, cfg_scale=s, write_scale=scales, **base)
        for b, ws in enumerate(scales):
            one = {k: (v[b:b + 1] if isinstance(v, np.ndarray) else v) for k, v in inp.items()}
            cb, ub = CC.oracle_pair_at(name, sd, one, inp["x"][b:b + 1], tv, write_scale=ws, **base)
            assert CC.module_err(rows[b:b + 1].cpu().numpy(), CC.guided_reference(cb, ub, s), cb, ub) <= bound, b
        assert torch.equal(rows[1], out[1])
        with pytest.raises(ValueError, match="mid read"):
            net(x, t, y, cfg_scale=s, edit_loc="mid", dissect_task="uspace_uvit", dissect_name="read", read_path_root=os.path.join(d, "rd"),
                batch_id=0)
        assert not os.path.exists(os.path.join(d, "rd"))
        # head: x is edited first, both branches see the edited x; tail: the guided result is edited and read
        di = os.path.join(d, "img")
        os.makedirs(di)
        np.save(os.path.join(di, "delta_0.20.npy"), (0.5 * rng.standard_normal((3, 4, 16, 16))).astype(np.float32))
        img = dict(base, write_scale=1.0, write_path_root=di)
        for loc in ("head", "tail"):
            kw = dict(img, edit_loc=loc)
            ch, uh = CC.oracle_pair_at(name, sd, inp, inp["x"], tv, **kw)
            if loc == "tail":                     # the oracle adds the delta to each branch; on the guided result it is added once
                delta = ch - c0
                ref = CC.guided_reference(c0, u0, s) + delta
            else:
                ref = CC.guided_reference(ch, uh, s)
            got, _ = net(x, t, y, cfg_scale=s, **kw)
            assert CC.module_err(got.cpu().numpy(), ref, c0, u0) <= bound, loc
            assert CC.module_err(CC.guided_reference(c0, u0, s), ref, c0, u0) > 3 * bound, loc
        rd = os.path.join(d, "rd_tail")
        got, _ = net(x, t, y, cfg_scale=s, edit_loc="tail", dissect_task="uspace_uvit", dissect_name="read", read_path_root=rd, batch_id=4)
        np.testing.assert_array_equal(np.load(os.path.join(rd, "4_0.20.npy")), got.cpu().numpy())
        rd = os.path.join(d, "rd_head")
        net(x, t, y, cfg_scale=s, edit_loc="head", dissect_task="uspace_uvit", dissect_name="read", read_path_root=rd, batch_id=1)
        np.testing.assert_array_equal(np.load(os.path.join(rd, "1_0.20.npy")), inp["x"])


# ------------------------------------------------------------------------------------------------------------------ solve
def test_cnf_euler_decode_follows_the_guided_oracle_field():
    """CNF.decode, four Euler steps, cfg_scale = 0.4, TINY T2I against the oracle solver over the guided oracle field:
    rel-L2 < (1 + 0.8) 1e-2.  Measured on an MI355X: 1.7e-4."""
    from oracle import odeint_oracle as OO
    from uspace_amd.flow_matching_t2i import CNF
    name, B, s = "tiny_t2i", 3, CC.S_CFG
    sd, inp, _, _ = CC.oracle_case(name, B)
    net = gpu_net(name)
    cnf = CNF(net)
    got = cnf.decode(dev(inp["x"]), dev(inp["ctx"]), cfg_scale=s, empty_context=dev(inp["empty"]), dissect_name="none",
                     solver_kwargs=dict(solver="fixed", solver_fix="euler", solver_fix_step=0.25))
    assert cnf.last_stats.nfe == 4

    def field(t, yy):
        vc, vu = CC.oracle_pair_at(name, sd, inp, yy, t)
        return CC.guided_reference(vc, vu, s).astype(np.float32)

    ref = OO.solve(field, inp["x"], 0.0, 1.0, method="euler", step_size=0.25)
    r = rel_l2(got.cpu().numpy(), ref)
    print(f"euler-4 guided decode vs oracle: rel-L2 {r:.3e}")
    assert r < CC.module_bound(s)


# ------------------------------------------------------------------------------------------------------------------ the plain path
def test_unguided_path_is_untouched():
    B = 3
    inp = CC.inputs("tiny_t2i", B)
    net = CC.make("tiny_t2i").to("cuda").eval()                  # a module of its own: its caches are counted
    x, t, ctx, empty = dev(inp["x"]), expand_t(CC.T_VAL, B), dev(inp["ctx"]), dev(inp["empty"])
    net.use_graph = False
    a, _ = net(x, t, ctx)
    b, _ = net(x, t, ctx, cfg_scale=None)
    c, _ = net(x, t, ctx, cfg_scale=None, empty_context=empty)
    assert torch.equal(a, b) and torch.equal(a, c)
    assert len(net._cfg_workspace) == 0 and net._cfg_rows is None
    net.use_graph = True
    first, _ = net(x, t, ctx)
    n = len(net._graphs)
    assert n == 1 and torch.equal(first, a)
    guided, _ = net(x, t, ctx, cfg_scale=CC.S_CFG, empty_context=empty)
    assert len(net._graphs) == n and len(net._cfg_workspace) == 1 and not torch.equal(guided, a)
    net.use_graph = False
    eager, _ = net(x, t, ctx, cfg_scale=CC.S_CFG, empty_context=empty)
    net.use_graph = True
    assert torch.equal(guided, eager)
    replay, _ = net(x, t, ctx)
    assert len(net._graphs) == n and torch.equal(replay, first)
