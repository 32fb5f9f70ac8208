"""Pin the CPU oracle (oracle/) against the golden vectors produced by importing the reference."""
import json
import os
import tempfile

import numpy as np
import pytest

from oracle import uvit_oracle as O
from tests.util import rel_l2

TINY = dict(img_size=16, patch_size=2, in_chans=4, embed_dim=64, depth=2, num_heads=1)
TOL = dict(rtol=2e-5, atol=2e-5)


def _load(golden_dir, name):
    z = np.load(os.path.join(golden_dir, name))
    sd = {k[3:]: z[k] for k in z.files if k.startswith("sd/")}
    return z, sd


def test_tiny_u_outputs_and_taps(golden_dir):
    z, sd = _load(golden_dir, "tiny_u.npz")
    spec = O.UViTSpec(**TINY)
    for i, tv in enumerate(z["tvals"]):
        taps = {}
        out = O.uvit_forward(spec, sd, z["x"], tv, taps=taps, edit_loc=None)
        np.testing.assert_allclose(out, z[f"out{i}"], **TOL)
        if i == 1:
            for k in [f for f in z.files if f.startswith("tap/")]:
                name = k[4:]
                assert name in taps, name
                np.testing.assert_allclose(taps[name], z[k], err_msg=name, **TOL)


def test_tiny_u_cond_label_token_order(golden_dir):
    z, sd = _load(golden_dir, "tiny_u_cond.npz")
    spec = O.UViTSpec(num_classes=10, **TINY)
    assert spec.extras == 2
    taps = {}
    out = O.uvit_forward(spec, sd, z["x"], z["tval"], y=z["y"], taps=taps, edit_loc=None)
    np.testing.assert_allclose(taps["tok"], z["tok"], **TOL)
    np.testing.assert_allclose(out, z["out"], **TOL)


def test_tiny_t2i_outputs_and_taps(golden_dir):
    z, sd = _load(golden_dir, "tiny_t2i.npz")
    spec = O.UViTSpec(t2i=True, clip_dim=64, num_clip_token=77, **TINY)
    assert spec.L == 142
    for i, tv in enumerate(z["tvals"]):
        taps = {}
        out = O.uvit_forward(spec, sd, z["x"], tv, context=z["ctx"], taps=taps)
        np.testing.assert_allclose(out, z[f"out{i}"], **TOL)
        if i == 1:
            for k in [f for f in z.files if f.startswith("tap/")]:
                np.testing.assert_allclose(taps[k[4:]], z[k], err_msg=k, **TOL)


def test_uspace_hook_cases(golden_dir):
    zt, sd = _load(golden_dir, "tiny_u.npz")
    z = np.load(os.path.join(golden_dir, "hooks_u.npz"))
    cases = json.loads(bytes(z["cases_json"]).decode())
    spec = O.UViTSpec(**TINY)
    with tempfile.TemporaryDirectory() as d:
        for ts in ("0.00", "0.20", "0.40", "0.41"):
            np.save(os.path.join(d, f"delta_{ts}.npy"), z["img_attr"])
            np.save(os.path.join(d, f"pca4_{ts}.npy"), z["img_pca"])
        for i, c in enumerate(cases):
            kw = dict(dissect_task="uspace_uvit", t_edit=0.4, write_path_root=d)
            kw.update(c)
            tv = kw.pop("tval")
            out = O.uvit_forward(spec, sd, zt["x"], tv, **kw)
            np.testing.assert_allclose(out, z[f"case{i}"], err_msg=str(c), **TOL)
        # skipped-edit cases equal the plain forward at that t
        plain = O.uvit_forward(spec, sd, zt["x"], 0.41, edit_loc=None)
        np.testing.assert_allclose(z["case7"], plain, **TOL)
        # mid hook (token-shaped delta)
        md = os.path.join(d, "mid")
        os.makedirs(md)
        np.save(os.path.join(md, "delta_0.20.npy"), z["tok_attr"])
        base = dict(dissect_task="uspace_uvit", dissect_name="write_attr", t_edit=0.4,
                    write_path_root=md, edit_loc="mid")
        np.testing.assert_allclose(
            O.uvit_forward(spec, sd, zt["x"], 0.2, ith_attr=2, write_scale=1.0, **base), z["mid0"], **TOL)
        np.testing.assert_allclose(
            O.uvit_forward(spec, sd, zt["x"], 0.2, ith_attr="1_3", write_scale=-0.5, **base), z["mid1"], **TOL)
        # read mode: file name and payload
        rd = os.path.join(d, "rd")
        O.uvit_forward(spec, sd, zt["x"], 0.37, edit_loc="tail", dissect_task="uspace_uvit",
                       dissect_name="read", read_path_root=rd, batch_id=5)
        assert sorted(os.listdir(rd)) == ["5_0.37.npy"]
        np.testing.assert_allclose(np.load(os.path.join(rd, "5_0.37.npy")), z["read_tail"], **TOL)
        with pytest.raises(ValueError):
            O.uvit_forward(spec, sd, zt["x"], 0.2, edit_loc="head", dissect_task="uspace_uvit", dissect_name="bogus")


def test_should_edit_table():
    assert not O.should_edit("0.00", 0.4)
    assert O.should_edit("0.40", 0.4) and not O.should_edit("0.41", 0.4)
    assert O.should_edit("0.40", "every_0.2") and not O.should_edit("0.30", "every_0.2")
    with pytest.raises(ValueError):
        O.should_edit("0.10", "sometimes")
    with pytest.raises(ValueError):
        O.should_edit("0.10", None)


def test_p2p_cases(golden_dir):
    zt, sd = _load(golden_dir, "tiny_t2i.npz")
    z = np.load(os.path.join(golden_dir, "p2p_t2i.npz"))
    cases = json.loads(bytes(z["cases_json"]).decode())
    spec = O.UViTSpec(t2i=True, clip_dim=64, num_clip_token=77, **TINY)
    ids = [z["ids_a0"], z["ids_a1"], z["ids_a2"]]
    outs = []
    for i, c in enumerate(cases):
        kw = dict(c)
        tv = kw.pop("tval")
        kw.pop("ids")
        kw["target_context_ids"] = ids
        out = O.uvit_forward(spec, sd, zt["x"], tv, context=zt["ctx"], **kw)
        np.testing.assert_allclose(out, z[f"case{i}"], err_msg=str(c), **TOL)
        outs.append(out)
    # un-edited variants (encode / lp_* / multiplier 1) equal the flash path at the same t
    plain = O.uvit_forward(spec, sd, zt["x"], 0.3, context=zt["ctx"])
    for i in (4, 6, 7):
        np.testing.assert_allclose(outs[i], plain, rtol=1e-4, atol=1e-5)
    assert np.abs(outs[0] - plain).max() > 1e-4


def test_attribute_directions_match_reference(golden_dir):
    from oracle import attr_oracle as A
    z = np.load(os.path.join(golden_dir, "attr_directions.npz"))
    for tag in ("celeba", "ffhq"):
        got = A.delta_directions(z[f"{tag}_attrs"], z[f"{tag}_feats"])
        np.testing.assert_allclose(got, z[f"{tag}_delta"], rtol=1e-5, atol=1e-6, equal_nan=True)
        assert np.isnan(got[1]).all()                 # attribute 1 has no negative example
    with pytest.raises(ValueError):
        A.delta_directions(np.zeros((4, 7), np.int64), np.zeros((4, 2), np.float32))


def test_vae_decoder_oracle_matches_reference(golden_dir):
    import json
    import torch
    from oracle import vae_oracle as V
    from uspace_amd.libs.autoencoder import FrozenAutoencoderKL
    z = np.load(os.path.join(golden_dir, "vae_decoder_tiny.npz"))
    meta = json.loads(bytes(z["meta_json"]).decode())
    torch.manual_seed(meta["weight_seed"])
    m = FrozenAutoencoderKL(meta["ddconfig"], 4)
    sd = {k: v.numpy() for k, v in m.state_dict().items()}
    assert list(sd.keys()) == meta["keys"]
    taps = {}
    img = V.decode(sd, z["z"], meta["ddconfig"]["ch_mult"], meta["ddconfig"]["num_res_blocks"], taps=taps)
    for k in [f for f in z.files if f.startswith("tap/")]:
        np.testing.assert_allclose(taps[k[4:]], z[k], rtol=2e-4, atol=2e-5, err_msg=k)
    np.testing.assert_allclose(img, z["img"], rtol=2e-4, atol=2e-5)


def test_vae_fp64_stage_reference_matches_reference(golden_dir):
    """oracle/vae_stages.py (float64, stage by stage) against the reference's taps and image: the whole chain from z, and
    single stages started from a reference tap.  Measured: rel-L2 1e-7 ... 9e-7, max error <= 1.3e-6 of the largest value
    (the golden is fp32 arithmetic)."""
    import json
    import torch
    from oracle import vae_stages as S
    from uspace_amd.libs.autoencoder import FrozenAutoencoderKL
    z = np.load(os.path.join(golden_dir, "vae_decoder_tiny.npz"))
    meta = json.loads(bytes(z["meta_json"]).decode())
    torch.manual_seed(meta["weight_seed"])
    sd = FrozenAutoencoderKL(meta["ddconfig"], 4).state_dict()
    spec = S.Spec.from_ddconfig(meta["ddconfig"], meta["scale_factor"])
    assert [(k, h, c) for k, _, h, c in spec.stages] == [("conv_in", 8, 128), ("res", 8, 128), ("attn", 8, 128)] + \
        [("res", 8, 128)] * 3 + [("upsample", 16, 128), ("res", 16, 64), ("res", 16, 64)]

    def close(got, want, what):
        got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
        assert got.shape == want.shape, what
        err = np.abs(got - want).max() / np.abs(want).max()
        assert err < 5e-6 and rel_l2(got, want) < 3e-6, (what, err, rel_l2(got, want))

    taps = {}
    img = S.decode(spec, sd, z["z"], taps=taps)
    assert img.dtype == torch.float64
    for name, k in dict(conv_in=0, attn=2, up1_us=6, up0_b0=7, norm_out="norm_out").items():
        close(taps[k], z["tap/" + name], name)
    close(img, z["img"], "img")
    # each stage stands alone: input map + state_dict -> output map
    close(S.run_stage(spec, sd, 7, z["tap/up1_us"]), z["tap/up0_b0"], "stage 7 from up1_us")
    h = z["tap/attn"]
    for k in range(3, 7):
        h = S.run_stage(spec, sd, k, h)
    close(h, z["tap/up1_us"], "stages 3-6 from attn")
    close(S.run_stage(spec, sd, 0, z["z"]), z["tap/conv_in"], "stage 0")
    # the bf16-operand mode rounds where the kernels do: close to, but measurably off, the fp32 reference
    r = rel_l2(S.decode(spec, sd, z["z"], bf16=True), z["img"])
    assert 1e-4 < r < 3e-2, r


def test_clip_text_oracle_matches_hf_module(golden_dir):
    """libs/clip.py:85-88: CLIPTextModel(input_ids).last_hidden_state (HF transformers, tiny random-init config)."""
    import json
    from oracle import clip_oracle as K
    z = np.load(os.path.join(golden_dir, "clip_text_tiny.npz"))
    meta = json.loads(bytes(z["meta_json"]).decode())
    sd = {k[3:]: z[k] for k in z.files if k.startswith("sd/")}
    hidden = []
    out = K.text_forward(sd, z["ids"], meta["num_attention_heads"], eps=meta["layer_norm_eps"], hidden=hidden)
    assert len(hidden) == meta["num_hidden_layers"] + 1
    for i, h in enumerate(hidden):
        np.testing.assert_allclose(h, z[f"hidden/{i}"], rtol=2e-4, atol=2e-5, err_msg=f"hidden {i}")
    np.testing.assert_allclose(out, z["out"], rtol=2e-4, atol=2e-5)


def test_pca_oracle_matches_reference(golden_dir):
    """tools/utils_vis.py:80-118 (sklearn PCA, full SVD) on the fixture activations: same directions, up to sklearn's
    sign convention (which moved between u- and v-based across versions, so compare up to sign)."""
    from oracle import pca_oracle as P
    z = np.load(os.path.join(golden_dir, "pca_components.npz"))
    got = P.pca_components(z["feats"], int(z["n_components"]))
    ref = z["components"]
    assert got.shape == ref.shape
    for g, r in zip(got.reshape(len(got), -1), ref.reshape(len(ref), -1)):
        s = np.sign(np.dot(g, r))
        np.testing.assert_allclose(g * s, r, atol=2e-5)


def hooked_delta_table(k, shape=(5, 4, 16, 16)):
    """tests/golden/make_golden.py::hooked_delta_table: the table of delta_{k/100:.2f}.npy (a different one for every time)."""
    return (np.random.default_rng(4000 + k).standard_normal(shape) * 0.3).astype(np.float32)


def write_hooked_tables(d, shape=(5, 4, 16, 16)):
    for k in range(0, 101):
        np.save(os.path.join(d, f"delta_{k / 100:.2f}.npy"), hooked_delta_table(k, shape))


HOOKED_MID = dict(edit_loc="mid", ith_attr="1_3", write_scale=6.0)          # token-shaped tables [5, 65, 64]: documented semantics


HOOKED_U = (("tail", dict(edit_loc="tail", ith_attr=2, write_scale=1.0)), ("head", dict(edit_loc="head", ith_attr="1_3", write_scale=-4.0)))
HOOKED_T = dict(dissect_name="p2p", t_edit=0.5, block_id=[1], token_kwargs=dict(token_dissect="p2p_rescale", p2p_multiplier=40.0))
HOOKED_T_IDS = [np.array([3, 5], dtype=np.int64), np.array([], dtype=np.int64), np.array([0, 76, 76], dtype=np.int64)]


def test_hooked_trajectories_follow_the_reference(golden_dir, monkeypatch):
    """Hook x solver interplay pinned by the REFERENCE (VERDICT r3 task 4): hooked_traj.npz holds whole solves driven through the
    reference networks with the reference's own hooks active (generator: make_golden.py::make_hooked_traj).  The oracle's
    integrator + forward + hooks must land on the same end states AND edit in the same evaluations: 40 of 100 Euler steps on the
    fp32 grid k * 0.01 (files delta_0.01 ... delta_0.40: "0.00" never edits, 0.29999998 reads delta_0.30), and for the attention-map
    hook none of the 20 encode evaluations and 11 of the 20 decode evaluations (t = 0.00 ... 0.50; no "0.00" rule there)."""
    from oracle import odeint_oracle as OO
    z = np.load(os.path.join(golden_dir, "hooked_traj.npz"))
    zt, sd = _load(golden_dir, "tiny_u.npz")
    spec = O.UViTSpec(**TINY)
    tol = dict(rtol=2e-4, atol=2e-4)               # 100 steps of fp32 round-off on O(1) states
    with tempfile.TemporaryDirectory() as d:
        write_hooked_tables(d)
        files = []
        real_load = np.load
        monkeypatch.setattr(O.np, "load", lambda p, *a, **k: (files.append(os.path.basename(str(p))), real_load(p, *a, **k))[1])
        for tag, kw in HOOKED_U:
            files.clear()
            kwargs = dict(dissect_task="uspace_uvit", dissect_name="write_attr", t_edit=0.4, write_path_root=d, **kw)
            cnt = {}
            x1 = OO.solve(lambda t, y: O.uvit_forward(spec, sd, y, t, **kwargs), zt["x"], 0.0, 1.0, method="euler", step_size=0.01, counters=cnt)
            assert cnt["nfe"] == 100
            assert files == json.loads(bytes(z[f"u_{tag}_files"]).decode()) == [f"delta_{k / 100:.2f}.npy" for k in range(1, 41)]
            np.testing.assert_allclose(x1, z[f"u_{tag}_x1"], **tol)
            assert np.abs(z[f"u_{tag}_x1"] - z["u_plain_x1"]).max() > 0.02          # the edits moved the end state by 100x the tolerance
        monkeypatch.undo()
    # mid block (documented semantics: the reference's reader cannot take token-shaped tables; its should_edit() and file naming
    # decided per evaluation in the generator): same 40 evaluations, token-shaped tables of their own
    with tempfile.TemporaryDirectory() as d:
        write_hooked_tables(d, (5, 65, 64))
        files = []
        real_load = np.load
        monkeypatch.setattr(O.np, "load", lambda p, *a, **k: (files.append(os.path.basename(str(p))), real_load(p, *a, **k))[1])
        kwargs = dict(dissect_task="uspace_uvit", dissect_name="write_attr", t_edit=0.4, write_path_root=d, **HOOKED_MID)
        x1 = OO.solve(lambda t, y: O.uvit_forward(spec, sd, y, t, **kwargs), zt["x"], 0.0, 1.0, method="euler", step_size=0.01)
        assert files == [f"delta_{k / 100:.2f}.npy" for k in range(1, 41)]
        np.testing.assert_allclose(x1, z["u_mid_x1"], **tol)
        monkeypatch.undo()
    zt2, sd2 = _load(golden_dir, "tiny_t2i.npz")
    spec2 = O.UViTSpec(t2i=True, clip_dim=64, num_clip_token=77, **TINY)
    fired = []
    real = O.p2p_column_scale
    monkeypatch.setattr(O, "p2p_column_scale", lambda B, L, t, kw, blk: (lambda r: (fired.append(blk) if r is not None else None, r)[1])(real(B, L, t, kw, blk)))

    def field(direction):
        return lambda t, y: O.uvit_forward(spec2, sd2, y, t, context=zt2["ctx"], fm_direction=direction, target_context_ids=HOOKED_T_IDS, **HOOKED_T)
    z_enc = OO.solve(field("encode"), zt2["x"], 1.0, 0.0, method="euler", step_size=0.05)
    n_enc = len(fired)
    x_dec = OO.solve(field("decode"), z["t_z_enc"], 0.0, 1.0, method="euler", step_size=0.05)
    assert [n_enc, len(fired) - n_enc] == z["t_edit_calls"].tolist() == [0, 11] and set(fired) == {1}
    np.testing.assert_allclose(z_enc, z["t_z_enc"], **tol)
    np.testing.assert_allclose(x_dec, z["t_x_dec"], **tol)
    assert np.abs(z["t_x_dec"] - z["t_x_dec_plain"]).max() > 2e-3


ADAPTIVE_HOOK = dict(dissect_task="uspace_uvit", dissect_name="write_attr", t_edit=0.4, edit_loc="tail", ith_attr=2, write_scale=1.0)


def test_hooked_fixadp_follows_the_reference(golden_dir, monkeypatch):
    """adaptive_traj.npz (make_golden.py::make_adaptive_traj): the reference's tiny U-ViT with its own write_attr hook live, solved
    the fixadp way of every dissection config -- Euler 0.01 up to t_edit = 0.4, then dopri5 rtol = atol = 1e-5 -- by the oracle
    solver.  The oracle forward + hook must edit in the same evaluations (the dopri5 stage at t = 0.4048 formats to "0.40" and
    edits; the probe at 0.415 does not), take the same attempts and land on the same end state."""
    from oracle import odeint_oracle as OO
    z = np.load(os.path.join(golden_dir, "adaptive_traj.npz"))
    zt, sd = _load(golden_dir, "tiny_u.npz")
    spec = O.UViTSpec(**TINY)
    np.testing.assert_array_equal(z["tiny_fixadp_z"], zt["x"])
    with tempfile.TemporaryDirectory() as d:
        write_hooked_tables(d)
        files, ts, edited = [], [], []
        real_load = np.load
        monkeypatch.setattr(O.np, "load", lambda p, *a, **k: (files.append(os.path.basename(str(p))), real_load(p, *a, **k))[1])
        kwargs = dict(ADAPTIVE_HOOK, write_path_root=d)

        def f(t, y):
            n = len(files)
            ts.append(t)
            v = O.uvit_forward(spec, sd, y, t, **kwargs)
            edited.append(len(files) > n)
            return v

        cnt_fix, cnt = {}, {"t_accepted": []}
        mid = OO.solve(f, zt["x"], 0.0, 0.4, method="euler", step_size=0.01, counters=cnt_fix)
        x1 = OO.solve(f, mid, 0.4, 1.0, method="dopri5", rtol=1e-5, atol=1e-5, counters=cnt)
        monkeypatch.undo()
    assert cnt_fix["nfe"] == 40
    assert edited == z["tiny_fixadp_edited"].tolist()
    assert edited[40:43] == [True, False, True]              # f0 at 0.40, probe at 0.415 ("0.42"), stage 1 at 0.4048 ("0.40")
    assert (cnt["nfe"], cnt["accepted"], cnt["rejected"]) == (int(z["tiny_fixadp_nfe_adaptive"]), int(z["tiny_fixadp_accepted"]),
                                                               int(z["tiny_fixadp_rejected"]))
    # every time up to the last attempt; that attempt's dt comes from an error ratio at the round-off floor of an almost linear
    # field (it steps from 0.72 to 2.7, past t1, and the dense output lands on 1.0), so its size differs by a few percent
    np.testing.assert_allclose(ts[:-6], z["tiny_fixadp_t_eval"][:-6], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(cnt["t_accepted"][:-1], z["tiny_fixadp_t_accepted"][:-1], rtol=1e-5)
    np.testing.assert_allclose(x1, z["tiny_fixadp_x1"], rtol=2e-4, atol=2e-4)
