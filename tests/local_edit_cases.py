"""Local edits, shared by tests/test_local_edit_host.py and tests/test_gpu_local_edit.py: the case lists of the three kernels of
csrc/local_edit.hip, their numpy / float64 references, the reference of a blended Euler solve, one wrong implementation per planted
fault (``PERTURBED``), and the bounds (``TOL``).

The blend: out[B + b] = s where m <= 0 or m is NaN, e where m >= 1, otherwise fmaf(m, e - s, s) in fp32 (s = pair[b], e = pair[B + b]).
A mask from labels is exact (integer counts, one fp32 division).  A mask from maps sums in fp32 in a fixed order; its reference is
float64."""
import functools
import os
import tempfile

import numpy as np
import torch

# ------------------------------------------------------------------------------------------------------------------ bounds
# blend_ulp: |got - ref64| in ulps of the float64 value rounded to fp32, where s and e have one sign and lie within a factor 2 of each
#   other: e - s is then exact (Sterbenz), the fused multiply-add rounds once, and the result is the correctly rounded value (0.5 ulp;
#   the bound of 1 ulp is the issue's).  On arbitrary operands 1 ulp of the RESULT is not derivable: s = 1, e = -1.0000001, m = 0.5
#   gives a result of -6e-8 whose fp32 subtraction alone was rounded by 6e-8.  There the bound is the derived one, blend_general:
#   |got - ref64| <= 2^-24 (m |e - s| + |ref64|) -- the rounding of e - s carried through the product, and the rounding of the fma.
# maps_soft: max |soft - ref64| of the normalised value (<= 1) over the case MAPS_TOL_CASE, the one with the longest sums; 3 x the worst
#   value measured on the MI355X (1.511e-7), below the a-priori n_blocks * nk * 2^-24 = 7.8e-5 of that case.
# solve_rel_l2: rel-L2 of ``edited`` of the Euler solve SOLVE_CASE against the CPU oracle's blended solve; 3 x the value measured on the
#   MI355X (1.874e-4), capped by the 1e-2 tests/test_gpu_uvit_long.py::test_euler_solve_matches_the_oracle_solve allows such a solve.
MAPS_TOL_CASE = (17, 4, 16, 77, 2)
TOL = {
    "blend_ulp": 1.0,
    "blend_general": 2.0 ** -24,
    "maps_soft": 4.54e-7,
    "solve_rel_l2": 5.63e-4,
}
SOLVE_CAP = 1e-2
MAPS_EXCUSED_SHARE = 0.01          # of the cells of a binary mask may lie within maps_soft of the threshold


def maps_apriori(case):
    n_blocks, _R, _G, nk, _patch = case
    return n_blocks * nk * 2.0 ** -24


# ------------------------------------------------------------------------------------------------------------------ pair_blend
# (B, C, cells): one element; odd cells (scalar form); cells % 4 != 0 with C = 4; the 16-byte form; more than one workgroup
BLEND_SHAPES = [(1, 4, 1), (2, 3, 49), (2, 4, 25), (3, 4, 256), (5, 4, 1024)]
BLEND_EXACT_M = (0.0, 1.0, float("nan"), -0.5, 1.5)


def blend_inputs(shape, seed=0, near=False):
    """pair fp32 [2B, C, cells] and mask fp32 [B, cells]: a third of the cells 0, a third 1, the rest inside (0, 1).  ``near``: s and e
    of one sign within a factor 2 (the operands of the 1-ulp bound)."""
    B, C, cells = shape
    rng = np.random.default_rng(1000 * cells + 10 * B + C + seed)
    if near:
        s = (1.0 + rng.random((B, C, cells))) * np.where(rng.random((B, C, cells)) < 0.5, -1.0, 1.0) * np.exp2(rng.integers(-6, 7, (B, C, cells)))
        e = s * (0.5 + 1.5 * rng.random((B, C, cells)))
        pair = np.concatenate([s, e]).astype(np.float32)
    else:
        pair = (rng.standard_normal((2 * B, C, cells)) * np.exp(rng.standard_normal((2 * B, C, cells)))).astype(np.float32)
    kind = rng.integers(0, 3, (B, cells))
    mask = np.where(kind == 0, 0.0, np.where(kind == 1, 1.0, rng.random((B, cells)))).astype(np.float32)
    return pair, mask


def blend_reference(pair, mask):
    """float64, of ``pair``'s shape [2B, C, ...]: rows [0, B) the source rows, rows [B, 2B) the blend."""
    shape = np.shape(pair)
    p = np.asarray(pair, np.float64).reshape(shape[0], shape[1], -1)
    B = p.shape[0] // 2
    s, e = p[:B], p[B:]
    m = np.asarray(mask, np.float64).reshape(B, 1, -1)
    with np.errstate(invalid="ignore"):
        out = np.where(m >= 1, e, np.where(~(m > 0), s, s + m * (e - s)))
    return np.concatenate([s, out]).reshape(shape)


def ulps(got, ref64):
    """|got - ref64| in units of the fp32 spacing at ref64."""
    r32 = np.asarray(ref64, np.float64).astype(np.float32)
    sp = np.spacing(np.abs(r32)).astype(np.float64)
    return np.abs(np.asarray(got, np.float64) - np.asarray(ref64, np.float64)) / sp


def blend_general_bound(pair, mask):
    p = np.asarray(pair, np.float64)
    B = p.shape[0] // 2
    m = np.clip(np.nan_to_num(np.asarray(mask, np.float64), nan=0.0), 0.0, 1.0).reshape(B, 1, -1)
    return TOL["blend_general"] * (m * np.abs(p[B:] - p[:B]) + np.abs(blend_reference(pair, mask)[B:]))


# ------------------------------------------------------------------------------------------------------------------ mask_from_labels
NUM_LABELS = 19
REGION = (1, 4, 5, 17)
# (B, H, W, S, dilate): H = W = S (a cell is one pixel); S = 1; H = 8 S; H != W both ways; B up to 3; dilate 0, 1, 2
LABEL_CASES = [(1, 4, 4, 4, 0), (2, 16, 16, 16, 1), (1, 8, 8, 1, 0), (2, 128, 128, 16, 2), (3, 32, 64, 4, 1), (3, 64, 32, 16, 2),
               (1, 16, 16, 4, 2), (2, 32, 32, 16, 0)]
LABEL_THRESHOLDS = (0.0, 0.5)


def member_of(region=REGION):
    m = np.zeros(256, np.uint8)
    m[list(region)] = 1
    return m


def label_maps(case, seed=0):
    """uint8 [B, H, W]: noise over all 256 values (labels above the set among them) with a block of a region label in a corner -- the
    top-left one for even samples, the bottom-right one for odd ones -- so that the region touches the border and samples differ."""
    B, H, W, S, dilate = case
    rng = np.random.default_rng(7 * H + W + S + seed)
    lab = rng.integers(0, 256, (B, H, W)).astype(np.uint8)
    lab[np.isin(lab, REGION)] = 0                         # the region is only where it is put
    for b in range(B):
        h, w = max(1, (H * (b + 2)) // 5), max(1, (W * (b + 1)) // 4)
        ys, xs = (slice(0, h), slice(0, w)) if b % 2 == 0 else (slice(H - h, H), slice(W - w, W))
        lab[b, ys, xs] = REGION[b % len(REGION)]
        sprinkle = rng.random((H, W)) < 0.3                # partial cells in a band across the middle: shares strictly between 0 and 1
        sprinkle[:H // 2 - H // 8] = False
        sprinkle[H // 2 + max(1, H // 8):] = False
        lab[b][sprinkle] = REGION[0]
    return lab


def _window_max(a, d, wrap=False):
    """Maximum over the (2 d + 1)^2 window of the last two axes, clipped at the border (``wrap``: wrapping round it)."""
    out = a.copy()
    H, W = a.shape[-2:]
    for dy in range(-d, d + 1):
        for dx in range(-d, d + 1):
            if wrap:
                sh = np.roll(a, (dy, dx), axis=(-2, -1))
            else:
                sh = np.full_like(a, -np.inf)
                ys, yd = slice(max(0, -dy), H - max(0, dy)), slice(max(0, dy), H - max(0, -dy))
                xs, xd = slice(max(0, -dx), W - max(0, dx)), slice(max(0, dx), W - max(0, -dx))
                sh[..., yd, xd] = a[..., ys, xs]
            out = np.maximum(out, sh)
    return out


def labels_mask_reference(labels, member, S, dilate, thr, soft, fault=None):
    """fp32 [B, S, S], exact: integer counts, one fp32 division, maxima, one comparison."""
    B, H, W = labels.shape
    ch, cw = H // S, W // S
    inside = member[labels] != 0
    count = inside.reshape(B, S, ch, S, cw).sum(axis=(2, 4)).astype(np.int64)
    denom = S * S if fault == "share_over_S2" else ch * cw
    share = count.astype(np.float32) / np.float32(denom)
    v = _window_max(share, dilate, wrap=fault == "dilation_wraps")
    return v.astype(np.float32) if soft else (v > np.float32(thr)).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ mask_from_maps
# (n_blocks, R, G, nk, patch): G in {1, 8, 16}, patch in {1, 2, 4}, nk in {1, 77}, n_blocks in {1, 3, 17}; R even where the two
# halves stand for the two branches
MAPS_CASES = [(1, 1, 1, 1, 1), (3, 2, 8, 77, 2), MAPS_TOL_CASE, (3, 3, 16, 1, 4), (1, 2, 8, 77, 1), (17, 2, 1, 77, 4)]
MAPS_THR = 0.3


@functools.lru_cache(maxsize=None)
def maps_inputs(case, seed=0):
    """(maps fp32 [n_blocks, R, G * G, nk], block_w fp32 [n_blocks], cols fp32 [R, nk]): attention-like values (positive, of the order
    of 1 / L) with, per row and column, a bump somewhere on the grid -- off the diagonal, in another place for every row, of another
    height for every row; a few chosen columns per row, other ones in the second half of the rows; the LAST row of a case with more
    than two rows has all-zero cols."""
    n_blocks, R, G, nk, patch = case
    rng = np.random.default_rng(n_blocks * 1000 + R * 100 + G * 10 + nk + patch + seed)
    maps = rng.random((n_blocks, R, G * G, nk)) ** 3 / 142.0
    yy, xx = np.mgrid[0:G, 0:G]
    for r in range(R):
        for j in range(nk):
            cy, cx = (2 + 3 * r + j) % G, (5 + 2 * r + 3 * j) % G
            bump = np.exp(-((yy - cy) ** 2 / 6.0 + (xx - cx) ** 2 / 2.0)).reshape(-1)
            maps[:, r, :, j] += (0.02 + 0.015 * r) * bump * (0.5 + rng.random((n_blocks, 1)))
    maps = maps.astype(np.float32)
    block_w = np.ones(n_blocks, np.float32)
    if n_blocks > 1:
        block_w[1] = 0.0                                   # a block left out
    cols = np.zeros((R, nk), np.float32)
    for r in range(R):
        picks = [(3 + 5 * r) % nk, (11 + 7 * r) % nk] if r < (R + 1) // 2 else [(20 + 3 * r) % nk]
        cols[r, picks] = 1.0
    if R > 2:
        cols[R - 1] = 0.0
    for a in (maps, block_w, cols):
        a.setflags(write=False)
    return maps, block_w, cols


def maps_mask_reference(maps, block_w, cols, G, patch, thr, soft, fault=None):
    """(mask float64 [R, G * patch, G * patch], the normalised values float64 of the same shape) of the float64 formula."""
    m = np.asarray(maps, np.float64)
    c = np.asarray(cols, np.float64)
    R = m.shape[1]
    if fault == "cols_wrong_branch":
        c = np.roll(c, R // 2, axis=0)
    a = np.einsum("k,krpj,rj->rp", np.asarray(block_w, np.float64), m, c).reshape(R, G, G)
    pooled = a if fault == "no_maxpool" else _window_max(a, 1)
    top = pooled.reshape(R, -1).max(axis=1)
    if fault == "batch_max":
        top = np.full(R, top.max())
    live = (top > 0) & (np.abs(c).sum(axis=1) > 0)
    norm = np.where(live[:, None, None], pooled / np.where(live, top, 1.0)[:, None, None], 0.0)
    norm = np.repeat(np.repeat(norm, patch, axis=1), patch, axis=2)
    if fault == "patch_transposed":
        norm = np.ascontiguousarray(norm.transpose(0, 2, 1))
    mask = norm if soft else np.where(live[:, None, None], (norm > thr).astype(np.float64), 0.0)
    return mask, norm


def excused(norm, thr, bound):
    """Cells of a binary mask whose reference value lies within ``bound`` of the threshold: either side is right there."""
    return np.abs(norm - thr) <= bound


# ------------------------------------------------------------------------------------------------------------------ the solve
_BASE = dict(img_size=16, patch_size=2, in_chans=4, embed_dim=64, depth=2, num_heads=1, mlp_ratio=4, qkv_bias=False, mlp_time_embed=False)
NETS = {
    "tiny_u": (dict(_BASE, num_classes=-1), False),
    "tiny_t2i": (dict(_BASE, clip_dim=64, num_clip_token=77), True),
}
SEED = 2
STEP = 0.25
SOLVER = dict(solver="fixed", solver_fix="euler", solver_fix_step=STEP)


def make(name):
    from tests import uvit_stages as US
    kw, t2i = NETS[name]
    return US.make_net(dict(kw), kind="workflow", seed=SEED, t2i=t2i)


def spec(name):
    from oracle import uvit_oracle as O
    kw, t2i = NETS[name]
    keep = {k: kw[k] for k in ("img_size", "patch_size", "in_chans", "embed_dim", "depth", "num_heads", "mlp_ratio")}
    if t2i:
        return O.UViTSpec(t2i=True, clip_dim=kw["clip_dim"], num_clip_token=kw["num_clip_token"], **keep)
    return O.UViTSpec(num_classes=kw["num_classes"], **keep)


def solve_inputs(name, B, seed=11):
    kw, t2i = NETS[name]
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, kw["in_chans"], kw["img_size"], kw["img_size"], generator=g).numpy()
    out = dict(z=z)
    if t2i:
        out["ctx"] = torch.randn(B, kw["num_clip_token"], kw["clip_dim"], generator=g).numpy()
        out["ctx_src"] = torch.randn(B, kw["num_clip_token"], kw["clip_dim"], generator=g).numpy()
    return out


def half_plane(B, S=16):
    m = np.zeros((B, S, S), np.float32)
    m[:, :, S // 2:] = 1.0
    return m


def checkerboard(B, S=16, cell=2):
    yy, xx = np.mgrid[0:S, 0:S]
    m = (((yy // cell) + (xx // cell)) % 2).astype(np.float32)
    return np.broadcast_to(m, (B, S, S)).copy()


def soft_bands(B, S=16):
    """0 | 0.5 | 1 in three vertical bands, the bands shifted by one column per sample: a soft mask (where blending the state is not
    blending the velocity) that differs between samples."""
    m = np.zeros((B, S, S), np.float32)
    for b in range(B):
        m[b, :, S // 3 + b:] = 0.5
        m[b, :, (2 * S) // 3 + b:] = 1.0
    return m


def write_deltas(root, shape, digits, seed=5, name="delta"):
    """The direction files of a write hook at the given timestep digits: [3, *shape] each, 0.5 N(0, 1)."""
    rng = np.random.default_rng(seed)
    for d in digits:
        np.save(os.path.join(root, f"{name}_{d}.npy"), (0.5 * rng.standard_normal((3,) + tuple(shape))).astype(np.float32))


EULER_DIGITS = ("0.25", "0.50", "0.75")                   # the evaluations of four Euler steps after t = 0 (a hook never edits at "0.00")


def write_kwargs(root, loc, scale=1.0):
    return dict(edit_loc=loc, dissect_task="uspace_uvit", dissect_name="write_attr", t_edit=1.0, write_path_root=root, ith_attr=1,
                write_scale=scale)


def euler_blend_reference(field_src, field_edit, z, mask, n_steps=4, fault=None):
    """(edited, source) float32 of the blended Euler solve over both branches, both started from ``z``: v_e <- blend(v_s, v_e, mask)
    at every evaluation (float64 blend, fp32 state).  ``field_*(t, x) -> v``.  ``fault="state_blended"``: the plain velocities, and
    the STATE of the edited branch blended after every step."""
    B = z.shape[0]
    xs, xe = z.astype(np.float32).copy(), z.astype(np.float32).copy()
    m = np.asarray(mask, np.float32).reshape(B, -1)
    h = np.float32(1.0 / n_steps)
    for k in range(n_steps):
        t = np.float32(k) * h
        vs, ve = field_src(t, xs), field_edit(t, xe)
        pair = np.concatenate([vs, ve]).reshape(2 * B, z.shape[1], -1)
        if fault == "halves_swapped":
            pair = np.concatenate([pair[B:], pair[:B]])
        if fault != "state_blended":
            ve = blend_reference(pair, m)[B:].reshape(z.shape).astype(np.float32)
        xs = (xs + h * vs).astype(np.float32)
        xe = (xe + h * ve).astype(np.float32)
        if fault == "state_blended":
            st = np.concatenate([xs, xe]).reshape(2 * B, z.shape[1], -1)
            xe = blend_reference(st, m)[B:].reshape(z.shape).astype(np.float32)
    return xe, xs


SOLVE_CASE = ("tiny_u", 2, "tail", "soft_bands")


@functools.lru_cache(maxsize=None)
def oracle_solve(fault=None):
    """``edited`` of SOLVE_CASE on the CPU oracle: a tail write on the edited branch, none on the source, the soft mask.  Computed once
    per fault, shared, never modified."""
    from oracle import uvit_oracle as O
    name, B, loc, _ = SOLVE_CASE
    sp = spec(name)
    sd = {k: v.detach().numpy() for k, v in make(name).state_dict().items()}
    z = solve_inputs(name, B)["z"]
    with tempfile.TemporaryDirectory() as d:
        write_deltas(d, z.shape[1:], EULER_DIGITS)
        kw = write_kwargs(d, loc)
        src = lambda t, x: O.uvit_forward(sp, sd, x, np.float32(t), edit_loc=None)
        edt = lambda t, x: O.uvit_forward(sp, sd, x, np.float32(t), **kw)
        edited, source = euler_blend_reference(src, edt, z, soft_bands(B), fault=fault)
    edited.setflags(write=False)
    return edited


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


# ------------------------------------------------------------------------------------------------------------------ planted faults
def _blend_fault(kind):
    def fn(pair, mask):
        p = np.asarray(pair, np.float64)
        B = p.shape[0] // 2
        if kind == "mask_row_stride":                      # sample b reads the mask of sample b + 1
            return blend_reference(pair, np.roll(np.asarray(mask), -1, axis=0))
        if kind == "mask_channel0_only":                   # the mask is not broadcast over the channels: only channel 0 is blended
            out = blend_reference(pair, mask)
            out[B:, 1:] = p[B:, 1:]
            return out
        if kind == "halves_swapped":
            return blend_reference(np.concatenate([p[B:], p[:B]]), mask)
        raise KeyError(kind)
    return fn


# name -> (which reference it perturbs, the wrong implementation or the ``fault=`` the reference takes)
PERTURBED = {
    "mask_row_stride": ("blend", _blend_fault("mask_row_stride")),
    "mask_channel0_only": ("blend", _blend_fault("mask_channel0_only")),
    "halves_swapped": ("blend", _blend_fault("halves_swapped")),
    "state_blended": ("solve", "state_blended"),
    "share_over_S2": ("labels", "share_over_S2"),
    "dilation_wraps": ("labels", "dilation_wraps"),
    "no_maxpool": ("maps", "no_maxpool"),
    "batch_max": ("maps", "batch_max"),
    "cols_wrong_branch": ("maps", "cols_wrong_branch"),
    "patch_transposed": ("maps", "patch_transposed"),
}
