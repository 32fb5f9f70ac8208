"""float64 restatement of the ArcFace identity tower of csrc/idnet.hip, written from the published architecture (TreB1eN's
InsightFace_Pytorch ``model_irse.py``, eval mode) with torch's CPU float64 F.conv2d: the preprocessing of the ID similarity of
pSp / e4e, the tower stage by stage as ``uspace_idnet_tap`` numbers it, and the similarity.  It holds the model, the cases of the
GPU tests, the planted faults and the tolerances.  Not a test.

All maps are NCHW float64 here (``nhwc`` / ``nchw`` convert).  ``stage(sd, blocks, se, s, x)`` maps the output of stage s - 1 to
stage s: 0 ``input_layer`` (from the preprocessed image), 1 + u unit u, 1 + U the 512-vector before the l2 normalisation.

``faults`` plants numeric mutations for the test that shows the tolerances catch them: "bn_through_padding" (``res_layer.0``
folded into the convolution: the padding carries the batch norm's shift), "prelu_as_relu", "flatten_hwc" (the Linear over a
(y, x, c) flatten), "no_se", "se_mean_over_window" (the SE mean over the first half of the pixels), "shortcut_offset" (the
subsample shortcut taken from pixel 1), "crop_shifted" (the crop one pixel off), "pool_floor_windows" (adaptive windows floor ..
floor instead of floor .. ceil), "no_l2norm", "bn_eps_0"."""
import torch
import torch.nn.functional as F

FAULTS = ("bn_through_padding", "prelu_as_relu", "flatten_hwc", "no_se", "se_mean_over_window", "shortcut_offset", "crop_shifted",
          "pool_floor_windows", "no_l2norm", "bn_eps_0")
WIDTHS = (64, 128, 256, 512)
TINY = (1, 1, 1, 1)
UNIT_BLOCKS = (1, 2, 1, 1)      # units: 0 (64, 64, 2), 1 (64, 128, 2), 2 (128, 128, 1), 3 (128, 256, 2), 4 (256, 512, 2)

# The cases of tests/test_gpu_id_metrics.py.
PREPROCESS_CASES = [(2, 256, 256, True), (1, 512, 512, True), (2, 300, 300, True), (2, 130, 130, False)]     # B, H, W, crop
# unit index in UNIT_BLOCKS, (H, W): the subsample shortcut on an even and an odd size, the convolution shortcut on an odd size, the
# stride-1 unit, the widest channels -- each at B = 1 and 3
UNIT_CASES = [(0, (8, 8)), (0, (7, 7)), (1, (9, 9)), (2, (5, 5)), (4, (4, 4))]
TINY_SIZES = (32, 48, 112)      # blocks TINY through the tap; at 112, B = 3 is 147 rows at the last level: past the convolution's 128-row tile

# Tolerances: each bound is 3 x the worst value an MI355X measured against this restatement over every case of every test that
# uses it, none excluded (the convention of tests/attention_map_cases.py and tests/lpips_stages.py); the measured value and its
# case stand beside it, and in profiles/id_metrics.md.  All are rel-L2 per sample (|got - want| / |want|) except "similarity", an absolute difference.
# tests/test_id_metrics_host.py requires every bound to lie 10 x below the smallest deviation of every planted fault it is to catch.
TOL = {
    "preprocess": 1.6e-7,        # 5.23e-8: 300 x 300 -> 256 -> crop -> 112 (ragged windows), normalize, B = 2
    "input_layer": 3.0e-7,       # 9.91e-8: the low-variance tiny tower at 32, B = 3
    "unit_interior": 1.3e-6,     # 4.24e-7: unit (256, 512, 2) of the tiny tower at 112, B = 3 (147 rows)
    "unit_border": 1.4e-6,       # 4.67e-7: unit (256, 512, 2) of the mode "ir" tower at 32, B = 2
    "head": 1.1e-6,              # 3.63e-7: 512 x 7 x 7 (the tiny tower at 112), B = 3
    "embedding": 6.5e-6,         # 2.16e-6: IR-100 at 112, B = 1 (IR-SE50: 1.38e-6 through the preprocess from 256 x 256)
    "similarity": 2.5e-7,        # 8.20e-8: four PNG pairs of 96 x 96 through the tiny tower at 32
}


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


# ------------------------------------------------------------------------------------------------------------------ cases
def smooth_images(n, h, w, seed):
    """Images in [0, 1]: a 7 x 7 Gaussian field upsampled bilinearly plus 0.1 Gaussian noise, scaled into the range and clamped."""
    g = torch.Generator().manual_seed(seed)
    field = F.interpolate(torch.randn(n, 3, 7, 7, generator=g, dtype=torch.float64), size=(h, w), mode="bilinear", align_corners=False)
    x = field + 0.1 * torch.randn(n, 3, h, w, generator=g, dtype=torch.float64)
    return (0.5 + 0.25 * x).clamp(0, 1).float()


def perturbed(x, amplitude, seed):
    """A copy of x moved by ``amplitude`` times another smooth image's deviation from grey (clamped to [0, 1])."""
    other = smooth_images(x.shape[0], x.shape[2], x.shape[3], seed)
    return (x + amplitude * (other - 0.5)).clamp(0, 1)


def unit_input(B, H, W, C, seed):
    """A unit's input map NCHW fp32: smooth structure plus noise, of the magnitude activations have."""
    g = torch.Generator().manual_seed(seed)
    field = F.interpolate(torch.randn(B, C, 3, 3, generator=g), size=(H, W), mode="bilinear", align_corners=False)
    return field + 0.5 * torch.randn(B, C, H, W, generator=g)


def low_variance(sd, k=1e-3):
    """A copy of a state dict whose batch norms have running variances k times smaller and weights sqrt(k) times smaller: the same
    network up to eps, which now weighs 1e-5 / k against the variances -- the case that exposes a wrong eps."""
    out = {key: v.detach().clone() for key, v in sd.items()}
    for key in sd:
        if key.endswith("running_var"):
            out[key] *= k
            out[key[:-len("running_var")] + "weight"] *= k ** 0.5
    return out


def unit_specs(blocks):
    out, cin = [], 64
    for depth, n in zip(WIDTHS, blocks):
        out.append((cin, depth, 2))
        out += [(depth, depth, 1)] * (n - 1)
        cin = depth
    return out


# ------------------------------------------------------------------------------------------------------------ preprocess
def _pool_matrix(N, O, faults=()):
    P = torch.zeros(O, N, dtype=torch.float64)
    for i in range(O):
        lo = (i * N) // O
        hi = ((i + 1) * N) // O if "pool_floor_windows" in faults else -((-(i + 1) * N) // O)
        hi = max(hi, lo + 1)
        P[i, lo:hi] = 1.0 / (hi - lo)
    return P


def adaptive_pool(x, O, faults=()):
    """adaptive_avg_pool2d to O x O: output i averages inputs floor(i N / O) .. ceil((i + 1) N / O) - 1 (a mean over a rectangle
    is the mean of its rows' means, exactly in this precision)."""
    Py, Px = _pool_matrix(x.shape[2], O, faults), _pool_matrix(x.shape[3], O, faults)
    return torch.einsum("oy,bcyx,px->bcop", Py, x, Px)


def preprocess(x, normalize, crop, out_size, faults=()):
    x = torch.as_tensor(x).double()
    if normalize:
        x = 2 * x - 1
    if crop:
        if tuple(x.shape[2:]) != (256, 256):
            x = adaptive_pool(x, 256, faults)
        d = 1 if "crop_shifted" in faults else 0
        x = x[:, :, 35 + d:223 + d, 32 + d:220 + d]
    return adaptive_pool(x, out_size, faults)


# ----------------------------------------------------------------------------------------------------------------- tower
def _p(sd, key):
    return torch.as_tensor(sd[key]).double()


def bn(sd, prefix, x, faults=()):
    eps = 0.0 if "bn_eps_0" in faults else 1e-5
    shape = (1, -1) + (1,) * (x.dim() - 2)
    s = _p(sd, prefix + ".weight") / torch.sqrt(_p(sd, prefix + ".running_var") + eps)
    return (x - _p(sd, prefix + ".running_mean").reshape(shape)) * s.reshape(shape) + _p(sd, prefix + ".bias").reshape(shape)


def prelu(sd, key, x, faults=()):
    a = _p(sd, key).reshape(1, -1, 1, 1)
    if "prelu_as_relu" in faults:
        a = torch.zeros_like(a)
    return x.clamp(min=0) + a * x.clamp(max=0)


def input_layer(sd, x, faults=()):
    y = F.conv2d(x, _p(sd, "input_layer.0.weight"), None, 1, 1)
    return prelu(sd, "input_layer.2.weight", bn(sd, "input_layer.1", y, faults), faults)


def unit(sd, prefix, x, cin, depth, stride, se, faults=()):
    if cin == depth:
        o = 1 if ("shortcut_offset" in faults and stride > 1 and x.shape[2] % stride == 0 and x.shape[3] % stride == 0) else 0
        sc = x[:, :, o::stride, o::stride]
    else:
        sc = bn(sd, prefix + ".shortcut_layer.1", F.conv2d(x, _p(sd, prefix + ".shortcut_layer.0.weight"), None, stride, 0), faults)
    r = prefix + ".res_layer"
    if "bn_through_padding" in faults:      # what folding res_layer.0 into the convolution computes: the padding is normalised too
        y = F.conv2d(bn(sd, r + ".0", F.pad(x, (1, 1, 1, 1)), faults), _p(sd, r + ".1.weight"), None, 1, 0)
    else:
        y = F.conv2d(bn(sd, r + ".0", x, faults), _p(sd, r + ".1.weight"), None, 1, 1)
    y = prelu(sd, r + ".2.weight", y, faults)
    y = bn(sd, r + ".4", F.conv2d(y, _p(sd, r + ".3.weight"), None, stride, 1), faults)
    if se and "no_se" not in faults:
        if "se_mean_over_window" in faults:
            flat = y.flatten(2)
            m = flat[:, :, :(flat.shape[2] + 1) // 2].mean(2)[:, :, None, None]
        else:
            m = y.mean((2, 3), keepdim=True)
        h = torch.relu(F.conv2d(m, _p(sd, r + ".5.fc1.weight")))
        y = y * torch.sigmoid(F.conv2d(h, _p(sd, r + ".5.fc2.weight")))
    return y + sc


def head(sd, x, faults=()):
    """The 512-vector before the l2 normalisation."""
    y = bn(sd, "output_layer.0", x, faults)
    flat = y.permute(0, 2, 3, 1).flatten(1) if "flatten_hwc" in faults else y.flatten(1)
    return bn(sd, "output_layer.4", flat @ _p(sd, "output_layer.3.weight").T + _p(sd, "output_layer.3.bias"), faults)


def stage(sd, blocks, se, s, x, faults=()):
    """Output of tap stage s from the output of stage s - 1 (stage 0: from the preprocessed image), NCHW float64."""
    x = torch.as_tensor(x).double()
    specs = unit_specs(blocks)
    if s == 0:
        return input_layer(sd, x, faults)
    if s <= len(specs):
        cin, depth, stride = specs[s - 1]
        return unit(sd, f"body.{s - 1}", x, cin, depth, stride, se, faults)
    return head(sd, x, faults)


def embed(sd, blocks, se, x, faults=()):
    """x: the preprocessed image NCHW in [-1, 1] -> embeddings float64 [B, 512] (unit length unless "no_l2norm")."""
    x = torch.as_tensor(x).double()
    for s in range(len(unit_specs(blocks)) + 2):
        x = stage(sd, blocks, se, s, x, faults)
    return x if "no_l2norm" in faults else x / x.norm(dim=1, keepdim=True)


def id_similarity(sd, blocks, se, a, b, input_size=112, crop=True, faults=()):
    """Images a, b [B, 3, H, W] in [0, 1] -> (similarity [B], embeddings of a, of b), float64."""
    ea, eb = (embed(sd, blocks, se, preprocess(t, True, crop, input_size, faults), faults) for t in (a, b))
    return (ea * eb).sum(1), ea, eb


# --------------------------------------------------------------------------------------------------------------- measures
def rel_l2(got, want):
    """|got - want| / |want| per sample (dim 0), float64."""
    got, want = torch.as_tensor(got).double().flatten(1), torch.as_tensor(want).double().flatten(1)
    return (got - want).norm(dim=1) / want.norm(dim=1)


def border_mask(h, w):
    m = torch.zeros(h, w, dtype=torch.bool)
    m[0, :] = m[-1, :] = True
    m[:, 0] = m[:, -1] = True
    return m


def rel_l2_split(got, want):
    """(interior, border) rel-L2 per sample of NCHW maps: the border is the outermost ring of pixels, judged on its own so that a
    border fault cannot hide in a mean.  A map without interior (side <= 2) gives interior = 0."""
    got, want = torch.as_tensor(got).double(), torch.as_tensor(want).double()
    m = border_mask(got.shape[2], got.shape[3])
    out = []
    for sel in (~m, m):
        g, w_ = got[:, :, sel].flatten(1), want[:, :, sel].flatten(1)
        out.append((g - w_).norm(dim=1) / w_.norm(dim=1) if sel.any() else torch.zeros(got.shape[0], dtype=torch.float64))
    return out[0], out[1]
