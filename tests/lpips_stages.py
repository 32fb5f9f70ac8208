"""float64 restatement of the paired metrics of csrc/lpips.hip, written from the math: LPIPS (Zhang et al. 2018) with torch's CPU
float64 F.conv2d / max_pool2d over torchvision's AlexNet / VGG-16 feature stacks, SSIM (Wang et al. 2004) and PSNR in numpy
float64.  It holds the model, the cases of the GPU tests and the planted faults.

scaled(x, normalize) is tap stage 0; stage(sd, net, s, x) maps the output of tap stage s - 1 (NCHW float64) to stage s as
uspace_lpips_tap numbers them (1 .. 5: the five tapped ReLUs); lpips(sd, net, x0, x1) is the whole metric.

``faults`` plants numeric mutations for the tests that show the tolerances catch them.  LPIPS: "no_scaling" (no ScalingLayer),
"tap_before_relu", "ceil_mode" (pooling), "normalize_after_diff" (unit-normalise a - b instead of a and b), "w_before_square"
((w d)^2 instead of w d^2), "ignore_normalize" (the [0, 1] -> [-1, 1] map skipped).  SSIM: "uniform_window" (11 x 11 box),
"sigma_1", "same_padding" (zero padding, H x W map), "k2_0.01"."""
import numpy as np
import torch
import torch.nn.functional as F

SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
EPS = 1e-10
LPIPS_FAULTS = ("no_scaling", "tap_before_relu", "ceil_mode", "normalize_after_diff", "w_before_square", "ignore_normalize")
SSIM_FAULTS = ("uniform_window", "sigma_1", "same_padding", "k2_0.01")

# per tap stage: ("pool", kernel, stride) or ("conv", index in torchvision's features, stride, padding)
PLAN = {
    "alex": [[("conv", 0, 4, 2)], [("pool", 3, 2), ("conv", 3, 1, 2)], [("pool", 3, 2), ("conv", 6, 1, 1)], [("conv", 8, 1, 1)],
             [("conv", 10, 1, 1)]],
    "vgg": [[("conv", 0, 1, 1), ("conv", 2, 1, 1)], [("pool", 2, 2), ("conv", 5, 1, 1), ("conv", 7, 1, 1)],
            [("pool", 2, 2), ("conv", 10, 1, 1), ("conv", 12, 1, 1), ("conv", 14, 1, 1)],
            [("pool", 2, 2), ("conv", 17, 1, 1), ("conv", 19, 1, 1), ("conv", 21, 1, 1)],
            [("pool", 2, 2), ("conv", 24, 1, 1), ("conv", 26, 1, 1), ("conv", 28, 1, 1)]],
}

# the cases of tests/test_gpu_pair_metrics.py
HEAD_CASES = [(B, HW, C) for C in (64, 192, 512) for HW in (1, 9, 225) for B in (1, 3)]
BACKBONE_CASES = [("alex", 3, 64, 64), ("alex", 3, 70, 95), ("vgg", 3, 32, 32), ("vgg", 3, 38, 51), ("alex", 2, 256, 256)]
SSIM_CASES = [(B, 3, H, W) for (H, W) in ((11, 11), (12, 29), (64, 64)) for B in (1, 3)]


def images(n, h, w, seed, c=3):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, c, h, w, generator=g)


def pair(n, h, w, seed, noise=0.1, c=3):
    """Images in [0, 1] and a perturbed copy (clamped uniform noise of the given amplitude)."""
    a = images(n, h, w, seed, c)
    b = (a + noise * (2 * images(n, h, w, seed + 1, c) - 1)).clamp(0, 1)
    return a, b


# --------------------------------------------------------------------------------------------------------------- LPIPS
def scaled(x, normalize=False, faults=()):
    """Tap stage 0: the ScalingLayer applied to x (or to 2 x - 1 with ``normalize``)."""
    x = torch.as_tensor(x).double()
    if normalize and "ignore_normalize" not in faults:
        x = 2 * x - 1
    if "no_scaling" in faults:
        return x
    sh = torch.tensor(SHIFT, dtype=torch.float64)[None, :, None, None]
    sc = torch.tensor(SCALE, dtype=torch.float64)[None, :, None, None]
    return (x - sh) / sc


def _stage(sd, net, s, x, faults=()):
    """(output after the stage's last ReLU, the same before that ReLU)."""
    pre = None
    for op in PLAN[net][s - 1]:
        if op[0] == "pool":
            x = F.max_pool2d(x, op[1], op[2], ceil_mode="ceil_mode" in faults)
        else:
            _, i, stride, pad = op
            w = torch.as_tensor(sd[f"features.{i}.weight"]).double()
            b = torch.as_tensor(sd[f"features.{i}.bias"]).double()
            pre = F.conv2d(x, w, b, stride=stride, padding=pad)
            x = torch.relu(pre)
    return x, pre


def stage(sd, net, s, x, faults=()):
    """Output of tap stage s (1 .. 5) from the output of stage s - 1, float64 NCHW."""
    return _stage(sd, net, s, torch.as_tensor(x).double(), faults)[0]


def distance(f0, f1, w, faults=()):
    """One layer's term: f0, f1 float64 [B, C, H, W], w [C] -> [B]."""
    f0, f1, w = (torch.as_tensor(t).double() for t in (f0, f1, w))
    unit = lambda t: t / (t.pow(2).sum(1, keepdim=True).sqrt() + EPS)
    d = unit(f0 - f1) if "normalize_after_diff" in faults else unit(f0) - unit(f1)
    wc = w[None, :, None, None]
    term = (wc * d).pow(2) if "w_before_square" in faults else wc * d.pow(2)
    return term.sum(1).mean((1, 2))


def lpips(sd, net, x0, x1, normalize=False, faults=()):
    """(total [B], layers [5, B]) float64."""
    B = x0.shape[0]
    x = scaled(torch.cat([torch.as_tensor(x0), torch.as_tensor(x1)]), normalize, faults)
    layers = []
    for s in range(1, 6):
        x, pre = _stage(sd, net, s, x, faults)
        f = pre if "tap_before_relu" in faults else x
        layers.append(distance(f[:B], f[B:], sd[f"lin{s - 1}.weight"], faults))
    layers = torch.stack(layers)
    return layers.sum(0), layers


# -------------------------------------------------------------------------------------------------------- SSIM and PSNR
def window(faults=()):
    if "uniform_window" in faults:
        return np.full(11, 1.0 / 11)
    sigma = 1.0 if "sigma_1" in faults else 1.5
    g = np.exp(-((np.arange(11) - 5.0) ** 2) / (2 * sigma * sigma))
    return g / g.sum()


def _filter_valid(a, g):
    k = len(g)
    H, W = a.shape[-2:]
    t = sum(g[i] * a[..., i:H - k + 1 + i, :] for i in range(k))
    return sum(g[j] * t[..., :, j:W - k + 1 + j] for j in range(k))


def ssim(x, y, data_range=1.0, faults=()):
    """x, y [B, C, H, W] -> float64 [B]: the mean over channels and valid window positions."""
    x, y = (np.asarray(t, np.float64) for t in (x, y))
    if "same_padding" in faults:
        x, y = (np.pad(t, ((0, 0), (0, 0), (5, 5), (5, 5))) for t in (x, y))
    g = window(faults)
    c1 = (0.01 * data_range) ** 2
    c2 = ((0.01 if "k2_0.01" in faults else 0.03) * data_range) ** 2
    mx, my = _filter_valid(x, g), _filter_valid(y, g)
    sxx = _filter_valid(x * x, g) - mx * mx
    syy = _filter_valid(y * y, g) - my * my
    sxy = _filter_valid(x * y, g) - mx * my
    m = ((2 * mx * my + c1) * (2 * sxy + c2)) / ((mx * mx + my * my + c1) * (sxx + syy + c2))
    return m.mean((1, 2, 3))


def psnr(x, y, data_range=1.0):
    x, y = (np.asarray(t, np.float64) for t in (x, y))
    mse = ((x - y) ** 2).reshape(x.shape[0], -1).mean(1)
    with np.errstate(divide="ignore"):
        return 10 * np.log10(data_range ** 2 / mse)
