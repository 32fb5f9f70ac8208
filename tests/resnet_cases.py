"""The networks, the cases and the tolerances of the attribute-classifier tower's tests (tests/test_resnet_host.py,
tests/test_gpu_resnet.py, tests/test_gpu_attr_metrics.py); the float64 model and the planted faults are tests/resnet_stages.py.
Not a test."""
import functools

import numpy as np
import torch

from tests import resnet_stages as R

# Networks: the two golden models (tests/golden/resnet_tiny.npz, what Hugging Face computes) and a seeded bottleneck net whose
# channel counts reach the convolution's other paths: Cin 20, 24 and 40 (no multiple of 16: the gathered K slice), Cout 16 .. 40
# (below the 64-column tile), 96 and 160 (a partial second tile).
SEEDED = R.Arch("bottleneck", (1, 2, 1, 1), (16, 24, 40, 64), 20)
NETS = ("golden_bottleneck", "golden_basic", "seeded")


@functools.lru_cache(maxsize=None)
def net(name):
    """(arch, state dict on the host) of one of NETS."""
    if name.startswith("golden_"):
        arch, sd, _ = R.golden(name[len("golden_"):])
        return arch, sd
    from uspace_amd.libs.resnet import ResNet
    m = ResNet(SEEDED.block, SEEDED.layers, 40, SEEDED.planes, SEEDED.stem, seed=3)
    return SEEDED, {k: v.detach().clone() for k, v in m.state_dict().items()}


def module(name):
    """The ``ResNet`` module of a net, on the host."""
    from uspace_amd.libs.resnet import ResNet
    arch, sd = net(name)
    m = ResNet(arch.block, arch.layers, sd["fc.weight"].shape[0], arch.planes, arch.stem, arch.mean, arch.std)
    m.load_state_dict(sd)
    return m


def images(B, H, W):
    """The images of a case: a function of its sizes alone."""
    return R.smooth_images(B, H, W, 1000 * B + 10 * H + W)


# Image sizes: 40 x 56 (the golden's: non-square, odd sides further down), 64 x 64, 33 x 47 (odd from the start: 17 x 24 after
# conv1, 9 x 12 after the pool).  B in 1, 3, 5: the pixel rows M are no multiple of the 128-row tile (3 x 20 x 28 = 1680 after
# conv1 at 40 x 56, 5 x 9 x 12 = 540 ...), and more than one row tile from B = 1 on.
SIZES = ((40, 56), (64, 64), (33, 47))
BATCHES = (1, 3, 5)
PARITY_CASES = [(n, h, w, b) for n in NETS for h, w in SIZES for b in BATCHES]
# The pooled vector's partial sums are 64 pixels long: a last map of 1 x 1 (one pixel, one chunk) and one of 7 x 10 = 70 pixels
# (a full chunk and a ragged one).
POOL_CASES = [("seeded", 32, 32, 3), ("seeded", 224, 320, 1)]

# Tolerances: each bound is about 3 x the worst value an MI355X measured against the float64 model over every case of every test
# that uses it, none excluded (the convention of tests/attention_map_cases.py); the measured value and its case stand beside it,
# and in profiles/attr_metrics.md.  stem / block / pooled / logits: the worst (sample, stage) rel-L2, |got - want| / |want|, of a
# stage computed from the GPU's own previous stage (the stem from the images, the logits from the GPU's pooled vector); tower: the
# rel-L2 of the logits from the images through the whole tower; effect: the largest absolute difference of target_shift,
# off_target and selectivity from the images end to end.  tests/test_resnet_host.py brackets every bound: at least the error of
# the float32 CPU restatement, at most 1 / 10 of the distance of every planted fault tied to it.
TOL = {
    "stem": 7.2e-7,        # 2.42e-7: the seeded net at 40 x 56, B = 5
    "block": 7.6e-7,       # 2.54e-7: layer3.0 of the golden bottleneck net at 64 x 64, B = 5
    "pooled": 1.0e-7,      # 3.39e-8: the seeded net at 64 x 64 (2 x 2 pixels), B = 5
    "logits": 1.0e-6,      # 3.49e-7: the seeded net (F = 256) at 33 x 47, B = 5
    "tower": 1.4e-6,       # 4.68e-7: the seeded net at 33 x 47, B = 5
    "effect": 1.8e-5,      # 5.91e-6: the golden bottleneck net at 40 x 56 (logits of magnitude 7: the difference is absolute)
}

# Where each planted fault must show: (fault, kind of bound, [(net, H, W, B)], which stages of those cases -- a predicate on the
# block's spec, None for every stage of the kind).
FAULT_TIES = [
    ("norm_after_padding", "stem", [("golden_bottleneck", 40, 56, 3), ("seeded", 33, 47, 3)], None),
    # the two max-pool faults change the map's size (pad 0 always; ceil mode where conv1's output is even, where it adds a row
    # and a column and leaves the others as they are): no stage map can be compared, the logits through the whole tower can
    ("maxpool_pad_0", "tower", [("golden_bottleneck", 40, 56, 3), ("golden_basic", 40, 56, 3)], None),
    ("maxpool_ceil", "tower", [("golden_bottleneck", 40, 56, 3), ("golden_basic", 40, 56, 3)], None),
    ("bn_eps_1e-3", "block", [("golden_bottleneck", 40, 56, 3), ("golden_basic", 40, 56, 3), ("seeded", 33, 47, 3)], None),
    ("stride_on_first_1x1", "block", [("golden_bottleneck", 40, 56, 3), ("seeded", 33, 47, 3)], lambda spec: spec[4] == 2),
    ("relu_before_add", "block", [("golden_bottleneck", 40, 56, 3), ("golden_basic", 40, 56, 3), ("seeded", 33, 47, 3)], None),
    ("shortcut_without_bn", "block", [("golden_bottleneck", 40, 56, 3), ("golden_basic", 40, 56, 3)], lambda spec: spec[5]),
    ("avgpool_padded_count", "pooled", [("golden_bottleneck", 40, 56, 3), ("seeded", 224, 320, 1)], None),
    ("fc_bias_omitted", "logits", [("golden_bottleneck", 40, 56, 3), ("golden_basic", 40, 56, 3), ("seeded", 33, 47, 3)], None),
]


@functools.lru_cache(maxsize=None)
def reference(name, H, W, B):
    """The float64 model on a case, computed once and shared: (images fp32, logits, [stage outputs]); left unchanged."""
    arch, sd = net(name)
    x = images(B, H, W)
    z, outs = R.forward(sd, arch, x)
    return x, z, outs


def effect_pairs(B, H, W):
    """Originals and edits of the effect tests: smooth images and copies moved at amplitude 0.3; pair 0 is left unmoved."""
    a = images(B, H, W)
    b = R.perturbed(a, 0.3, 77)
    b[0] = a[0]
    return a, b


def quantized(x):
    """``save_image``'s rounding, as ``tools._inputs.quantize``."""
    return (x * 255 + 0.5).clamp(0, 255).to(torch.uint8).float() / 255


# Hand-made logits of three pairs over four attributes (a, b, c, d) and the columns worked out by hand.  Per pair: target a with
# sign +1; target b with sign +1 where nothing moved; target d with sign -1.
HAND_ZA = [[0, 0, 0, 0], [1, 2, 3, 4], [0, 0, 0, 1]]
HAND_ZB = [[1, 0.5, 0, -0.5], [1, 2, 3, 4], [0, 0, 2, -1]]
HAND_TARGET, HAND_SIGN = [0, 1, 3], [1.0, 1.0, -1.0]
HAND = np.array([[1.0, 1.0, 1.0 / 3, 0.5], [0.0, 1.0, 0.0, 0.0], [2.0, 1.0, 2.0 / 3, 0.5]])
HAND_SIGMA_VALUES = [1.0, 2.0, 4.0, 0.5]
HAND_WITH_SIGMA = np.array([[1.0, 1.0, 1.25 / 3, 1 / 2.25], [0.0, 1.0, 0.0, 0.0], [2.0, 1.0, 0.5 / 3, 4 / 4.5]])
