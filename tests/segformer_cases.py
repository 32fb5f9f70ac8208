"""The SegFormer tower's test nets, images, bounds and the tie of every planted fault to the bound that must catch it.  A helper of
tests/test_segformer_host.py, tests/test_gpu_segformer.py and tests/golden/make_segformer_golden.py, not a test.

Nets: ``golden`` -- the tiny model of tests/golden/segformer_tiny.npz (hidden 64 / 128 / 192 / 256, heads 1 / 2 / 3 / 4, depths
1 / 1 / 2 / 1, sr 8 / 4 / 2 / 1, decoder 128, 6 labels), whose weights ``seeded_state`` regenerates from the key names and shapes the
file holds (the file holds no weights -- they would be 17 MB -- and the images' sha256 instead of the images); ``seeded19`` --
the same encoder with 19 labels and the module's own ``seed=`` recipe; ``eps5`` -- that again (seed 2) with a different epsilon in
every kind of norm (``EPS5``), set on the modules after construction.

Bounds (``TOL``): each is 3 x the worst value an MI355X measured against the float64 model of tests/segformer_stages.py over every
case that uses it (the convention of tests/resnet_cases.py); the measured value and its case stand beside it and in
profiles/seg_metrics.md.  tests/test_segformer_host.py brackets each from both sides on the CPU.  From below: ``embed``, ``norm``
and ``head`` lie above the error of the same statements run in fp32, ``block_tight`` above the working-precision block run in fp32
instead of float64 (fp32 residual stream, LayerNorms and accumulation), ``block_loose``, ``logits`` and ``label_share`` above the
working-precision restatement's distance from float64.  From above: every fault lies at least 10 x above the bound of every stage
it acts in."""
import os

import numpy as np
import torch

from tests import segops_cases as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "segformer_tiny.npz")
TINY = dict(hidden_sizes=(64, 128, 192, 256), num_attention_heads=(1, 2, 3, 4), depths=(1, 1, 2, 1), sr_ratios=(8, 4, 2, 1),
            mlp_ratios=(4, 4, 4, 4), decoder_hidden_size=128)
GOLDEN_SEED = 20240917
GOLDEN_SIZE = (100, 132)
# (H, W): one key tile and whole maps; 15 keys in stage 0 (less than one key tile); odd maps 25 x 33 -> 4 x 5 with sr flooring
SIZES = [(64, 64), (96, 160), (100, 132)]
BATCHES = [1, 3]

# A tap stage is judged from the GPU's own previous stages (rel-L2 over the batch); 18 cases each: 3 nets x 3 sizes x B in (1, 3).
TOL = dict(
    embed=2.1e-6,        # measured 6.86e-7 (seeded19, 96 x 160, B 1): a patch embedding, fp32 convolution + LayerNorm
    block_tight=2.5e-3,  # measured 8.36e-4 (golden, 100 x 132, B 1): a block against the working-precision model (bf16 where the kernels round)
    block_loose=6.0e-3,  # measured 2.00e-3 (golden, 64 x 64, B 1): a block against plain float64
    norm=2.1e-7,         # measured 7.03e-8 (seeded19, 64 x 64, B 1): a stage's closing LayerNorm
    head=1.2e-6,         # measured 4.00e-7 (golden, 96 x 160, B 1): the concatenation, the fused map, the classifier, each from its own input
    logits=1.0e-2,       # measured 3.48e-3 (golden, 64 x 64, B 3): the logits end to end from the images (2.42e-3 against transformers' own
                         # float64 logits of the golden file)
    label_share=1.3e-2,  # measured 4.24e-3 (seeded19, 100 x 132, B 1): share of pixels whose label differs from the float64 model's; no
                         # differing pixel had a float64 margin beyond 4 x the worst logit error (5.5e-3 .. 1.04e-2 absolute)
)


def arch_of(module):
    """The ``arch`` dict of tests/segformer_stages.py for a ``libs.segformer.SegFormer`` (or anything with its attributes)."""
    e = module._eps()
    return dict(hidden=module.hidden_sizes, depths=module.depths, heads=module.num_attention_heads, sr=module.sr_ratios,
                mlp=module.mlp_ratios, D=module.decoder_hidden_size, L=module.num_labels,
                eps=dict(embed=e[0], block=e[1], sr=e[2], stage=e[3], bn=e[4]))


def seeded_state(shapes, seed=GOLDEN_SEED):
    """A well-conditioned state dict for the key -> shape mapping ``shapes``, drawn key by key in sorted key order from one
    generator (the recipe the golden's maker and the tests share): norm weights U(0.8, 1.2) and biases N(0, 0.1^2); running means
    N(0, 0.2^2), running variances U(0.5, 1.5); other weights N(0, 1 / fan_in) (o_proj and fc2 scaled by 0.5), other biases
    N(0, 0.1^2).  fp32 tensors (``num_batches_tracked``: int64 0)."""
    g = torch.Generator().manual_seed(int(seed))
    out = {}
    for name in sorted(shapes):
        shape = tuple(int(v) for v in shapes[name])
        if name.endswith("num_batches_tracked"):
            out[name] = torch.zeros(shape, dtype=torch.int64)
            continue
        r, u = torch.randn(shape, generator=g, dtype=torch.float64), torch.rand(shape, generator=g, dtype=torch.float64)
        is_norm = "norm" in name
        if name.endswith("running_var"):
            t = 0.5 + u
        elif name.endswith("running_mean"):
            t = 0.2 * r
        elif name.endswith(".bias"):
            t = 0.1 * r
        elif is_norm:
            t = 0.8 + 0.4 * u
        else:
            k = 0.5 if (".o_proj." in name or ".fc2." in name) else 1.0
            t = k * r * (1.0 / float(np.prod(shape[1:]))) ** 0.5
        out[name] = t.to(torch.float32)
    return out


# 'eps5': a different epsilon for every kind of norm, far enough apart that the embed / block swap moves every stage it acts in by
# at least 10 x that stage's bound, and that any of the five config fields reaching the wrong norm moves its stage by at least 2 x
# the bound (tests/test_segformer_host.py shows both, the second for all twenty mis-wirings).  The values are test values, not a
# model's: a block's bound is bf16-sized, so an epsilon has to be of the order of the variance to be seen there.  The large one
# sits in the blocks' norms, not in the patch embeddings', so that the residual stream keeps the scale it has in the other nets.
EPS5 = dict(embed=1e-5, block=0.5, sr=0.2, stage=0.05, bn=0.1)
_NETS = {}


def build(name):
    """A new ``SegFormer`` module of a test net, on the host: 'golden', 'seeded19' or 'eps5'."""
    from uspace_amd.libs.segformer import SegFormer
    if name == "golden":
        m = SegFormer(**TINY, num_labels=6)
        m.load_state_dict(seeded_state({k: v.shape for k, v in m.state_dict().items()}))
        return m
    if name == "seeded19":
        return SegFormer(**TINY, num_labels=19, seed=1)
    if name == "eps5":
        m = SegFormer(**TINY, num_labels=19, seed=2)
        for n, mod in m.named_modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.eps = EPS5["bn"]
            elif isinstance(mod, torch.nn.LayerNorm):
                mod.eps = EPS5["embed" if "patch_embeddings" in n else "sr" if "sequence_reduction" in n else
                               "block" if "layernorm_" in n else "stage"]
        return m
    raise KeyError(name)


def module(name):
    """The host module of a test net, built once (move a ``build`` to the device, not this one: ``.cuda()`` acts in place)."""
    if name not in _NETS:
        _NETS[name] = build(name)
    return _NETS[name]


def net(name):
    """(arch, float64 state dict) of a test net."""
    m = module(name)
    return arch_of(m), {k: v.detach().cpu().to(torch.float64) for k, v in m.state_dict().items() if v.is_floating_point()}


def sha256(a):
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def images(B, H, W):
    """Smooth fp32 test images [B, 3, H, W] in [0, 1]."""
    return S.images(B, H, W, 77)


# fault -> the bound that must catch it ('stage': the tap stage it acts in, from that stage's own inputs; 'logits': end to end;
# 'labels': the label map -- argmax_highest moves no logit, only exact ties, and is caught by the tie test of the label kernel)
FAULT_BOUND = {
    "concat_not_reversed": "stage", "align_corners": "stage", "sr_padded": "stage", "sr_norm_omitted": "stage", "scale_1/sqrtC": "stage",
    "dwconv_bias_omitted": "stage", "gelu_before_dwconv": "stage", "bn_eps_1e-3": "stage", "argmax_highest": "labels",
    "eps_swapped": "stage",           # judged on 'eps5': the identity where the two kinds hold one epsilon
}
