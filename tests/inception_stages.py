"""float64 restatement of the FID Inception-v3 (pytorch-fid's fid_inception_v3 up to the final average pool), written from
the math with torch's CPU float64 F.conv2d / avg_pool2d / max_pool2d / interpolate: every BasicConv2d is
relu(BN_eps=1e-3(conv(x))), the Mixed blocks concatenate their branches in the order listed in uspace_amd/tools/inception.py.

stage(sd, s, x) maps the output of tap stage s - 1 (NCHW float64) to the output of stage s, as uspace_inception_tap numbers
them (0: resize + 2x - 1 of the raw input; 19: the global mean).  ``faults`` plants numeric mutations for the tests that
show the tolerances catch them: "count_include_pad", "avg_7c", "eps_1e-5", "align_corners", "swap_1x7", "swap_concat"."""
import torch
import torch.nn.functional as F


def conv_bn_relu(sd, name, x, stride=1, padding=(0, 0), faults=()):
    w = torch.as_tensor(sd[f"{name}.conv.weight"]).double()
    g, b = (torch.as_tensor(sd[f"{name}.bn.{k}"]).double() for k in ("weight", "bias"))
    m, v = (torch.as_tensor(sd[f"{name}.bn.{k}"]).double() for k in ("running_mean", "running_var"))
    if "swap_1x7" in faults and tuple(w.shape[2:]) in ((1, 7), (7, 1)):
        w = w.transpose(2, 3)
        padding = padding[::-1]
    eps = 1e-5 if "eps_1e-5" in faults else 1e-3
    y = F.conv2d(x, w, stride=stride, padding=padding)
    s = g / torch.sqrt(v + eps)
    return torch.relu(y * s[None, :, None, None] + (b - m * s)[None, :, None, None])


def _avg(x, faults):
    return F.avg_pool2d(x, 3, 1, 1, count_include_pad="count_include_pad" in faults)


def _cat(parts, faults):
    if "swap_concat" in faults:
        parts = [parts[1], parts[0]] + parts[2:]
    return torch.cat(parts, 1)


def block_a(sd, n, x, f):
    c = lambda name, t, **k: conv_bn_relu(sd, f"{n}.{name}", t, faults=f, **k)
    b1 = c("branch1x1", x)
    b5 = c("branch5x5_2", c("branch5x5_1", x), padding=(2, 2))
    b3 = c("branch3x3dbl_3", c("branch3x3dbl_2", c("branch3x3dbl_1", x), padding=(1, 1)), padding=(1, 1))
    bp = c("branch_pool", _avg(x, f))
    return torch.cat([b1, b5, b3, bp], 1)


def block_b(sd, n, x, f):
    c = lambda name, t, **k: conv_bn_relu(sd, f"{n}.{name}", t, faults=f, **k)
    b3 = c("branch3x3", x, stride=2)
    bd = c("branch3x3dbl_3", c("branch3x3dbl_2", c("branch3x3dbl_1", x), padding=(1, 1)), stride=2)
    return torch.cat([b3, bd, F.max_pool2d(x, 3, 2)], 1)


def block_c(sd, n, x, f):
    c = lambda name, t, **k: conv_bn_relu(sd, f"{n}.{name}", t, faults=f, **k)
    b1 = c("branch1x1", x)
    b7 = c("branch7x7_3", c("branch7x7_2", c("branch7x7_1", x), padding=(0, 3)), padding=(3, 0))
    d = c("branch7x7dbl_1", x)
    d = c("branch7x7dbl_2", d, padding=(3, 0))
    d = c("branch7x7dbl_3", d, padding=(0, 3))
    d = c("branch7x7dbl_4", d, padding=(3, 0))
    d = c("branch7x7dbl_5", d, padding=(0, 3))
    bp = c("branch_pool", _avg(x, f))
    return _cat([b1, b7, d, bp], f)


def block_d(sd, n, x, f):
    c = lambda name, t, **k: conv_bn_relu(sd, f"{n}.{name}", t, faults=f, **k)
    b3 = c("branch3x3_2", c("branch3x3_1", x), stride=2)
    d = c("branch7x7x3_1", x)
    d = c("branch7x7x3_2", d, padding=(0, 3))
    d = c("branch7x7x3_3", d, padding=(3, 0))
    d = c("branch7x7x3_4", d, stride=2)
    return torch.cat([b3, d, F.max_pool2d(x, 3, 2)], 1)


def block_e(sd, n, x, f, max_pool):
    c = lambda name, t, **k: conv_bn_relu(sd, f"{n}.{name}", t, faults=f, **k)
    b1 = c("branch1x1", x)
    t = c("branch3x3_1", x)
    b3 = torch.cat([c("branch3x3_2a", t, padding=(0, 1)), c("branch3x3_2b", t, padding=(1, 0))], 1)
    t = c("branch3x3dbl_2", c("branch3x3dbl_1", x), padding=(1, 1))
    bd = torch.cat([c("branch3x3dbl_3a", t, padding=(0, 1)), c("branch3x3dbl_3b", t, padding=(1, 0))], 1)
    if max_pool and "avg_7c" not in f:
        p = F.max_pool2d(x, 3, 1, 1)
    else:
        p = _avg(x, f)
    return torch.cat([b1, b3, bd, c("branch_pool", p)], 1)


def stage(sd, s, x, faults=()):
    """Output of tap stage s from the output of stage s - 1 (for s = 0: from the raw [B, 3, H, W] input), float64 NCHW."""
    f = tuple(faults)
    x = torch.as_tensor(x).double()
    if s == 0:
        y = F.interpolate(x, size=(299, 299), mode="bilinear", align_corners="align_corners" in f)
        return 2 * y - 1
    stem = {1: ("Conv2d_1a_3x3", 2, (0, 0)), 2: ("Conv2d_2a_3x3", 1, (0, 0)), 3: ("Conv2d_2b_3x3", 1, (1, 1)),
            5: ("Conv2d_3b_1x1", 1, (0, 0)), 6: ("Conv2d_4a_3x3", 1, (0, 0))}
    if s in stem:
        name, st, p = stem[s]
        return conv_bn_relu(sd, name, x, stride=st, padding=p, faults=f)
    if s in (4, 7):
        return F.max_pool2d(x, 3, 2)
    if s in (8, 9, 10):
        return block_a(sd, ("Mixed_5b", "Mixed_5c", "Mixed_5d")[s - 8], x, f)
    if s == 11:
        return block_b(sd, "Mixed_6a", x, f)
    if s in (12, 13, 14, 15):
        return block_c(sd, ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e")[s - 12], x, f)
    if s == 16:
        return block_d(sd, "Mixed_7a", x, f)
    if s in (17, 18):
        return block_e(sd, ("Mixed_7b", "Mixed_7c")[s - 17], x, f, max_pool=s == 18)
    if s == 19:
        return x.mean((2, 3))
    raise ValueError(s)


def forward(sd, x, last=19, faults=()):
    """Stages 0 .. last from the raw input."""
    for s in range(last + 1):
        x = stage(sd, s, x, faults)
    return x
