"""float64 restatement of the SD KL-VAE decoder (libs/autoencoder.py:303-409 Decoder, :446-450 decode), stage by stage.

TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).  Written from the math with torch CPU functional ops.  The stages
follow uspace_vae_decode_tap: 0 conv_in (z / scale -> post_quant_conv -> conv_in), 1 mid.block_1, 2 mid.attn_1,
3 mid.block_2, then every res block and upsample conv of the up path, highest level first.  ``run_stage`` maps the
input map of one stage to its output map; ``finish`` is norm_out + SiLU + conv_out; ``decode`` chains them from z.

``bf16=True`` rounds to bf16 exactly where vae.hip does (GroupNorm(+SiLU) outputs, the 3x3 / 1x1 conv weights but not
those of conv_in / post_quant_conv / conv_out, the 1x1 shortcut's input, q / k / v / P and the attention output before
proj_out, the nearest-2x upsample output); every sum is still taken in the working dtype.  Pinned against
tests/golden/vae_decoder_tiny.npz (taps and image produced by the reference's Decoder).
"""
import numpy as np
import torch
import torch.nn.functional as F


class Spec:
    """Decoder geometry (ddconfig of FrozenAutoencoderKL) and its stage list."""

    def __init__(self, ch, ch_mult, num_res_blocks, resolution, scale_factor=0.18215):
        self.ch, self.ch_mult, self.num_res_blocks, self.resolution = ch, tuple(ch_mult), num_res_blocks, resolution
        self.scale_factor = scale_factor
        n = len(self.ch_mult)
        self.z_res = resolution // 2 ** (n - 1)
        c, h = ch * self.ch_mult[-1], self.z_res
        st = [("conv_in", "decoder", h, c), ("res", "decoder.mid.block_1", h, c), ("attn", "decoder.mid.attn_1", h, c),
              ("res", "decoder.mid.block_2", h, c)]
        for lvl in reversed(range(n)):
            c = ch * self.ch_mult[lvl]
            for i in range(num_res_blocks + 1):
                st.append(("res", f"decoder.up.{lvl}.block.{i}", h, c))
            if lvl != 0:
                h *= 2
                st.append(("upsample", f"decoder.up.{lvl}.upsample.conv", h, c))
        self.stages = st     # (kind, state_dict prefix, output H, output C)

    @classmethod
    def from_ddconfig(cls, dd, scale_factor=0.18215):
        return cls(dd["ch"], dd["ch_mult"], dd["num_res_blocks"], dd["resolution"], scale_factor)


def _t(a, dtype):
    if isinstance(a, torch.Tensor):
        return a.detach().to("cpu", dtype)
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def _bf(x, on):
    return x.to(torch.bfloat16).to(x.dtype) if on else x


class _P:
    """state_dict view in the working dtype; with bf16 the kernel operands (3x3 / 1x1 weights) are rounded."""

    def __init__(self, sd, dtype, bf16):
        self.sd, self.dtype, self.bf16 = sd, dtype, bf16

    def __call__(self, key, operand=False):
        v = self.sd[key]
        if operand and self.bf16:       # fp32 checkpoint value -> bf16 (RNE), as the weight pack does
            return _t(_t(v, torch.float32).to(torch.bfloat16), self.dtype)
        return _t(v, self.dtype)


def _gn(x, p, pre, silu, eps=1e-6):
    h = F.group_norm(x, 32, p(pre + ".weight"), p(pre + ".bias"), eps)
    if silu:
        h = h * torch.sigmoid(h)
    return _bf(h, p.bf16)


def _conv(x, p, pre, operand=True):
    w = p(pre + ".weight", operand)
    return F.conv2d(x, w, p(pre + ".bias"), padding=w.shape[-1] // 2)


def _res(x, p, pre):
    """libs/autoencoder.py:114-134 with temb=None, dropout 0."""
    h = _conv(_gn(x, p, pre + ".norm1", True), p, pre + ".conv1")
    h = _conv(_gn(h, p, pre + ".norm2", True), p, pre + ".conv2")
    if pre + ".nin_shortcut.weight" in p.sd:
        x = _conv(_bf(x, p.bf16), p, pre + ".nin_shortcut")
    return x + h


def _attn(x, p, pre):
    """libs/autoencoder.py:171-195: one head over h*w tokens, scale c^-0.5, no SiLU after the norm."""
    B, C, H, W = x.shape
    h = _gn(x, p, pre + ".norm", False)
    q, k, v = (_bf(_conv(h, p, f"{pre}.{n}"), p.bf16).reshape(B, C, H * W) for n in ("q", "k", "v"))
    s = torch.einsum("bci,bcj->bij", q, k) * C ** -0.5
    w = _bf(torch.softmax(s, dim=2), p.bf16)
    o = _bf(torch.einsum("bcj,bij->bci", v, w).reshape(B, C, H, W), p.bf16)
    return x + _conv(o, p, pre + ".proj_out")


def attn_peak(spec, sd, x, dtype=torch.float64):
    """Largest softmax probability of the mid-block attention on its input map x (fp64, no rounding)."""
    p = _P(sd, dtype, False)
    pre = "decoder.mid.attn_1"
    x = _t(x, dtype)
    B, C, H, W = x.shape
    h = _gn(x, p, pre + ".norm", False)
    q, k = (_conv(h, p, f"{pre}.{n}").reshape(B, C, H * W) for n in ("q", "k"))
    return float(torch.softmax(torch.einsum("bci,bcj->bij", q, k) * C ** -0.5, dim=2).max())


def run_stage(spec, sd, k, x, bf16=False, dtype=torch.float64):
    """Stage k of the decode: input map [B, C, H, W] (for k = 0 the scaled latents z) -> output map, as a torch tensor
    of ``dtype`` on the CPU."""
    kind, pre, _, _ = spec.stages[k]
    p = _P(sd, dtype, bf16)
    x = _t(x, dtype)
    if kind == "conv_in":
        h = _conv(x * (1.0 / spec.scale_factor), p, "post_quant_conv", operand=False)
        return _conv(h, p, "decoder.conv_in", operand=False)
    if kind == "res":
        return _res(x, p, pre)
    if kind == "attn":
        return _attn(x, p, pre)
    up = _bf(x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3), bf16)     # F.interpolate(scale 2, nearest)
    return _conv(up, p, pre)


def finish(spec, sd, x, bf16=False, dtype=torch.float64, taps=None):
    """norm_out -> SiLU -> conv_out: last map -> image [B, 3, R, R]."""
    p = _P(sd, dtype, bf16)
    x = _t(x, dtype)
    h = F.group_norm(x, 32, p("decoder.norm_out.weight"), p("decoder.norm_out.bias"), 1e-6)
    if taps is not None:
        taps["norm_out"] = h
    h = _bf(h * torch.sigmoid(h), bf16)
    return _conv(h, p, "decoder.conv_out", operand=False)


def decode(spec, sd, z, bf16=False, dtype=torch.float64, taps=None, dtype_at=None):
    """The whole chain from z; taps (optional dict) receives every stage output under its index.  ``dtype_at(H)``, when
    given, picks the working dtype of the stages whose output resolution is H (a cheaper dtype for the largest maps)."""
    h = z
    for k, (_, _, H, _) in enumerate(spec.stages):
        h = run_stage(spec, sd, k, h, bf16, dtype_at(H) if dtype_at else dtype)
        if taps is not None:
            taps[k] = h
    return finish(spec, sd, h, bf16, dtype_at(spec.resolution) if dtype_at else dtype, taps)
