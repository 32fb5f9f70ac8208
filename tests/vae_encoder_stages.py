"""float64 restatement of the SD KL-VAE encoder (libs/autoencoder.py:215-300 Encoder, :428-442 encode_moments / sample),
stage by stage, for the tests.  Written from the math with torch CPU functional ops; the res block, GroupNorm, conv and
attention pieces are those of oracle/vae_stages.py (imported, not restated).

Stages follow uspace_vae_encode_tap: 0 conv_in, then every res block and downsample of the down path in execution
order, then mid.block_1, mid.attn_1, mid.block_2.  ``finish`` is norm_out + SiLU + conv_out + quant_conv.

``bf16=True`` rounds to bf16 where vae.hip does: GroupNorm(+SiLU) outputs, the 3x3 / 1x1 weights of the GEMM convolutions
(not those of conv_in, conv_out or quant_conv), the 1x1 shortcut's input, q / k / v / P / the attention output, and the
downsample's input (the bf16 phase maps).  Pinned against tests/golden/vae_encoder_tiny.npz.
"""
import torch
import torch.nn.functional as F

from oracle.vae_stages import _P, _attn, _bf, _conv, _gn, _res, _t


class EncSpec:
    """Encoder geometry (ddconfig of FrozenAutoencoderKL) and its stage list."""

    def __init__(self, ch, ch_mult, num_res_blocks, resolution, scale_factor=0.18215):
        self.ch, self.ch_mult, self.num_res_blocks, self.resolution = ch, tuple(ch_mult), num_res_blocks, resolution
        self.scale_factor = scale_factor
        n = len(self.ch_mult)
        h, c = resolution, ch
        st = [("conv_in", "encoder.conv_in", h, c)]
        for lvl in range(n):
            c = ch * self.ch_mult[lvl]
            for i in range(num_res_blocks):
                st.append(("res", f"encoder.down.{lvl}.block.{i}", h, c))
            if lvl != n - 1:
                h //= 2
                st.append(("down", f"encoder.down.{lvl}.downsample.conv", h, c))
        st += [("res", "encoder.mid.block_1", h, c), ("attn", "encoder.mid.attn_1", h, c), ("res", "encoder.mid.block_2", h, c)]
        self.stages = st     # (kind, state_dict prefix, output H, output C)
        self.z_res = h

    @classmethod
    def from_ddconfig(cls, dd, scale_factor=0.18215):
        return cls(dd["ch"], dd["ch_mult"], dd["num_res_blocks"], dd["resolution"], scale_factor)


def downsample(x, p, pre):
    """Downsample with_conv (libs/autoencoder.py:64-70): zero pad right / bottom by one, 3x3 stride 2, no padding."""
    x = F.pad(_bf(x, p.bf16), (0, 1, 0, 1))
    return F.conv2d(x, p(pre + ".weight", True), p(pre + ".bias"), stride=2)


def run_stage(spec, sd, k, x, bf16=False, dtype=torch.float64):
    """Stage k of the encode: input map [B, C, H, W] (for k = 0 the images) -> output map, a CPU tensor of ``dtype``."""
    kind, pre, _, _ = spec.stages[k]
    p = _P(sd, dtype, bf16)
    x = _t(x, dtype)
    if kind == "conv_in":
        return _conv(x, p, pre, operand=False)
    if kind == "res":
        return _res(x, p, pre)
    if kind == "attn":
        return _attn(x, p, pre)
    return downsample(x, p, pre)


def finish(spec, sd, x, bf16=False, dtype=torch.float64, taps=None):
    """norm_out -> SiLU -> conv_out -> quant_conv: last map -> moments [B, 8, h, h]."""
    p = _P(sd, dtype, bf16)
    x = _t(x, dtype)
    h = F.group_norm(x, 32, p("encoder.norm_out.weight"), p("encoder.norm_out.bias"), 1e-6)
    if taps is not None:
        taps["norm_out"] = h
    h = _bf(h * torch.sigmoid(h), bf16)
    h = _conv(h, p, "encoder.conv_out", operand=False)
    return F.conv2d(h, p("quant_conv.weight"), p("quant_conv.bias"))


def encode_moments(spec, sd, x, bf16=False, dtype=torch.float64, taps=None, dtype_at=None):
    """The whole chain from the images; taps (optional dict) receives every stage output under its index.  ``dtype_at(H)``
    picks the working dtype of the stages whose output resolution is H (a cheaper dtype for the largest maps)."""
    h = x
    for k, (_, _, H, _) in enumerate(spec.stages):
        h = run_stage(spec, sd, k, h, bf16, dtype_at(H) if dtype_at else dtype)
        if taps is not None:
            taps[k] = h
    return finish(spec, sd, h, bf16, dtype_at(spec.z_res) if dtype_at else dtype, taps)


def sample(moments, eps, scale_factor):
    """FrozenAutoencoderKL.sample with a given eps, in the dtype of ``moments``."""
    mean, logvar = torch.chunk(moments, 2, dim=1)
    logvar = torch.clamp(logvar, -30.0, 20.0)
    return scale_factor * (mean + torch.exp(0.5 * logvar) * eps)
