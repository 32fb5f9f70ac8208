"""Drop-in for the reference's frozen SD KL-VAE (libs/autoencoder.py:215-300 ``Encoder``, :303-409 ``Decoder``,
:412-458 ``FrozenAutoencoderKL``): latents [B,4,32,32] -> images [B,3,256,256] and, with ``encoder=True``, images ->
moments [B,8,32,32] -> latents.  Those are the nominal sizes (``ddconfig["resolution"]``): the network is fully
convolutional, so ``decode`` takes any square [B,4,h,h] and ``encode*`` any square [B,3,R,R] with R a multiple of 2^(levels-1) (8 here), with
the same weights -- 64x64 latents <-> 512^2 images among them.  Beyond 1 024 latent positions the mid-block attention is
the streaming kernel of attention_wide.hip.

Same ``state_dict`` keys as the reference.  Decoder-only (the default) holds ``decoder.*`` and ``post_quant_conv.*``
and ignores the encoder half of a checkpoint; ``encoder=True`` holds all four halves and loads strictly.  The
arithmetic runs in libuspace_hip.so: 3x3 convolutions (stride 2 over four phase maps in the down path) as 9-slab
bf16 MFMA GEMMs over a zero-bordered NHWC layout, GroupNorm+SiLU, resampling, the single-head mid-block attention
and the posterior sample as HIP kernels; no torch compute.  SURVEY.md 8(f) rank 1.
"""
import ctypes
import json

import torch
import torch.nn as nn

from .. import _hip
from .._blob import PackedWeights, WorkspaceCache
from ._uvit_core import ParamGroup


def _conv(group, name, cout, cin, k):
    c = group.child(name)
    c.add("weight", cout, cin, k, k)
    c.add("bias", cout)
    return c


def _norm(group, name, ch):
    n = group.child(name)
    n.add("weight", ch)
    n.add("bias", ch)
    return n


def _resblock(cin, cout):
    b = ParamGroup()
    _norm(b, "norm1", cin)
    _conv(b, "conv1", cout, cin, 3)
    _norm(b, "norm2", cout)
    _conv(b, "conv2", cout, cout, 3)
    if cin != cout:
        _conv(b, "nin_shortcut", cout, cin, 1)
    b.cin, b.cout = cin, cout
    return b


def _attn_block(group, name, ch):
    attn = group.child(name)
    _norm(attn, "norm", ch)
    for n in ("q", "k", "v", "proj_out"):
        _conv(attn, n, ch, ch, 1)
    return attn


def _max_chunk(res_channels):
    """Largest batch whose every zero-bordered map [B, H+2, H+2, C] stays below 2^30 elements (32-bit offsets)."""
    return max(1, ((1 << 30) - 1) // max((h + 2) ** 2 * c for h, c in res_channels))


class FrozenAutoencoderKL(nn.Module):
    def __init__(self, ddconfig, embed_dim=4, pretrained_path=None, scale_factor=0.18215, encoder=False):
        super().__init__()
        dd = dict(ddconfig)
        if dd.get("attn_resolutions"):
            raise NotImplementedError("attention inside the up path is not used by the reference (attn_resolutions=[])")
        if dd.get("give_pre_end") or dd.get("tanh_out") or dd.get("use_linear_attn") or dd.get("resamp_with_conv") is False:
            raise NotImplementedError("non-default Decoder options")
        self.ch, self.ch_mult = dd["ch"], tuple(dd["ch_mult"])
        self.num_res_blocks, self.resolution = dd["num_res_blocks"], dd["resolution"]
        self.z_channels, self.out_ch = dd["z_channels"], dd["out_ch"]
        if embed_dim != self.z_channels or self.z_channels != 4 or self.out_ch != 3:
            raise NotImplementedError("embed_dim == z_channels == 4 and out_ch == 3 (the SD VAE the reference uses)")
        if self.ch % 64:
            raise NotImplementedError("ch must be a multiple of 64 (128 in the reference)")
        self.embed_dim, self.scale_factor = embed_dim, scale_factor
        nres = len(self.ch_mult)
        self.z_res = self.resolution // 2 ** (nres - 1)
        self.has_encoder = bool(encoder)
        if self.has_encoder:
            if not dd.get("double_z", True) or dd.get("in_channels", 3) != 3:
                raise NotImplementedError("the encoder needs double_z=True and in_channels=3 (the SD VAE the reference uses)")
            if self.ch & (self.ch - 1):
                raise NotImplementedError("the encoder needs a power-of-two ch (128 in the reference)")
            self.encoder = self._build_encoder()
        block_in = self.ch * self.ch_mult[-1]

        dec = ParamGroup()
        _conv(dec, "conv_in", block_in, self.z_channels, 3)
        mid = dec.child("mid")
        mid.add_module("block_1", _resblock(block_in, block_in))
        _attn_block(mid, "attn_1", block_in)
        mid.add_module("block_2", _resblock(block_in, block_in))
        ups = [None] * nres
        for lvl in reversed(range(nres)):                       # construction order of the reference
            up = ParamGroup()
            block_out = self.ch * self.ch_mult[lvl]
            blocks = []
            for _ in range(self.num_res_blocks + 1):
                blocks.append(_resblock(block_in, block_out))
                block_in = block_out
            up.add_module("block", nn.ModuleList(blocks))
            up.add_module("attn", nn.ModuleList())
            if lvl != 0:
                _conv(up.child("upsample"), "conv", block_in, block_in, 3)
            ups[lvl] = up
        dec.add_module("up", nn.ModuleList(ups))
        _norm(dec, "norm_out", block_in)
        _conv(dec, "conv_out", self.out_ch, block_in, 3)
        self.decoder = dec
        if self.has_encoder:
            self.quant_conv = ParamGroup()
            self.quant_conv.add("weight", 2 * embed_dim, 2 * self.z_channels, 1, 1)
            self.quant_conv.add("bias", 2 * embed_dim)
        self.post_quant_conv = ParamGroup()
        self.post_quant_conv.add("weight", self.z_channels, embed_dim, 1, 1)
        self.post_quant_conv.add("bias", self.z_channels)
        self._reference_init_()
        mult = (ctypes.c_int * 4)(*(list(self.ch_mult) + [0] * (4 - nres)))
        self._cfg = _hip.VaeConfig(self.ch, mult, nres, self.num_res_blocks, self.resolution)
        self._packed = PackedWeights("uspace_vae_", "VAE", self._canonical_params, self._cfg)
        self._packed_enc = PackedWeights("uspace_vae_enc_", "VAE encoder", self._canonical_enc_params, self._cfg)
        self._ws = WorkspaceCache(1)
        self._ws_enc = WorkspaceCache(1)
        if pretrained_path is not None:
            self.load_state_dict(torch.load(pretrained_path, map_location="cpu"))
        self.eval()
        self.requires_grad_(False)

    def _build_encoder(self):
        """Encoder (libs/autoencoder.py:215-262) with no attention in the down path: conv_in, per level num_res_blocks
        res blocks and a stride-2 Downsample conv (not after the last level), mid, norm_out, conv_out to 2*z_channels."""
        enc = ParamGroup()
        _conv(enc, "conv_in", self.ch, 3, 3)
        block_in = self.ch
        downs = []
        for lvl in range(len(self.ch_mult)):
            down = ParamGroup()
            block_out = self.ch * self.ch_mult[lvl]
            blocks = []
            for _ in range(self.num_res_blocks):
                blocks.append(_resblock(block_in, block_out))
                block_in = block_out
            down.add_module("block", nn.ModuleList(blocks))
            down.add_module("attn", nn.ModuleList())
            if lvl != len(self.ch_mult) - 1:
                _conv(down.child("downsample"), "conv", block_in, block_in, 3)
            downs.append(down)
        enc.add_module("down", nn.ModuleList(downs))
        mid = enc.child("mid")
        mid.add_module("block_1", _resblock(block_in, block_in))
        _attn_block(mid, "attn_1", block_in)
        mid.add_module("block_2", _resblock(block_in, block_in))
        _norm(enc, "norm_out", block_in)
        _conv(enc, "conv_out", 2 * self.z_channels, block_in, 3)
        return enc

    # ------------------------------------------------------------------ init / checkpoints
    def _encoder_convs_in_construction_order(self):
        e = self.encoder
        yield e.conv_in
        for lvl in range(len(self.ch_mult)):
            for blk in e.down[lvl].block:
                yield from self._block_convs(blk)
            if lvl != len(self.ch_mult) - 1:
                yield e.down[lvl].downsample.conv
        yield from self._block_convs(e.mid.block_1)
        a = e.mid.attn_1
        yield from (a.q, a.k, a.v, a.proj_out)
        yield from self._block_convs(e.mid.block_2)
        yield e.conv_out

    def _conv_modules_in_construction_order(self):
        if self.has_encoder:
            yield from self._encoder_convs_in_construction_order()
        d = self.decoder
        yield d.conv_in
        for blk in (d.mid.block_1,):
            yield from self._block_convs(blk)
        a = d.mid.attn_1
        yield from (a.q, a.k, a.v, a.proj_out)
        yield from self._block_convs(d.mid.block_2)
        for lvl in reversed(range(len(self.ch_mult))):
            for blk in d.up[lvl].block:
                yield from self._block_convs(blk)
            if lvl != 0:
                yield d.up[lvl].upsample.conv
        yield d.conv_out
        if self.has_encoder:
            yield self.quant_conv
        yield self.post_quant_conv

    @staticmethod
    def _block_convs(blk):
        yield blk.conv1
        yield blk.conv2
        if hasattr(blk, "nin_shortcut"):
            yield blk.nin_shortcut

    @torch.no_grad()
    def _reference_init_(self):
        """torch's default Conv2d init in the reference's construction order ([Encoder,] Decoder, [quant_conv,]
        post_quant_conv), so the same ``torch.manual_seed`` yields the same weights; GroupNorm affine = (1, 0)."""
        for c in self._conv_modules_in_construction_order():
            cout, cin, k, _ = c.weight.shape
            ref = nn.Conv2d(cin, cout, k, padding=k // 2)
            c.weight.copy_(ref.weight)
            c.bias.copy_(ref.bias)
        for name, p in self.named_parameters():       # GroupNorm affine defaults
            if name.split(".")[-2].startswith("norm"):
                p.fill_(1.0 if name.endswith("weight") else 0.0)

    def load_state_dict(self, state_dict, strict=True):
        """Accepts a full autoencoder checkpoint.  Decoder-only: ``encoder.*`` / ``quant_conv.*`` entries are ignored;
        with the encoder every key is loaded (strict over the full set)."""
        if self.has_encoder:
            return super().load_state_dict(state_dict, strict=strict)
        sd = {k: v for k, v in state_dict.items() if not (k.startswith("encoder.") or k.startswith("quant_conv."))}
        return super().load_state_dict(sd, strict=strict)

    # ------------------------------------------------------------------ HIP decode
    def invalidate_packed(self):
        """Forget the packed weight blobs; needed only after in-place edits through ``p.data`` (``PackedWeights.invalidate``)."""
        self._packed.invalidate()
        self._packed_enc.invalidate()

    def _canonical_params(self):
        """The decoder half (decoder.*, post_quant_conv.*), packed for uspace_vae_decode."""
        return list(self.decoder.parameters()) + list(self.post_quant_conv.parameters())

    def _canonical_enc_params(self):
        """The encoder half (encoder.*, quant_conv.*), packed for uspace_vae_encode_moments."""
        return list(self.encoder.parameters()) + list(self.quant_conv.parameters())

    def _packed_blob(self, device):
        return self._packed.blob(device)

    def _packed_enc_blob(self, device):
        return self._packed_enc.blob(device)

    def _tap_map(self, dump, hc, B):
        """What a ``*_tap`` entry point left in ``dump`` (zero-bordered NHWC, hc = {H, C}) as [B, C, H, W]."""
        torch.cuda.synchronize()
        H, C = hc[0], hc[1]
        m = dump[: B * (H + 2) * (H + 2) * C].view(B, H + 2, H + 2, C)
        return m[:, 1:-1, 1:-1, :].permute(0, 3, 1, 2).contiguous()

    def _cfg_at(self, resolution):
        """The model's config at another image size.  The network is fully convolutional and takes its size from the tensor, as
        the reference's does; ``self.resolution`` stays the nominal size and the packed weights do not depend on it."""
        if resolution == self.resolution:
            return self._cfg
        c = self._cfg
        return _hip.VaeConfig(c.ch, c.ch_mult, c.n_levels, c.num_res_blocks, int(resolution))

    def _ws_key(self, chunk, resolution):
        """Workspace cache key: (chunk, resolution) off the nominal size; at the nominal size the chunk alone, the key every
        wrapper's cache uses (``WorkspaceCache``: (batch or chunk, device))."""
        return chunk if resolution == self.resolution else (chunk, resolution)

    def _check_latents(self, z):
        """-> the image size R = h * 2^(levels-1) of latents z [B, z_channels, h, h]: any square h >= 1."""
        _hip.require_device(z, "z")
        if z.dim() != 4 or z.shape[1] != self.z_channels or z.shape[2] != z.shape[3] or z.shape[2] < 1:
            raise ValueError(f"z must be square [B,{self.z_channels},h,h] with h >= 1 ({self.z_res} at the nominal "
                             f"resolution {self.resolution}), got {tuple(z.shape)}")
        return z.shape[2] * 2 ** (len(self.ch_mult) - 1)

    def decode(self, z, chunk=8):
        """z [B,4,h,h] (scaled latents, as produced by the sampler; any h >= 1) -> images [B,3,R,R] fp32, R = h *
        2^(levels-1).  Decodes ``chunk`` images at a time (the reference chunks by 50, dissect_lfm.py:86-98)."""
        R = self._check_latents(z)
        dev = z.device
        if z.shape[0] == 0:
            return torch.empty(0, self.out_ch, R, R, dtype=z.dtype, device=dev)
        blob = self._packed_blob(dev)
        L = _hip.lib()
        cfg = self._cfg_at(R)
        zin = z.detach().to(torch.float32).contiguous()
        B = zin.shape[0]
        out = torch.empty(B, self.out_ch, R, R, dtype=torch.float32, device=dev)
        max_chunk = _max_chunk([(R, 512)])
        chunk = max(1, min(chunk, max_chunk, B))
        ws = self._ws.take(self._ws_key(chunk, R), dev, L.uspace_vae_workspace_bytes(ctypes.byref(cfg), chunk))
        for lo in range(0, B, chunk):
            n = min(chunk, B - lo)
            _hip.check(L.uspace_vae_decode(ctypes.byref(cfg), _hip.ptr(blob), _hip.ptr(ws), ws.numel(),
                                           _hip.ptr(zin[lo:lo + n]), float(self.scale_factor), _hip.ptr(out[lo:lo + n]),
                                           n, _hip.stream_ptr()), "uspace_vae_decode")
        return out if z.dtype == torch.float32 else out.to(z.dtype)

    def decode_tap(self, z, stage):
        """Test aid: the fp32 feature map after ``stage`` (see uspace_vae_decode_tap) as [B, C, H, W]."""
        R = self._check_latents(z)
        dev = z.device
        blob = self._packed_blob(dev)
        L = _hip.lib()
        cfg = self._cfg_at(R)
        zin = z.detach().to(torch.float32).contiguous()
        B = zin.shape[0]
        nbytes = L.uspace_vae_workspace_bytes(ctypes.byref(cfg), B)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        dump = torch.zeros(B * (R + 2) ** 2 * 512, dtype=torch.float32, device=dev)
        hc = (ctypes.c_int * 2)()
        _hip.check(L.uspace_vae_decode_tap(ctypes.byref(cfg), _hip.ptr(blob), _hip.ptr(ws), ws.numel(), _hip.ptr(zin),
                                           float(self.scale_factor), B, int(stage), _hip.ptr(dump), hc, _hip.stream_ptr()),
                   "uspace_vae_decode_tap")
        return self._tap_map(dump, hc, B)

    # ------------------------------------------------------------------ HIP encode
    def _require_encoder(self, what):
        if not self.has_encoder:
            raise NotImplementedError(f"{what}: this model was built without the encoder (encoder=False)")

    def max_encode_chunk(self, resolution=None):
        """Largest legal encode chunk at ``resolution`` (the nominal one where None): every map of the down path below
        2^30 elements (126 images at 256^2)."""
        res, chan, rc = (self.resolution if resolution is None else resolution), self.ch, []
        for lvl, m in enumerate(self.ch_mult):
            rc.append((res, max(chan, self.ch * m)))
            chan = self.ch * m
            if lvl != len(self.ch_mult) - 1:
                res //= 2
        return _max_chunk(rc)

    def _check_images(self, x):
        """-> the size R of images x [B, 3, R, R]: any square R that the down path halves evenly."""
        _hip.require_device(x, "x")
        f = 2 ** (len(self.ch_mult) - 1)
        if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] != x.shape[3] or x.shape[2] < f or x.shape[2] % f:
            raise ValueError(f"x must be square [B,3,R,R] with R a positive multiple of {f} ({self.resolution} at the "
                             f"nominal resolution), got {tuple(x.shape)}")
        return x.shape[2]

    def encode_moments(self, x, chunk=8):
        """images x [B,3,R,R] in [-1, 1] (any R that is a multiple of 2^(levels-1)) -> moments [B, 2*embed_dim, h, h]
        (mean, logvar) fp32, ``chunk`` images at a time (the reference's feature extraction runs batches of 256,
        scripts/extract_*_feature.py)."""
        self._require_encoder("encode_moments")
        R = self._check_images(x)
        dev = x.device
        h = R // 2 ** (len(self.ch_mult) - 1)
        if x.shape[0] == 0:
            return torch.empty(0, 2 * self.embed_dim, h, h, dtype=x.dtype, device=dev)
        blob = self._packed_enc_blob(dev)
        L = _hip.lib()
        cfg = self._cfg_at(R)
        xin = x.detach().to(torch.float32).contiguous()
        B = xin.shape[0]
        out = torch.empty(B, 2 * self.embed_dim, h, h, dtype=torch.float32, device=dev)
        chunk = max(1, min(chunk, self.max_encode_chunk(R), B))
        ws = self._ws_enc.take(self._ws_key(chunk, R), dev, L.uspace_vae_enc_workspace_bytes(ctypes.byref(cfg), chunk))
        for lo in range(0, B, chunk):
            n = min(chunk, B - lo)
            _hip.check(L.uspace_vae_encode_moments(ctypes.byref(cfg), _hip.ptr(blob), _hip.ptr(ws), ws.numel(),
                                                   _hip.ptr(xin[lo:lo + n]), _hip.ptr(out[lo:lo + n]), n,
                                                   _hip.stream_ptr()), "uspace_vae_encode_moments")
        return out if x.dtype == torch.float32 else out.to(x.dtype)

    def sample(self, moments):
        """z = scale_factor * (mean + exp(0.5 * clamp(logvar, -30, 20)) * eps) with eps = ONE torch.randn_like(mean)
        over the whole batch, as the reference draws it (libs/autoencoder.py:433-439).  Needs no encoder weights."""
        _hip.require_device(moments, "moments")
        if moments.dim() != 4 or moments.shape[1] != 2 * self.embed_dim or moments.shape[2] != moments.shape[3]:
            raise ValueError(f"moments must be [B,{2 * self.embed_dim},h,h], got {tuple(moments.shape)}")
        mean, _ = torch.chunk(moments, 2, dim=1)
        eps = torch.randn_like(mean)
        B, h = moments.shape[0], moments.shape[2]
        z = torch.empty(B, self.embed_dim, h, h, dtype=torch.float32, device=moments.device)
        if B == 0:
            return z.to(moments.dtype)
        m = moments.detach().to(torch.float32).contiguous()
        e = eps.to(torch.float32).contiguous()
        _hip.check(_hip.lib().uspace_vae_sample(_hip.ptr(m), _hip.ptr(e), float(self.scale_factor), _hip.ptr(z), B, h,
                                                _hip.stream_ptr()), "uspace_vae_sample")
        return z if moments.dtype == torch.float32 else z.to(moments.dtype)

    def encode(self, x, chunk=8):
        """images -> scaled latents: the moments of every chunk first, then one ``sample`` over the batch."""
        return self.sample(self.encode_moments(x, chunk=chunk))

    def encode_tap(self, x, stage):
        """Test aid: the fp32 feature map after encode ``stage`` (see uspace_vae_encode_tap) as [B, C, H, W]."""
        self._require_encoder("encode_tap")
        R = self._check_images(x)
        dev = x.device
        blob = self._packed_enc_blob(dev)
        L = _hip.lib()
        cfg = self._cfg_at(R)
        xin = x.detach().to(torch.float32).contiguous()
        B = xin.shape[0]
        nbytes = L.uspace_vae_enc_workspace_bytes(ctypes.byref(cfg), B)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        cmax = self.ch * max(self.ch_mult)
        dump = torch.zeros(B * (R + 2) ** 2 * cmax, dtype=torch.float32, device=dev)
        hc = (ctypes.c_int * 2)()
        _hip.check(L.uspace_vae_encode_tap(ctypes.byref(cfg), _hip.ptr(blob), _hip.ptr(ws), ws.numel(), _hip.ptr(xin),
                                           B, int(stage), _hip.ptr(dump), hc, _hip.stream_ptr()), "uspace_vae_encode_tap")
        return self._tap_map(dump, hc, B)

    def forward(self, inputs, fn):
        if fn == "decode":
            return self.decode(inputs)
        if fn in ("encode_moments", "encode"):
            if not self.has_encoder:
                raise NotImplementedError(f"{fn}: this model was built without the encoder (encoder=False)")
            return self.encode_moments(inputs) if fn == "encode_moments" else self.encode(inputs)
        raise NotImplementedError(fn)


def get_model(pretrained_path, scale_factor=0.18215, encoder=None):
    """The SD KL-f8 autoencoder the reference samples through (libs/autoencoder.py:463-476): 256^2 images,
    4x32x32 latents, ch=128, multipliers 1-2-4-4, two res blocks per level, no attention in the up path.
    ``encoder=None`` includes the encoder iff the checkpoint holds ``encoder.*`` keys (so ``get_model(None)`` is
    decoder-only and a full SD checkpoint gives the full model, as in the reference)."""
    sd_vae = dict(double_z=True, z_channels=4, resolution=256, in_channels=3, out_ch=3, ch=128,
                  ch_mult=[1, 2, 4, 4], num_res_blocks=2, attn_resolutions=[], dropout=0.0)
    if pretrained_path is None:
        return FrozenAutoencoderKL(sd_vae, 4, None, scale_factor, encoder=bool(encoder))
    sd = torch.load(pretrained_path, map_location="cpu")
    if encoder is None:
        encoder = any(k.startswith("encoder.") for k in sd)
    vae = FrozenAutoencoderKL(sd_vae, 4, None, scale_factor, encoder=encoder)
    vae.load_state_dict(sd)
    return vae
