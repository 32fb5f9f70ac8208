"""The packed-weight blobs of the models as the library lays them out: which configurations are pinned, how a size
record and a blob digest are taken.  Shared by tests/golden/make_blob_golden.py (which records them) and by
tests/test_blob_layout.py / tests/test_gpu_blob_pack.py (which compare).  Nothing here goes through the Python wrappers'
own pack path: the size queries and ``uspace_*_pack_weights`` are called through ctypes."""
import ctypes
import hashlib
import json
import os

import numpy as np
import torch

BATCHES = (1, 3, 8, 64)
SD_DDCONFIG = dict(double_z=True, z_channels=4, resolution=256, in_channels=3, out_ch=3, ch=128,
                   ch_mult=[1, 2, 4, 4], num_res_blocks=2, attn_resolutions=[], dropout=0.0)
TINY_UVIT = dict(img_size=16, patch_size=2, in_chans=4, embed_dim=64, depth=2, num_heads=1, mlp_ratio=4,
                 qkv_bias=False, mlp_time_embed=False)
TINY_UVIT_KINDS = {"tiny_u": ("uvit", "tiny_u.npz", dict(num_classes=-1)),
                   "tiny_t2i": ("uvit_t2i", "tiny_t2i.npz", dict(clip_dim=64, num_clip_token=77))}
CLIP_KEYS = ("vocab_size", "hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads",
             "max_position_embeddings", "layer_norm_eps")


def _meta(golden_dir, name):
    z = np.load(os.path.join(golden_dir, name))
    return z, json.loads(bytes(z["meta_json"]).decode())


def uvit_cfg(name, img_size, patch_size, in_chans, embed_dim, depth, num_heads, mlp_ratio=4, num_classes=-1, clip_dim=768,
             num_clip_token=77, **_):
    from uspace_amd import _hip
    hidden = int(embed_dim * mlp_ratio)
    if name == "uvit_t2i":
        return _hip.UvitConfig(img_size, patch_size, in_chans, embed_dim, depth, num_heads, hidden, num_clip_token, clip_dim, 1)
    return _hip.UvitConfig(img_size, patch_size, in_chans, embed_dim, depth, num_heads, hidden, 1 if num_classes > 0 else 0, 0, 0)


def vae_cfg(dd):
    from uspace_amd import _hip
    mult = (ctypes.c_int * 4)(*(list(dd["ch_mult"]) + [0] * (4 - len(dd["ch_mult"]))))
    return _hip.VaeConfig(dd["ch"], mult, len(dd["ch_mult"]), dd["num_res_blocks"], dd["resolution"])


def clip_cfg(vocab_size, hidden_size, intermediate_size, num_hidden_layers, num_attention_heads, max_position_embeddings,
             layer_norm_eps, **_):
    from uspace_amd import _hip
    return _hip.ClipConfig(vocab_size, hidden_size, num_attention_heads, num_hidden_layers, intermediate_size,
                           max_position_embeddings, layer_norm_eps)


def clipv_cfg(hidden_size, intermediate_size, num_hidden_layers, num_attention_heads, image_size, patch_size, projection_dim,
              layer_norm_eps, **_):
    from uspace_amd import _hip
    return _hip.ClipVisionConfig(image_size, patch_size, hidden_size, num_attention_heads, num_hidden_layers, intermediate_size,
                                 projection_dim, layer_norm_eps)


def dino_cfg(hidden_size, num_attention_heads, num_hidden_layers, patch_size, image_size, layerscale, layer_norm_eps, mlp_ratio=4, **_):
    from uspace_amd import _hip
    return _hip.DinoConfig(image_size, patch_size, hidden_size, num_attention_heads, num_hidden_layers, hidden_size * mlp_ratio,
                           1 if layerscale else 0, layer_norm_eps)


def idnet_cfg(input_size, blocks, se):
    from uspace_amd import _hip
    return _hip.IdnetConfig(input_size, (ctypes.c_int * 4)(*blocks), se)


def tiny_dino():
    """The golden DINOv2 tower of tests/dino_cases.py at its table's own side (no interpolation of the position table)."""
    from tests import dino_cases as D
    return D.golden_module_config("dinov2", 70)


def lead_args(cfg):
    """What every entry point of a family takes first: nothing, an int by value (``uspace_lpips_``'s ``net``) or its config struct."""
    return () if cfg is None else (cfg if isinstance(cfg, int) else ctypes.byref(cfg),)


def size_cases(golden_dir):
    """{case name: (symbol prefix, config or None, [(label, extra workspace arguments)])}.  The U-ViT cases are every model of
    tools/bench_configs.py and the two tiny fixtures; they are recorded once per setting of uspace_gemm_set_sk (size_table)."""
    from bench import COMMON, MODELS
    from tools.bench_configs import CONFIGS
    from tests.clip_vision_cases import TINY_VISION
    from uspace_amd.libs.clip import CLIP_L_TEXT, CLIP_L_VISION
    plain = [("", ())]
    cases = {}
    for model in sorted({c["model"] for c in CONFIGS}):
        cfg = dict(MODELS[model])
        cases[f"uvit/{model}"] = ("uspace_uvit_", uvit_cfg(cfg.pop("name"), **COMMON, **cfg), plain)
    for tag, (name, _f, kw) in TINY_UVIT_KINDS.items():
        cases[f"uvit/{tag}"] = ("uspace_uvit_", uvit_cfg(name, **TINY_UVIT, **kw), plain)
    tiny_dec = _meta(golden_dir, "vae_decoder_tiny.npz")[1]["ddconfig"]
    tiny_enc = _meta(golden_dir, "vae_encoder_tiny.npz")[1]["ddconfig"]
    for tag, dec, enc in (("sd", SD_DDCONFIG, SD_DDCONFIG), ("tiny", tiny_dec, tiny_enc)):
        cases[f"vae/{tag}"] = ("uspace_vae_", vae_cfg(dec), plain)
        cases[f"vae_enc/{tag}"] = ("uspace_vae_enc_", vae_cfg(enc), plain)
    cases["clip/L"] = ("uspace_clip_", clip_cfg(**CLIP_L_TEXT), plain)
    cases["clip/tiny"] = ("uspace_clip_", clip_cfg(**_meta(golden_dir, "clip_text_tiny.npz")[1]), plain)
    cases["clipv/L"] = ("uspace_clipv_", clipv_cfg(**CLIP_L_VISION), plain)
    cases["clipv/tiny"] = ("uspace_clipv_", clipv_cfg(**TINY_VISION), plain)
    cases["inception"] = ("uspace_inception_", None, [("299/", (299, 299)), ("64/", (64, 64))])
    from uspace_amd.libs.arcface import BLOCKS
    from uspace_amd.libs.dino import DINOV2_L14
    from uspace_amd.tools.lpips import NETS
    for net in ("alex", "vgg"):
        cases[f"lpips/{net}"] = ("uspace_lpips_", NETS[net], [("64/", (64, 64)), ("256/", (256, 256))])
    cases["idnet/IR_SE50"] = ("uspace_idnet_", idnet_cfg(112, BLOCKS[50], 1), plain)
    cases["idnet/tiny_se"] = ("uspace_idnet_", idnet_cfg(32, (1, 1, 1, 1), 1), plain)
    cases["idnet/tiny_ir"] = ("uspace_idnet_", idnet_cfg(32, (1, 1, 1, 1), 0), plain)
    cases["dino/L14"] = ("uspace_dino_", dino_cfg(**DINOV2_L14), plain)
    cases["dino/tiny"] = ("uspace_dino_", dino_cfg(**tiny_dino()), plain)
    return cases


def size_record(L, prefix, cfg, ws_forms):
    lead = lead_args(cfg)
    fn = lambda what: getattr(L, prefix + what)
    n = fn("num_params")(*lead)
    return dict(num_params=n, param_numel=[fn("param_numel")(*lead, i) for i in range(n)], weight_bytes=fn("weight_bytes")(*lead),
                workspace_bytes={f"{label}{B}": fn("workspace_bytes")(*lead, B, *extra) for label, extra in ws_forms for B in BATCHES})


def size_table(golden_dir):
    """Every size the library reports for the pinned configurations; U-ViT under both settings of the K-split tail switch."""
    from uspace_amd import _hip
    L = _hip.lib()
    out = {}
    try:
        for name, (prefix, cfg, ws_forms) in size_cases(golden_dir).items():
            if prefix == "uspace_uvit_":
                for sk in (1, 0):
                    assert L.uspace_gemm_set_sk(sk) == 0
                    out[f"{name}/sk{sk}"] = size_record(L, prefix, cfg, ws_forms)
                assert L.uspace_gemm_set_sk(-1) == 0
            else:
                out[name] = size_record(L, prefix, cfg, ws_forms)
    finally:
        L.uspace_gemm_set_sk(-1)
    return out


# --------------------------------------------------------------------------------------------- the tiny models (GPU)
def tiny_model(kind, golden_dir):
    """(module on the GPU, symbol prefix, config or None, tensors in the library's canonical order) of one tiny model."""
    if kind in TINY_UVIT_KINDS:
        from uspace_amd.tools.utils_uvit import get_nnet
        name, fixture, kw = TINY_UVIT_KINDS[kind]
        z = np.load(os.path.join(golden_dir, fixture))
        net = get_nnet(name, **TINY_UVIT, **kw)
        net.load_state_dict({k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd/")}, strict=True)
        net = net.cuda().eval()
        return net, "uspace_uvit_", uvit_cfg(name, **TINY_UVIT, **kw), net._canonical_params()
    if kind in ("vae", "vae_enc"):
        from uspace_amd.libs.autoencoder import FrozenAutoencoderKL
        enc = kind == "vae_enc"
        meta = _meta(golden_dir, "vae_encoder_tiny.npz" if enc else "vae_decoder_tiny.npz")[1]
        torch.manual_seed(meta["weight_seed"])
        vae = FrozenAutoencoderKL(meta["ddconfig"], 4, encoder=enc).cuda()
        ps = (list(vae.encoder.parameters()) + list(vae.quant_conv.parameters())) if enc else \
             (list(vae.decoder.parameters()) + list(vae.post_quant_conv.parameters()))
        return vae, "uspace_vae_enc_" if enc else "uspace_vae_", vae_cfg(meta["ddconfig"]), ps
    if kind == "clip":
        from uspace_amd.libs.clip import CLIPTextTransformer
        z, meta = _meta(golden_dir, "clip_text_tiny.npz")
        m = CLIPTextTransformer(**{k: meta[k] for k in CLIP_KEYS + ("hidden_act",)})
        m.load_state_dict({"text_model." + k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd/")})
        m = m.cuda()
        return m, "uspace_clip_", clip_cfg(**meta), list(m.parameters())
    if kind == "clipv":
        from tests import clip_vision_cases as V
        from uspace_amd.libs.clip import CLIPVisionTransformer
        cfg = V.TOWER_CASES["tiny"][0]
        m = CLIPVisionTransformer(**cfg)
        m.load_state_dict(V.case_params("tiny"))
        m = m.cuda()
        return m, "uspace_clipv_", clipv_cfg(**cfg), list(m.parameters())
    if kind == "inception":
        from uspace_amd.tools.inception import InceptionV3
        m = InceptionV3([3], seed=0).cuda()
        return m, "uspace_inception_", None, list(m.state_dict().values())
    if kind in ("lpips_alex", "lpips_vgg"):
        from uspace_amd.tools.lpips import LPIPS, NETS
        m = LPIPS(kind[6:], seed=3).cuda()
        return m, "uspace_lpips_", NETS[m.net], m._canonical_params()
    if kind in ("idnet", "idnet_ir"):
        from uspace_amd.libs.arcface import Backbone
        kw = dict(mode="ir", seed=9) if kind == "idnet_ir" else dict(seed=5)
        m = Backbone(input_size=32, blocks=(1, 1, 1, 1), **kw).cuda()
        return m, "uspace_idnet_", m.cfg, m._canonical_params()
    assert kind == "dino"
    from uspace_amd.libs.dino import DinoVisionTransformer
    m = DinoVisionTransformer(seed=0, **tiny_dino()).cuda()
    return m, "uspace_dino_", m._c_cfg(), m._canonical_params()


TINY_KINDS = ("tiny_u", "tiny_t2i", "vae", "vae_enc", "clip", "clipv", "inception", "lpips_alex", "lpips_vgg", "idnet", "idnet_ir",
              "dino")


def blob_digest(prefix, cfg, tensors):
    """sha256 of the whole blob ``{prefix}pack_weights`` writes into zeroed memory (so the padding is compared too)."""
    from uspace_amd import _hip
    L = _hip.lib()
    lead = lead_args(cfg)
    srcs = [t.detach().to(torch.float32).contiguous() for t in tensors]
    nbytes = getattr(L, prefix + "weight_bytes")(*lead)
    assert nbytes > 0 and getattr(L, prefix + "num_params")(*lead) == len(srcs)
    blob = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    arr = (ctypes.c_void_p * len(srcs))(*[s.data_ptr() for s in srcs])
    _hip.check(getattr(L, prefix + "pack_weights")(*lead, arr, len(srcs), _hip.ptr(blob), nbytes, _hip.stream_ptr()),
               prefix + "pack_weights")
    torch.cuda.synchronize()
    return hashlib.sha256(blob.cpu().numpy().tobytes()).hexdigest()
