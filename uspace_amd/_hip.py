"""ctypes binding of libuspace_hip.so (include/uspace_hip.h).

There is NO fallback: if the shared library is missing or an entry point returns an error the
caller gets an exception.  torch is used only to own device memory and to name the stream.
"""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# (USPACE_HIP_LIB: another build of the same ABI, for A/B measurements of whole solves on one box -- tools/lab/.  Lab builds can be WRONG on
# purpose (ablations that skip stores, forms that were not landed): lib() says so on stderr and library_info() carries it into bench.py's line.)
_DEFAULT_LIB = os.path.join(_HERE, "libuspace_hip.so")
LIB_PATH = os.environ.get("USPACE_HIP_LIB") or _DEFAULT_LIB

EPI_BIAS, EPI_GELU, EPI_RESIDUAL, EPI_OUT_F32, EPI_OUT_BF16 = 1, 2, 4, 8, 16
EPI_CEN_OUT, EPI_LN_IN, EPI_RANK1 = 32, 64, 128          # uspace_gemm_bf16_ext only (LayerNorm folded through the GEMMs)

ABI_VERSION = 11

_ERR = {-1: "USPACE_ERR_ARG", -2: "USPACE_ERR_LAUNCH", -3: "USPACE_ERR_WORKSPACE"}


class UspaceHipError(RuntimeError):
    pass


class UvitConfig(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in (
        "img_size", "patch_size", "in_chans", "embed_dim", "depth", "num_heads", "mlp_hidden",
        "n_extra", "clip_dim", "time_first")]


class UvitIO(ctypes.Structure):
    _fields_ = [
        ("x", ctypes.c_void_p), ("t", ctypes.c_void_p), ("t_stride", ctypes.c_int),
        ("context", ctypes.c_void_p), ("mid_delta", ctypes.c_void_p), ("mid_scale", ctypes.c_float),
        ("mid_tap", ctypes.c_void_p), ("key_scale", ctypes.c_void_p), ("out", ctypes.c_void_p),
        ("mid_row_scale", ctypes.c_void_p)]


class VaeConfig(ctypes.Structure):
    _fields_ = [("ch", ctypes.c_int), ("ch_mult", ctypes.c_int * 4), ("n_levels", ctypes.c_int),
                ("num_res_blocks", ctypes.c_int), ("resolution", ctypes.c_int)]


class ClipConfig(ctypes.Structure):
    _fields_ = [("vocab", ctypes.c_int), ("dim", ctypes.c_int), ("heads", ctypes.c_int), ("layers", ctypes.c_int),
                ("ffn", ctypes.c_int), ("max_pos", ctypes.c_int), ("eps", ctypes.c_float)]


class ClipVisionConfig(ctypes.Structure):
    _fields_ = [("image", ctypes.c_int), ("patch", ctypes.c_int), ("dim", ctypes.c_int), ("heads", ctypes.c_int),
                ("layers", ctypes.c_int), ("ffn", ctypes.c_int), ("proj_dim", ctypes.c_int), ("eps", ctypes.c_float)]


class DinoConfig(ctypes.Structure):
    _fields_ = [("image", ctypes.c_int), ("patch", ctypes.c_int), ("dim", ctypes.c_int), ("heads", ctypes.c_int),
                ("layers", ctypes.c_int), ("ffn", ctypes.c_int), ("layerscale", ctypes.c_int), ("eps", ctypes.c_float)]


class IdnetConfig(ctypes.Structure):
    _fields_ = [("input_size", ctypes.c_int), ("blocks", ctypes.c_int * 4), ("se", ctypes.c_int)]


class ResnetConfig(ctypes.Structure):
    _fields_ = [("stem", ctypes.c_int), ("planes", ctypes.c_int * 4), ("blocks", ctypes.c_int * 4), ("bottleneck", ctypes.c_int),
                ("num_outputs", ctypes.c_int)]


class SegformerConfig(ctypes.Structure):
    _fields_ = [("hidden", ctypes.c_int * 4), ("depths", ctypes.c_int * 4), ("heads", ctypes.c_int * 4), ("sr", ctypes.c_int * 4),
                ("mlp", ctypes.c_int * 4), ("decoder_dim", ctypes.c_int), ("num_labels", ctypes.c_int), ("eps_embed", ctypes.c_float),
                ("eps_block", ctypes.c_float), ("eps_sr", ctypes.c_float), ("eps_stage", ctypes.c_float), ("eps_bn", ctypes.c_float)]


class GemmExt(ctypes.Structure):
    _fields_ = [("row_c", ctypes.c_void_p), ("out_cen", ctypes.c_void_p), ("ld_cen", ctypes.c_int),
                ("part_out", ctypes.c_void_p), ("part_in", ctypes.c_void_p), ("np_in", ctypes.c_int),
                ("colsum", ctypes.c_void_p), ("c_out", ctypes.c_void_p), ("norm_dim", ctypes.c_int), ("eps", ctypes.c_float),
                ("row_add", ctypes.c_void_p), ("col_add", ctypes.c_void_p),
                ("split_ws", ctypes.c_void_p), ("split_ws_bytes", ctypes.c_size_t),
                ("sk_ws", ctypes.c_void_p), ("sk_ws_bytes", ctypes.c_size_t), ("sk_counters", ctypes.c_void_p)]


_P, _I, _L, _F, _SZ = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_size_t
_D = ctypes.c_double

# name -> (restype, argtypes); must list every symbol include/uspace_hip.h declares
SIGNATURES = {
    "uspace_abi_version": (_I, []),
    "uspace_gemm_bf16": (_I, [_P, _I, _P, _I, _I, _P, _I, _I, _I, _I, _I, _P, _P, _I, _P, _I, _P, _I, _P]),
    "uspace_gemm_bf16_ext": (_I, [_P, _I, _P, _I, _I, _P, _I, _I, _I, _I, _I, _P, _P, _I, _P, _I, _P, _I,
                                  ctypes.POINTER(GemmExt), _P]),
    "uspace_gemm_part_slots": (_I, [_I, _I]),
    "uspace_gemm_part_slots_k": (_I, [_I, _I, _I]),
    "uspace_gemm_split_ws_bytes": (_SZ, [_I, _I, _I]),
    "uspace_gemm_sk_ws_bytes": (_SZ, [_I, _I, _I]),
    "uspace_gemm_set_sk": (_I, [_I]),
    "uspace_gemm_get_sk": (_I, []),
    "uspace_fold_layernorm": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _P]),
    "uspace_center_rows": (_I, [_P, _P, _P, _P, _I, _I, _P]),
    "uspace_uvit_set_ln_fold": (_I, [_I]),
    "uspace_uvit_get_ln_fold": (_I, []),
    "uspace_gemm_tile_choice": (_I, [_I, _I, ctypes.POINTER(_I)]),
    "uspace_gemm_plan": (_I, [_I, _I, ctypes.POINTER(_I)]),
    "uspace_gemm_plan_k": (_I, [_I, _I, _I, _I, ctypes.POINTER(_I)]),
    "uspace_gemm_slabs_bf16": (_I, [_P, _I, _P, _I, _I, _I, _I, _I, ctypes.POINTER(_I), _I, _P, _P, _I, _P, _I, _P, _I, _P]),
    "uspace_layernorm_f32_bf16": (_I, [_P, _P, _P, _P, _I, _I, _F, _P]),
    "uspace_attention_bf16": (_I, [_P, _P, _P, _I, _I, _I, _P]),
    "uspace_attention_plan": (_I, [_I, _I, _I, _I, ctypes.POINTER(_I)]),
    "uspace_attention_long_bf16": (_I, [_P, _P, _P, _I, _I, _I, _P]),
    "uspace_attention_long_plan": (_I, [_I, _I, _I, _I, ctypes.POINTER(_I)]),
    "uspace_attention_wide_bf16": (_I, [_P, _P, _P, _I, _P, _I, _I, _I, _I, _F, _P]),
    "uspace_attention_wide_plan": (_I, [_I, _I, _I, ctypes.POINTER(_I)]),
    "uspace_attention_map_bf16": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "uspace_embed_tokens": (_I, [_P, _P, _I, _P, _I, _I, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "uspace_output_head": (_I, [_P, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _F, _P]),
    "uspace_add_broadcast": (_I, [_P, _P, _P, _F, _I, _L, _P]),
    "uspace_add_broadcast_rows": (_I, [_P, _P, _P, _F, _P, _I, _L, _P]),
    "uspace_cast_f32_bf16": (_I, [_P, _P, _L, _P]),
    "uspace_cfg_combine": (_I, [_P, _P, _F, _P, _I, _L, _P]),
    "uspace_direction_accumulate": (_I, [_P, _P, _P, _P, _I, _L, _I, _P]),
    "uspace_center_cols_f32": (_I, [_P, _P, _I, _L, _P]),
    "uspace_gram_f64": (_I, [_P, _P, _I, _L, _P]),
    "uspace_project_rows_f64": (_I, [_P, _P, _P, _I, _I, _L, _P]),
    "uspace_normalize_rows_signed": (_I, [_P, _I, _L, _P]),
    "uspace_ode_combine": (_I, [_P, _P, ctypes.POINTER(_P), ctypes.POINTER(_F), _I, _L, _P]),
    "uspace_ode_error_norm": (_I, [_P, _P, ctypes.POINTER(_P), ctypes.POINTER(_F), _I, _F, _F, _L, _P, _P, _P]),
    "uspace_uvit_num_params": (_I, [ctypes.POINTER(UvitConfig)]),
    "uspace_uvit_param_numel": (_L, [ctypes.POINTER(UvitConfig), _I]),
    "uspace_uvit_weight_bytes": (_SZ, [ctypes.POINTER(UvitConfig)]),
    "uspace_uvit_workspace_bytes": (_SZ, [ctypes.POINTER(UvitConfig), _I]),
    "uspace_uvit_pack_weights": (_I, [ctypes.POINTER(UvitConfig), ctypes.POINTER(_P), _I, _P, _SZ, _P]),
    "uspace_uvit_forward": (_I, [ctypes.POINTER(UvitConfig), _P, _P, _SZ, ctypes.POINTER(UvitIO), _I, _P]),
    "uspace_uvit_forward_maps": (_I, [ctypes.POINTER(UvitConfig), _P, _P, _SZ, ctypes.POINTER(UvitIO), _I, _I, _I, _I, _I, _P, _P]),
    "uspace_uvit_cfg_workspace_bytes": (_SZ, [ctypes.POINTER(UvitConfig), _I]),
    "uspace_uvit_forward_cfg": (_I, [ctypes.POINTER(UvitConfig), _P, _P, _SZ, ctypes.POINTER(UvitIO), _I, _P, _I, _F, _P, _P, _P]),
    "uspace_uvit_forward_tap": (_I, [ctypes.POINTER(UvitConfig), _P, _P, _SZ, ctypes.POINTER(UvitIO), _I, _I, _P, _P]),
    "uspace_uvit_graph_create": (_I, [ctypes.POINTER(UvitConfig), _P, _P, _SZ, ctypes.POINTER(UvitIO), _I, _P,
                                      ctypes.POINTER(_P)]),
    "uspace_uvit_graph_launch": (_I, [_P, _P]),
    "uspace_uvit_graph_destroy": (_I, [_P]),
    "uspace_groupnorm_map_bf16": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _F, _P]),
    "uspace_vae_num_params": (_I, [ctypes.POINTER(VaeConfig)]),
    "uspace_vae_param_numel": (_L, [ctypes.POINTER(VaeConfig), _I]),
    "uspace_vae_weight_bytes": (_SZ, [ctypes.POINTER(VaeConfig)]),
    "uspace_vae_workspace_bytes": (_SZ, [ctypes.POINTER(VaeConfig), _I]),
    "uspace_vae_pack_weights": (_I, [ctypes.POINTER(VaeConfig), ctypes.POINTER(_P), _I, _P, _SZ, _P]),
    "uspace_vae_decode": (_I, [ctypes.POINTER(VaeConfig), _P, _P, _SZ, _P, _F, _P, _I, _P]),
    "uspace_vae_decode_tap": (_I, [ctypes.POINTER(VaeConfig), _P, _P, _SZ, _P, _F, _I, _I, _P, ctypes.POINTER(_I), _P]),
    "uspace_vae_enc_num_params": (_I, [ctypes.POINTER(VaeConfig)]),
    "uspace_vae_enc_param_numel": (_L, [ctypes.POINTER(VaeConfig), _I]),
    "uspace_vae_enc_weight_bytes": (_SZ, [ctypes.POINTER(VaeConfig)]),
    "uspace_vae_enc_workspace_bytes": (_SZ, [ctypes.POINTER(VaeConfig), _I]),
    "uspace_vae_enc_pack_weights": (_I, [ctypes.POINTER(VaeConfig), ctypes.POINTER(_P), _I, _P, _SZ, _P]),
    "uspace_vae_encode_moments": (_I, [ctypes.POINTER(VaeConfig), _P, _P, _SZ, _P, _P, _I, _P]),
    "uspace_vae_encode_tap": (_I, [ctypes.POINTER(VaeConfig), _P, _P, _SZ, _P, _I, _I, _P, ctypes.POINTER(_I), _P]),
    "uspace_inception_num_params": (_I, []),
    "uspace_inception_param_numel": (_L, [_I]),
    "uspace_inception_weight_bytes": (_SZ, []),
    "uspace_inception_workspace_bytes": (_SZ, [_I, _I, _I]),
    "uspace_inception_pack_weights": (_I, [ctypes.POINTER(_P), _I, _P, _SZ, _P]),
    "uspace_inception_forward": (_I, [_P, _P, _SZ, _P, _I, _I, _I, _I, _P, _P]),
    "uspace_inception_tap": (_I, [_P, _P, _SZ, _P, _I, _I, _I, _I, _P, _P]),
    "uspace_fid_stats_accumulate": (_I, [_P, _I, _I, _P, _P, _P, _P]),
    "uspace_vae_sample": (_I, [_P, _P, _F, _P, _I, _I, _P]),
    "uspace_clip_num_params": (_I, [ctypes.POINTER(ClipConfig)]),
    "uspace_clip_param_numel": (_L, [ctypes.POINTER(ClipConfig), _I]),
    "uspace_clip_weight_bytes": (_SZ, [ctypes.POINTER(ClipConfig)]),
    "uspace_clip_workspace_bytes": (_SZ, [ctypes.POINTER(ClipConfig), _I]),
    "uspace_clip_pack_weights": (_I, [ctypes.POINTER(ClipConfig), _P, _I, _P, _SZ, _P]),
    "uspace_clip_text_forward": (_I, [ctypes.POINTER(ClipConfig), _P, _P, _SZ, _P, _P, _I, _I, _I, _P]),
    "uspace_attention_causal_bf16": (_I, [_P, _P, _I, _I, _I, _P]),
    "uspace_layernorm_f32": (_I, [_P, _P, _P, _P, _I, _I, _F, _P]),
    "uspace_table_embed": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "uspace_quick_gelu_bf16": (_I, [_P, _L, _P]),
    "uspace_clipv_num_params": (_I, [ctypes.POINTER(ClipVisionConfig)]),
    "uspace_clipv_param_numel": (_L, [ctypes.POINTER(ClipVisionConfig), _I]),
    "uspace_clipv_weight_bytes": (_SZ, [ctypes.POINTER(ClipVisionConfig)]),
    "uspace_clipv_workspace_bytes": (_SZ, [ctypes.POINTER(ClipVisionConfig), _I]),
    "uspace_clipv_pack_weights": (_I, [ctypes.POINTER(ClipVisionConfig), _P, _I, _P, _SZ, _P]),
    "uspace_clipv_forward": (_I, [ctypes.POINTER(ClipVisionConfig), _P, _P, _SZ, _P, _P, _P, _I, _I, _P, _P]),
    "uspace_clip_preprocess": (_I, [_P, _P, _I, _I, _I, _I, _I, ctypes.POINTER(_F), ctypes.POINTER(_F), _P]),
    "uspace_linear_f32": (_I, [_P, _P, _P, _I, _I, _I, _P]),
    "uspace_gather_rows_f32": (_I, [_P, _P, _P, _I, _I, _I, _P]),
    "uspace_cosine_f32": (_I, [_P, _P, _P, _I, _I, _F, _I, _P]),
    "uspace_normalized_diff_f32": (_I, [_P, _P, _P, _I, _I, _P]),
    "uspace_metric_workspace_bytes": (_SZ, [_I, _I, _I, _I]),
    "uspace_metric_knn_radius2": (_I, [_P, _I, _I, _I, _P, _P, _SZ, _P]),
    "uspace_metric_manifold": (_I, [_P, _I, _P, _I, _I, _P, _P, _P, _P, _SZ, _P]),
    "uspace_metric_poly_sums": (_I, [_P, _I, _P, _I, _I, _P, _P, _I, _I, _I, _D, _D, _P, _P, _SZ, _P]),
    "uspace_metric_rbf_sums": (_I, [_P, _I, _P, _I, _I, _D, _I, _P, _P, _SZ, _P]),
    "uspace_metric_topk": (_I, [_P, _I, _P, _I, _I, _I, _I, _I, _P, _P, _P, _SZ, _P]),
    "uspace_inception_forward_suite": (_I, [_P, _P, _SZ, _P, _I, _I, _I, _P, _P, _I, _I, _P]),
    "uspace_inception_logits": (_I, [_P, _P, _P, _P, _I, _I, _I, _P]),
    "uspace_inception_score_workspace_bytes": (_SZ, [_I, _I, _I]),
    "uspace_inception_score_f64": (_I, [_P, _I, _I, _I, _P, _SZ, _P, _P]),
    "uspace_lpips_num_params": (_I, [_I]),
    "uspace_lpips_param_numel": (_L, [_I, _I]),
    "uspace_lpips_weight_bytes": (_SZ, [_I]),
    "uspace_lpips_workspace_bytes": (_SZ, [_I, _I, _I, _I]),
    "uspace_lpips_pack_weights": (_I, [_I, ctypes.POINTER(_P), _I, _P, _SZ, _P]),
    "uspace_lpips_forward": (_I, [_I, _P, _P, _SZ, _P, _P, _I, _I, _I, _I, _P, _P, _P]),
    "uspace_lpips_tap": (_I, [_I, _P, _P, _SZ, _P, _P, _I, _I, _I, _I, _I, _P, _P]),
    "uspace_lpips_distance_workspace_bytes": (_SZ, [_I, _I, _I]),
    "uspace_lpips_distance_f64": (_I, [_P, _P, _P, _I, _I, _I, _P, _SZ, _P, _P]),
    "uspace_ssim_workspace_bytes": (_SZ, [_I, _I, _I, _I]),
    "uspace_ssim_f64": (_I, [_P, _P, _I, _I, _I, _I, _D, _P, _SZ, _P, _P]),
    "uspace_psnr_workspace_bytes": (_SZ, [_I, _L]),
    "uspace_psnr_f64": (_I, [_P, _P, _I, _L, _D, _P, _SZ, _P, _P]),
    "uspace_dino_num_params": (_I, [ctypes.POINTER(DinoConfig)]),
    "uspace_dino_param_numel": (_L, [ctypes.POINTER(DinoConfig), _I]),
    "uspace_dino_weight_bytes": (_SZ, [ctypes.POINTER(DinoConfig)]),
    "uspace_dino_workspace_bytes": (_SZ, [ctypes.POINTER(DinoConfig), _I]),
    "uspace_dino_pack_weights": (_I, [ctypes.POINTER(DinoConfig), _P, _I, _P, _SZ, _P]),
    "uspace_dino_forward": (_I, [ctypes.POINTER(DinoConfig), _P, _P, _SZ, _P, _P, _I, _I, _P, _I, _P, _P]),
    "uspace_self_similarity_mse_workspace_bytes": (_SZ, [_I, _I]),
    "uspace_self_similarity_mse_f64": (_I, [_P, _P, _I, _I, _I, _L, _L, _P, _SZ, _P, _P]),
    "uspace_idnet_num_params": (_I, [ctypes.POINTER(IdnetConfig)]),
    "uspace_idnet_param_numel": (_L, [ctypes.POINTER(IdnetConfig), _I]),
    "uspace_idnet_weight_bytes": (_SZ, [ctypes.POINTER(IdnetConfig)]),
    "uspace_idnet_workspace_bytes": (_SZ, [ctypes.POINTER(IdnetConfig), _I]),
    "uspace_idnet_pack_weights": (_I, [ctypes.POINTER(IdnetConfig), ctypes.POINTER(_P), _I, _P, _SZ, _P]),
    "uspace_idnet_preprocess": (_I, [_P, _I, _I, _I, _I, _I, _I, _P, _P]),
    "uspace_idnet_forward": (_I, [ctypes.POINTER(IdnetConfig), _P, _P, _SZ, _P, _I, _P, _P]),
    "uspace_idnet_tap": (_I, [ctypes.POINTER(IdnetConfig), _P, _P, _SZ, _P, _I, _I, _P, _P]),
    "uspace_idnet_unit_workspace_bytes": (_SZ, [ctypes.POINTER(IdnetConfig), _I, _I, _I, _I]),
    "uspace_idnet_unit": (_I, [ctypes.POINTER(IdnetConfig), _P, _P, _SZ, _I, _P, _I, _I, _I, _P, _P]),
    "uspace_idnet_similarity_f64": (_I, [_P, _P, _I, _P, _P]),
    "uspace_resnet_num_params": (_I, [ctypes.POINTER(ResnetConfig)]),
    "uspace_resnet_param_numel": (_L, [ctypes.POINTER(ResnetConfig), _I]),
    "uspace_resnet_weight_bytes": (_SZ, [ctypes.POINTER(ResnetConfig)]),
    "uspace_resnet_workspace_bytes": (_SZ, [ctypes.POINTER(ResnetConfig), _I, _I, _I]),
    "uspace_resnet_pack_weights": (_I, [ctypes.POINTER(ResnetConfig), ctypes.POINTER(_P), _I, _P, _SZ, _P]),
    "uspace_resnet_preprocess": (_I, [_P, _I, _I, _I, ctypes.POINTER(_F), ctypes.POINTER(_F), _P, _P]),
    "uspace_resnet_forward": (_I, [ctypes.POINTER(ResnetConfig), _P, _P, _SZ, _P, _I, _I, _I, _P, _P, _P]),
    "uspace_resnet_tap": (_I, [ctypes.POINTER(ResnetConfig), _P, _P, _SZ, _P, _I, _I, _I, _I, _P, _P]),
    "uspace_attr_effect_f64": (_I, [_P, _P, _P, _P, _P, _I, _I, _P, _P]),
    "uspace_attention_kv_plan": (_I, [_I, _I, _I, _I, ctypes.POINTER(_I)]),
    "uspace_attention_kv_bf16": (_I, [_P, _I, _P, _I, _P, _I, _I, _I, _I, _I, _P]),
    "uspace_dwconv3x3_gelu_bf16": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "uspace_bilinear_nhwc_f32": (_I, [_P, _I, _I, _I, _I, _P, _I, _I, _I, _I, _P]),
    "uspace_seg_labels_u8": (_I, [_P, _I, _I, _I, _I, _P, _I, _I, _P]),
    "uspace_seg_pair_counts": (_I, [_P, _P, _I, _L, _I, _P, _P]),
    "uspace_seg_region_sse_f64": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P]),
    "uspace_segformer_num_params": (_I, [ctypes.POINTER(SegformerConfig)]),
    "uspace_segformer_param_numel": (_L, [ctypes.POINTER(SegformerConfig), _I]),
    "uspace_segformer_weight_bytes": (_SZ, [ctypes.POINTER(SegformerConfig)]),
    "uspace_segformer_workspace_bytes": (_SZ, [ctypes.POINTER(SegformerConfig), _I, _I, _I]),
    "uspace_segformer_pack_weights": (_I, [ctypes.POINTER(SegformerConfig), ctypes.POINTER(_P), _I, _P, _SZ, _P]),
    "uspace_segformer_forward": (_I, [ctypes.POINTER(SegformerConfig), _P, _P, _SZ, _P, _I, _I, _I, _P, _P]),
    "uspace_segformer_num_stages": (_I, [ctypes.POINTER(SegformerConfig)]),
    "uspace_segformer_tap": (_I, [ctypes.POINTER(SegformerConfig), _P, _P, _SZ, _P, _I, _I, _I, _I, _P, _P]),
    "uspace_pair_blend": (_I, [_P, _P, _I, _I, _L, _P, _P]),
    "uspace_mask_from_labels": (_I, [_P, _I, _I, _I, _P, _I, _I, _F, _I, _P, _P]),
    "uspace_mask_from_maps": (_I, [_P, _I, _I, _I, _I, _P, _P, _I, _F, _I, _P, _P]),
    "uspace_prof_gemm_begin": (_I, [_I, _I, _I, _I]),
    "uspace_prof_gemm_end": (_I, [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_I)]),
    "uspace_prof_all_begin": (_I, [_I]),
    "uspace_prof_all_end": (_I, [ctypes.POINTER(_I), ctypes.POINTER(ctypes.c_double), _I, ctypes.POINTER(_I)]),
    "uspace_prof_dropped": (_L, []),
    "uspace_prof_mfma_peak": (_I, [_I, ctypes.POINTER(ctypes.c_double)]),
    "uspace_prof_mfma_peak_clock": (_I, [_I, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
    "uspace_prof_mfma_peak_gemm_op": (_I, [_I, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
    "uspace_prof_hbm_copy": (_I, [_SZ, _I, ctypes.POINTER(ctypes.c_double)]),
}

_lib = None


def lib():
    """Load libuspace_hip.so or raise -- the product path has no CPU / eager fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise UspaceHipError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). uspace_amd has no fallback path.")
        L = ctypes.CDLL(LIB_PATH)
        if os.path.realpath(LIB_PATH) != os.path.realpath(_DEFAULT_LIB):
            import sys
            print(f"uspace_amd: USPACE_HIP_LIB overrides the product library: loading {LIB_PATH} -- a lab build, results and timings are not the "
                  "product's", file=sys.stderr)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)  # AttributeError here = header/library mismatch
            fn.restype = res
            fn.argtypes = args
        if L.uspace_abi_version() != ABI_VERSION:
            raise UspaceHipError("libuspace_hip.so ABI version mismatch")
        # the library itself reads no environment: USPACE_LN_FOLD=0 selects the separate-LayerNorm path for A/B runs
        env = os.environ.get("USPACE_LN_FOLD")
        if env is not None and env != "":
            L.uspace_uvit_set_ln_fold(0 if env[0] == "0" else 1)
        env = os.environ.get("USPACE_GEMM_SK")   # ... USPACE_GEMM_SK=0 switches the GEMM's in-launch K-split tail off
        if env is not None and env != "":
            L.uspace_gemm_set_sk(0 if env[0] == "0" else 1)
        _lib = L
    return _lib


def library_info():
    """Which library is loaded: path, whether it is the in-tree product build, lab symbols it exports."""
    L = lib()
    lab = [s for s in ("uspace_lab_gemm_force_tile", "uspace_lab_gemm_trace") if hasattr(L, s)]
    return {"path": os.path.relpath(LIB_PATH, os.path.dirname(_HERE)), "product_build": os.path.realpath(LIB_PATH) == os.path.realpath(_DEFAULT_LIB),
            "lab_symbols": lab}


def check(rc, what):
    if rc != 0:
        raise UspaceHipError(f"{what} failed: {_ERR.get(rc, rc)}")


def stream_ptr():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def sync_current_stream():
    """Wait for the work enqueued so far on the stream the kernels are launched on."""
    torch.cuda.current_stream().synchronize()


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def require_device(t, name="tensor"):
    if not t.is_cuda:
        raise UspaceHipError(
            f"{name} lives on {t.device}: uspace_amd runs only on a ROCm device (MI355X); there is no CPU path")


# ------------------------------------------------------------------------------------------
# thin operator wrappers (used by the parity tests and by the solver); tensors are torch CUDA
# ------------------------------------------------------------------------------------------
def gemm(A, W, *, A2=None, bias=None, resid=None, gelu=False, out_f32=None, out_bf16=None, split_ws=None, sk_ws=None):
    """acc = [A|A2] @ W^T with fused epilogue; A/A2/W are torch.bfloat16, returns (out_f32, out_bf16).  split_ws: an optional
    fp32 workspace tensor (uspace_gemm_split_ws_bytes) that allows the K-split form of small launches.  sk_ws: an optional
    workspace tensor (uspace_gemm_sk_ws_bytes) that allows the in-launch K-split tail; its 256 arrival counters are made here."""
    require_device(A, "A")
    M, K1 = A.shape
    N, K = W.shape
    assert A.dtype == torch.bfloat16 and W.dtype == torch.bfloat16
    flags = 0
    if bias is not None:
        flags |= EPI_BIAS
    if gelu:
        flags |= EPI_GELU
    if resid is not None:
        flags |= EPI_RESIDUAL
    if out_f32 is not None:
        flags |= EPI_OUT_F32
    if out_bf16 is not None:
        flags |= EPI_OUT_BF16
    args = (ptr(A), A.stride(0), ptr(A2), A2.stride(0) if A2 is not None else 0, K1, ptr(W), W.stride(0), M, N, K, flags,
            ptr(bias), ptr(resid), resid.stride(0) if resid is not None else 0,
            ptr(out_f32), out_f32.stride(0) if out_f32 is not None else 0,
            ptr(out_bf16), out_bf16.stride(0) if out_bf16 is not None else 0)
    if split_ws is not None or sk_ws is not None:
        ext = GemmExt()
        if split_ws is not None:
            require_device(split_ws, "split_ws")
            ext.split_ws = ptr(split_ws).value
            ext.split_ws_bytes = split_ws.numel() * split_ws.element_size()
        if sk_ws is not None:
            require_device(sk_ws, "sk_ws")
            counters = torch.zeros(256, dtype=torch.int32, device=sk_ws.device)
            ext.sk_ws = ptr(sk_ws).value
            ext.sk_ws_bytes = sk_ws.numel() * sk_ws.element_size()
            ext.sk_counters = ptr(counters).value
        rc = lib().uspace_gemm_bf16_ext(*args, ctypes.byref(ext), stream_ptr())
    else:
        rc = lib().uspace_gemm_bf16(*args, stream_ptr())
    check(rc, "uspace_gemm_bf16")
    return out_f32, out_bf16


def gemm_slabs(A, W, row_shift, *, bias=None, resid=None, out_f32=None, out_bf16=None, M=None):
    """acc[m] = sum_t A[m + row_shift[t]] @ W[:, t*K1:(t+1)*K1]^T.  ``A`` points at row 0 of the map (the caller's
    buffer has guard rows around it); M rows are produced."""
    require_device(A, "A")
    K1 = A.shape[1]
    N = W.shape[0]
    n = len(row_shift)
    assert W.shape[1] == n * K1 and A.dtype == torch.bfloat16 and W.dtype == torch.bfloat16
    M = A.shape[0] if M is None else M
    flags = (EPI_BIAS if bias is not None else 0) | (EPI_RESIDUAL if resid is not None else 0) | \
            (EPI_OUT_F32 if out_f32 is not None else 0) | (EPI_OUT_BF16 if out_bf16 is not None else 0)
    shifts = (ctypes.c_int * n)(*[int(v) for v in row_shift])
    rc = lib().uspace_gemm_slabs_bf16(
        ptr(A), A.stride(0), ptr(W), W.stride(0), M, N, K1, n, shifts, flags, ptr(bias), ptr(resid),
        resid.stride(0) if resid is not None else 0, ptr(out_f32), out_f32.stride(0) if out_f32 is not None else 0,
        ptr(out_bf16), out_bf16.stride(0) if out_bf16 is not None else 0, stream_ptr())
    check(rc, "uspace_gemm_slabs_bf16")
    return out_f32, out_bf16


def layernorm(x, gamma, beta, eps=1e-5):
    require_device(x, "x")
    M, D = x.shape
    y = torch.empty(M, D, dtype=torch.bfloat16, device=x.device)
    check(lib().uspace_layernorm_f32_bf16(ptr(x), ptr(gamma), ptr(beta), ptr(y), M, D, eps, stream_ptr()),
          "uspace_layernorm_f32_bf16")
    return y


def attention(qkv, B, L, H, key_scale=None):
    require_device(qkv, "qkv")
    out = torch.empty(B * L, H * 64, dtype=torch.bfloat16, device=qkv.device)
    check(lib().uspace_attention_bf16(ptr(qkv), ptr(key_scale), ptr(out), B, L, H, stream_ptr()),
          "uspace_attention_bf16")
    return out


def attention_long(qkv, B, L, H, key_scale=None):
    """The streaming form of ``attention`` (K and V in key tiles, online softmax): any L; what the forward takes for L > 336."""
    require_device(qkv, "qkv")
    out = torch.empty(B * L, H * 64, dtype=torch.bfloat16, device=qkv.device)
    check(lib().uspace_attention_long_bf16(ptr(qkv), ptr(key_scale), ptr(out), B, L, H, stream_ptr()),
          "uspace_attention_long_bf16")
    return out


def attention_wide(q, k, v, B, N, C, scale, ld=None, out=None, ld_out=None):
    """Single-head attention with a wide head (C = 64 .. 512; the VAE's mid block beyond 1 024 tokens): q, k, v bf16 [B * N, ld]
    (``ld`` defaults to C), ``out`` bf16 [B * N, ld_out] (allocated [B * N, C] where None)."""
    require_device(q, "q")
    ld = C if ld is None else ld
    if out is None:
        out, ld_out = torch.empty(B * N, C, dtype=torch.bfloat16, device=q.device), C
    check(lib().uspace_attention_wide_bf16(ptr(q), ptr(k), ptr(v), ld, ptr(out), C if ld_out is None else ld_out, B, N, C,
                                           float(scale), stream_ptr()), "uspace_attention_wide_bf16")
    return out


def attention_map(qkv, B, L, H, q0, nq, k0, nk):
    """Head-mean softmax map of the packed bf16 qkv [B * L, 3 * H * 64]: rows q0 .. q0 + nq - 1, columns k0 .. k0 + nk - 1 of the
    [L, L] map (softmax over all L keys) -> fp32 [B, nq, nk]."""
    require_device(qkv, "qkv")
    assert qkv.dtype == torch.bfloat16 and qkv.is_contiguous() and qkv.numel() == B * L * 3 * H * 64
    out = torch.empty(B, max(int(nq), 0), max(int(nk), 0), dtype=torch.float32, device=qkv.device)
    check(lib().uspace_attention_map_bf16(ptr(qkv), ptr(out), B, L, H, int(q0), int(nq), int(k0), int(nk), stream_ptr()),
          "uspace_attention_map_bf16")
    return out


def add_broadcast(x, delta, scale, x_bf16=None, row_scale=None):
    """x[b] += scale * (row_scale[b] if given) * delta, in place."""
    require_device(x, "x")
    B = x.shape[0]
    per = x.numel() // B
    assert delta.numel() == per and delta.dtype == torch.float32 and x.dtype == torch.float32
    if row_scale is not None:
        assert row_scale.numel() == B and row_scale.dtype == torch.float32 and row_scale.is_cuda
    check(lib().uspace_add_broadcast_rows(ptr(x), ptr(x_bf16), ptr(delta), float(scale), ptr(row_scale), B, per,
                                          stream_ptr()), "uspace_add_broadcast_rows")
    return x


def cfg_combine(pair, scale, row_scale=None, out=None):
    """Classifier-free guidance of paired predictions: ``pair`` [2B, ...] fp32 with the conditional rows first ->
    out[b] = c + s_b (c - u), s_b = scale * (row_scale[b] if given); fp32 [B, ...]."""
    require_device(pair, "pair")
    if pair.dtype != torch.float32 or not pair.is_contiguous() or pair.shape[0] < 2 or pair.shape[0] % 2:
        raise ValueError(f"pair must be a contiguous fp32 tensor of 2B rows, got {pair.dtype} {tuple(pair.shape)}")
    B = pair.shape[0] // 2
    per = pair.numel() // (2 * B)
    if row_scale is not None and not (row_scale.numel() == B and row_scale.dtype == torch.float32 and row_scale.is_cuda
                                      and row_scale.is_contiguous()):
        raise ValueError(f"row_scale must be a contiguous fp32 device tensor of {B} entries")
    if out is None:
        out = torch.empty((B,) + tuple(pair.shape[1:]), dtype=torch.float32, device=pair.device)
    check(lib().uspace_cfg_combine(ptr(pair), ptr(row_scale), float(scale), ptr(out), B, per, stream_ptr()), "uspace_cfg_combine")
    return out


def uvit_forward_cfg(cfg, blob, ws, io, B, uncond, uncond_batched, scale, row_scale=None, pair_out=None):
    """``uspace_uvit_forward_cfg`` on the current stream: ``io`` (a ``UvitIO``) describes the B samples, ``ws`` is a uint8 tensor of
    ``uspace_uvit_cfg_workspace_bytes(cfg, B)`` bytes at least; the guided prediction lands in ``io.out``."""
    check(lib().uspace_uvit_forward_cfg(ctypes.byref(cfg), ptr(blob), ptr(ws), ws.numel(), ctypes.byref(io), B, ptr(uncond),
                                        1 if uncond_batched else 0, float(scale), ptr(row_scale), ptr(pair_out), stream_ptr()),
          "uspace_uvit_forward_cfg")


def cast_bf16(src):
    require_device(src, "src")
    dst = torch.empty(src.shape, dtype=torch.bfloat16, device=src.device)
    check(lib().uspace_cast_f32_bf16(ptr(src), ptr(dst), src.numel(), stream_ptr()), "uspace_cast_f32_bf16")
    return dst


def _ode_operands(what, ks, coefs):
    # ctypes zero-fills an array built from fewer values than its length: a short coefficient list would drop terms silently
    if len(coefs) != len(ks):
        raise UspaceHipError(f"{what}: {len(coefs)} coefficients for {len(ks)} operands")


def ode_combine(out, y, ks, coefs):
    _ode_operands("ode_combine", ks, coefs)
    require_device(y, "y")
    n = len(ks)
    karr = (ctypes.c_void_p * max(n, 1))(*[k.data_ptr() for k in ks])
    carr = (ctypes.c_float * max(n, 1))(*[float(c) for c in coefs])
    check(lib().uspace_ode_combine(ptr(out), ptr(y), karr, carr, n, y.numel(), stream_ptr()), "uspace_ode_combine")
    return out


def ode_error_norm(y0, y1, ks, coefs, rtol, atol, scratch, result):
    """``result``: device float[2] = [rms, sum of squares]."""
    _ode_operands("ode_error_norm", ks, coefs)
    if result.numel() < 2:
        raise UspaceHipError("ode_error_norm: result must hold 2 floats (ABI 6)")
    if scratch.numel() < 1024:
        raise UspaceHipError("ode_error_norm: scratch must hold 1024 floats (one partial per block)")
    n = len(ks)
    karr = (ctypes.c_void_p * n)(*[k.data_ptr() for k in ks])
    carr = (ctypes.c_float * n)(*[float(c) for c in coefs])
    check(lib().uspace_ode_error_norm(ptr(y0), ptr(y1), karr, carr, n, float(rtol), float(atol), y0.numel(),
                                      ptr(scratch), ptr(result), stream_ptr()), "uspace_ode_error_norm")
    return result


def _metric_features(t, name):
    require_device(t, name)
    if t.dtype != torch.float32 or t.dim() != 2 or not t.is_contiguous() or t.shape[0] < 1 or t.shape[1] < 1:
        raise UspaceHipError(f"{name} must be a contiguous fp32 [n, F] tensor with n, F >= 1, got {t.dtype} {tuple(t.shape)}")


def metric_workspace(nx, ny=0, n_subsets=0, m=0, device=None, fill=None):
    """A uint8 workspace tensor of ``uspace_metric_workspace_bytes(nx, ny, n_subsets, m)`` bytes (``fill``: a byte value to set it
    to; the kernels read nothing of it that they have not written)."""
    nbytes = lib().uspace_metric_workspace_bytes(int(nx), int(ny), int(n_subsets), int(m))
    if nbytes == 0:
        raise UspaceHipError(f"uspace_metric_workspace_bytes({nx}, {ny}, {n_subsets}, {m}): invalid sizes")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    if fill is not None:
        ws.fill_(fill)
    return ws


def metric_knn_radius2(x, k, ws=None):
    """fp64 [n]: the k-th smallest squared distance of every row of ``x`` (fp32 [n, F]) to the other rows, self excluded by index."""
    _metric_features(x, "x")
    n, F = x.shape
    if ws is None:
        ws = metric_workspace(n, device=x.device)
    out = torch.empty(n, dtype=torch.float64, device=x.device)
    check(lib().uspace_metric_knn_radius2(ptr(x), n, F, int(k), ptr(out), ptr(ws), ws.numel(), stream_ptr()),
          "uspace_metric_knn_radius2")
    return out


def metric_manifold(x, y, radius2_y=None, *, want_count=True, want_min=True, ws=None):
    """(count int32 [nx] or None, min_d2 fp64 [nx] or None) of the rows of ``x`` against the set ``y``: count[i] = the number of j
    with D2(i, j) <= radius2_y[j], min_d2[i] = min_j D2(i, j)."""
    _metric_features(x, "x")
    _metric_features(y, "y")
    if x.shape[1] != y.shape[1]:
        raise UspaceHipError(f"feature widths differ: {x.shape[1]} and {y.shape[1]}")
    nx, F = x.shape
    ny = y.shape[0]
    if radius2_y is not None:
        require_device(radius2_y, "radius2_y")
        if radius2_y.dtype != torch.float64 or radius2_y.numel() != ny or not radius2_y.is_contiguous():
            raise UspaceHipError(f"radius2_y must be a contiguous fp64 tensor of {ny} entries")
    if ws is None:
        ws = metric_workspace(nx, ny, device=x.device)
    count = torch.empty(nx, dtype=torch.int32, device=x.device) if want_count else None
    min_d2 = torch.empty(nx, dtype=torch.float64, device=x.device) if want_min else None
    check(lib().uspace_metric_manifold(ptr(x), nx, ptr(y), ny, F, ptr(radius2_y), ptr(count), ptr(min_d2), ptr(ws), ws.numel(),
                                       stream_ptr()), "uspace_metric_manifold")
    return count, min_d2


def metric_poly_sums(x, y, idx_x, idx_y, degree, gamma, coef0, ws=None):
    """fp64 [n_subsets, 3]: the sums of (gamma a.b + coef0)^degree over the pairs of every subset -- x with x and y with y without
    the positions p == q, x with y over all.  idx_x, idx_y: device int32 [n_subsets, m], validated by the caller."""
    _metric_features(x, "x")
    _metric_features(y, "y")
    if x.shape[1] != y.shape[1]:
        raise UspaceHipError(f"feature widths differ: {x.shape[1]} and {y.shape[1]}")
    for t, name in ((idx_x, "idx_x"), (idx_y, "idx_y")):
        require_device(t, name)
        if t.dtype != torch.int32 or t.dim() != 2 or not t.is_contiguous() or t.shape != idx_x.shape:
            raise UspaceHipError(f"{name} must be a contiguous int32 [n_subsets, m] tensor, got {t.dtype} {tuple(t.shape)}")
    n_subsets, m = idx_x.shape
    if ws is None:
        ws = metric_workspace(x.shape[0], y.shape[0], n_subsets, m, device=x.device)
    sums = torch.empty(n_subsets, 3, dtype=torch.float64, device=x.device)
    check(lib().uspace_metric_poly_sums(ptr(x), x.shape[0], ptr(y), y.shape[0], x.shape[1], ptr(idx_x), ptr(idx_y), n_subsets, m,
                                        int(degree), float(gamma), float(coef0), ptr(sums), ptr(ws), ws.numel(), stream_ptr()),
          "uspace_metric_poly_sums")
    return sums


def metric_rbf_sums(x, y, gamma, normalize=False, ws=None):
    """fp64 [3]: the sums of exp(-gamma D2(a, b)) over the pairs of x with x and of y with y without i == j, and of x with y over
    all; ``normalize``: D2 between the rows scaled to unit length in fp64 (a zero row counts as the zero vector)."""
    _metric_features(x, "x")
    _metric_features(y, "y")
    if x.shape[1] != y.shape[1]:
        raise UspaceHipError(f"feature widths differ: {x.shape[1]} and {y.shape[1]}")
    nx, ny = x.shape[0], y.shape[0]
    if ws is None:
        ws = metric_workspace(nx, ny, 1, max(nx, ny), device=x.device)
    sums = torch.empty(3, dtype=torch.float64, device=x.device)
    check(lib().uspace_metric_rbf_sums(ptr(x), nx, ptr(y), ny, x.shape[1], float(gamma), 1 if normalize else 0, ptr(sums), ptr(ws),
                                       ws.numel(), stream_ptr()), "uspace_metric_rbf_sums")
    return sums


def metric_topk(x, y, k, index_base=0, self_base=-1, ws=None):
    """(d2 fp64 [nx, k], idx int32 [nx, k]): the k nearest rows of ``y`` for every row of ``x`` in the order (d2, index), the
    distances refined to sum (x - y)^2 in fp64; idx holds ``index_base`` + the row of ``y``; ``self_base`` >= 0 leaves out the column
    with index_base + j == self_base + i.  A row with fewer than k eligible columns ends in (+inf, -1)."""
    _metric_features(x, "x")
    _metric_features(y, "y")
    if x.shape[1] != y.shape[1]:
        raise UspaceHipError(f"feature widths differ: {x.shape[1]} and {y.shape[1]}")
    nx, F = x.shape
    ny = y.shape[0]
    if ws is None:
        ws = metric_workspace(nx, ny, device=x.device)
    k = int(k)
    d2 = torch.empty(nx, max(k, 0), dtype=torch.float64, device=x.device)
    idx = torch.empty(nx, max(k, 0), dtype=torch.int32, device=x.device)
    check(lib().uspace_metric_topk(ptr(x), nx, ptr(y), ny, F, k, int(index_base), int(self_base), ptr(d2), ptr(idx), ptr(ws),
                                   ws.numel(), stream_ptr()), "uspace_metric_topk")
    return d2, idx


def inception_logits(pool, weight, bias=None):
    """fp32 [B, C] = pool [B, K] @ weight [C, K]^T (+ bias [C]): the k-ordered fp32 fma chain per logit, no activation."""
    for t, name in ((pool, "pool"), (weight, "weight")) + (((bias, "bias"),) if bias is not None else ()):
        require_device(t, name)
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise UspaceHipError(f"{name} must be a contiguous fp32 tensor, got {t.dtype} {tuple(t.shape)}")
    if pool.dim() != 2 or weight.dim() != 2 or pool.shape[1] != weight.shape[1] or pool.shape[0] < 1:
        raise UspaceHipError(f"expected pool [B, K] and weight [C, K], got {tuple(pool.shape)} and {tuple(weight.shape)}")
    B, K = pool.shape
    C = weight.shape[0]
    if bias is not None and tuple(bias.shape) != (C,):
        raise UspaceHipError(f"bias must have {C} entries, got {tuple(bias.shape)}")
    out = torch.empty(B, C, dtype=torch.float32, device=pool.device)
    check(lib().uspace_inception_logits(ptr(pool), ptr(weight), ptr(bias), ptr(out), B, K, C, stream_ptr()),
          "uspace_inception_logits")
    return out


def inception_score_splits(logits, splits, ws=None):
    """fp64 [splits] on the device: the per-split scores of ``uspace_inception_score_f64`` for fp32 logits [N, C]."""
    require_device(logits, "logits")
    if logits.dtype != torch.float32 or logits.dim() != 2 or not logits.is_contiguous():
        raise UspaceHipError(f"logits must be a contiguous fp32 [N, C] tensor, got {logits.dtype} {tuple(logits.shape)}")
    N, C = logits.shape
    if ws is None:
        nbytes = lib().uspace_inception_score_workspace_bytes(N, C, int(splits))
        if nbytes == 0:
            raise UspaceHipError(f"uspace_inception_score_workspace_bytes({N}, {C}, {splits}): invalid sizes")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=logits.device)
    scores = torch.empty(int(splits), dtype=torch.float64, device=logits.device)
    check(lib().uspace_inception_score_f64(ptr(logits), N, C, int(splits), ptr(ws), ws.numel(), ptr(scores), stream_ptr()),
          "uspace_inception_score_f64")
    return scores


def attention_kv_plan(B, Lq, Lk, H):
    """dict(NT, NW, chunk, nchunks, grid, block, lds): what ``attention_kv`` launches for these sizes (no device needed)."""
    out = (ctypes.c_int * 7)()
    check(lib().uspace_attention_kv_plan(int(B), int(Lq), int(Lk), int(H), out), "uspace_attention_kv_plan")
    return dict(zip(("NT", "NW", "chunk", "nchunks", "grid", "block", "lds"), out))


def attention_kv(q, kv, H, out=None):
    """Attention of many queries over few resident keys: q bf16 [B, Lq, ldq >= 64 H], kv bf16 [B, Lk, ldkv >= 128 H] (k | v),
    Lk <= 336 -> bf16 [B, Lq, 64 H] (``out``: a bf16 [B, Lq, ldo] tensor to write the first 64 H columns of)."""
    for t, name in ((q, "q"), (kv, "kv")) + (((out, "out"),) if out is not None else ()):
        require_device(t, name)
        if t.dtype != torch.bfloat16 or t.dim() != 3 or not t.is_contiguous() or t.shape[0] != q.shape[0]:
            raise UspaceHipError(f"{name} must be a contiguous bf16 [B, rows, columns] tensor, got {t.dtype} {tuple(t.shape)}")
    B, Lq, ldq = q.shape
    if out is None:
        out = torch.empty(B, Lq, int(H) * 64, dtype=torch.bfloat16, device=q.device)
    if out.shape[1] != Lq:
        raise UspaceHipError(f"out must have {Lq} rows per sample, got {tuple(out.shape)}")
    check(lib().uspace_attention_kv_bf16(ptr(q), ldq, ptr(kv), kv.shape[2], ptr(out), out.shape[2], B, Lq, kv.shape[1], int(H),
                                         stream_ptr()), "uspace_attention_kv_bf16")
    return out


def _seg_tensor(t, name, dtype, dims):
    require_device(t, name)
    if t.dtype != dtype or t.dim() != dims or not t.is_contiguous() or t.numel() < 1:
        raise UspaceHipError(f"{name} must be a contiguous {dtype} tensor of {dims} dimensions, got {t.dtype} {tuple(t.shape)}")


def dwconv3x3_gelu(x, w, bias):
    """bf16 NHWC [B, H, W, C] -> GELU(depthwise 3 x 3 convolution + bias), zero padding 1, bf16 NHWC; ``w`` fp32 [9, C] (tap
    ty * 3 + tx), ``bias`` fp32 [C]; C a multiple of 8."""
    _seg_tensor(x, "x", torch.bfloat16, 4)
    _seg_tensor(w, "w", torch.float32, 2)
    _seg_tensor(bias, "bias", torch.float32, 1)
    B, H, W, C = x.shape
    if tuple(w.shape) != (9, C) or tuple(bias.shape) != (C,):
        raise UspaceHipError(f"expected w [9, {C}] and bias [{C}], got {tuple(w.shape)} and {tuple(bias.shape)}")
    y = torch.empty_like(x)
    check(lib().uspace_dwconv3x3_gelu_bf16(ptr(x), ptr(w), ptr(bias), ptr(y), B, H, W, C, stream_ptr()), "uspace_dwconv3x3_gelu_bf16")
    return y


def bilinear_nhwc(x, size, out=None, coff=0):
    """fp32 NHWC [B, h, w, C] -> bilinear (align_corners=False) at ``size`` = (Ho, Wo), written to channels coff .. coff + C - 1 of
    ``out`` fp32 [B, Ho, Wo, ldo] (allocated [B, Ho, Wo, C] where None): a concatenation is filled slice by slice, never copied."""
    _seg_tensor(x, "x", torch.float32, 4)
    B, h, w, C = x.shape
    Ho, Wo = (int(v) for v in size)
    if out is None:
        out = torch.empty(B, Ho, Wo, C, dtype=torch.float32, device=x.device)
    _seg_tensor(out, "out", torch.float32, 4)
    if tuple(out.shape[:3]) != (B, Ho, Wo):
        raise UspaceHipError(f"out must be [{B}, {Ho}, {Wo}, ldo], got {tuple(out.shape)}")
    check(lib().uspace_bilinear_nhwc_f32(ptr(x), B, h, w, C, ptr(out), Ho, Wo, out.shape[3], int(coff), stream_ptr()),
          "uspace_bilinear_nhwc_f32")
    return out


def seg_labels(logits, size):
    """uint8 [B, H, W]: the argmax (lowest index on ties) over the channels of ``logits`` fp32 NHWC [B, h, w, L], L <= 256,
    resampled to ``size`` = (H, W) as ``bilinear_nhwc`` does; the resampled logits are never stored."""
    _seg_tensor(logits, "logits", torch.float32, 4)
    B, h, w, L = logits.shape
    H, W = (int(v) for v in size)
    labels = torch.empty(B, max(H, 0), max(W, 0), dtype=torch.uint8, device=logits.device)
    check(lib().uspace_seg_labels_u8(ptr(logits), B, h, w, L, ptr(labels), H, W, stream_ptr()), "uspace_seg_labels_u8")
    return labels


def _label_maps(la, lb):
    for t, name in ((la, "la"), (lb, "lb")):
        require_device(t, name)
        if t.dtype != torch.uint8 or t.dim() < 2 or not t.is_contiguous() or t.shape != la.shape or t.numel() < 1:
            raise UspaceHipError(f"{name} must be a contiguous uint8 [B, ...] label map, both of one shape, got {t.dtype} {tuple(t.shape)}")


def seg_pair_counts(la, lb, num_labels):
    """int32 [B, 3, L] on the device: per pair of label maps uint8 [B, ...] the pixels of each label in a, in b, and in both."""
    _label_maps(la, lb)
    B, L = la.shape[0], int(num_labels)
    counts = torch.empty(B, 3, max(L, 0), dtype=torch.int32, device=la.device)
    check(lib().uspace_seg_pair_counts(ptr(la), ptr(lb), B, la[0].numel(), L, ptr(counts), stream_ptr()), "uspace_seg_pair_counts")
    return counts


def seg_region_sse(img_a, img_b, la, lb, member):
    """fp64 [B, 2] on the device: (sum of squared differences over the 3 channels, pixel count) of images fp32 [B, 3, H, W] over the
    pixels whose label (uint8 [B, H, W]) is in the set ``member`` (uint8 [L], nonzero = in) in neither map."""
    _label_maps(la, lb)
    _seg_tensor(img_a, "img_a", torch.float32, 4)
    _seg_tensor(img_b, "img_b", torch.float32, 4)
    _seg_tensor(member, "member", torch.uint8, 1)
    B, _, H, W = img_a.shape
    if img_a.shape != img_b.shape or img_a.shape[1] != 3 or tuple(la.shape) != (B, H, W):
        raise UspaceHipError(f"expected images [B, 3, H, W] and label maps [B, H, W], got {tuple(img_a.shape)}, {tuple(img_b.shape)} "
                             f"and {tuple(la.shape)}")
    out = torch.empty(B, 2, dtype=torch.float64, device=img_a.device)
    check(lib().uspace_seg_region_sse_f64(ptr(img_a), ptr(img_b), ptr(la), ptr(lb), ptr(member), member.numel(), B, H, W, ptr(out),
                                          stream_ptr()), "uspace_seg_region_sse_f64")
    return out


def pair_blend(pair, mask, out=None):
    """The velocity blend of a paired solve: ``pair`` fp32 [2B, C, ...] (source rows first), ``mask`` fp32 [B, cells] (or [B, ...] of
    that many cells) -> ``out`` (``pair`` itself where None: in place) with the source rows unchanged and row B + b the edited row
    where the mask is 1, the source row where it is 0, fmaf(m, e - s, s) between."""
    require_device(pair, "pair")
    if pair.dtype != torch.float32 or not pair.is_contiguous() or pair.dim() < 2 or pair.shape[0] < 2 or pair.shape[0] % 2:
        raise ValueError(f"pair must be a contiguous fp32 [2B, C, ...] tensor, got {pair.dtype} {tuple(pair.shape)}")
    B, C = pair.shape[0] // 2, pair.shape[1]
    cells = pair.numel() // (2 * B * C)
    if not (mask.is_cuda and mask.dtype == torch.float32 and mask.is_contiguous() and mask.numel() == B * cells):
        raise ValueError(f"mask must be a contiguous fp32 device tensor of {B} x {cells} entries, got {mask.dtype} {tuple(mask.shape)}")
    if out is None:
        out = pair
    elif out.dtype != torch.float32 or not out.is_contiguous() or out.shape != pair.shape or not out.is_cuda:
        raise ValueError(f"out must be a contiguous fp32 device tensor like pair, got {out.dtype} {tuple(out.shape)}")
    check(lib().uspace_pair_blend(ptr(pair), ptr(mask), B, C, cells, ptr(out), stream_ptr()), "uspace_pair_blend")
    return out


def mask_from_labels(labels, member, S, dilate=0, thr=0.0, soft=False):
    """fp32 [B, S, S]: per latent cell the share of pixels of ``labels`` (uint8 [B, H, W]) whose label is in ``member`` (uint8 [256],
    nonzero = in), dilated by a maximum over (2 dilate + 1)^2 cells; ``soft`` keeps the share, otherwise share > thr."""
    _seg_tensor(labels, "labels", torch.uint8, 3)
    _seg_tensor(member, "member", torch.uint8, 1)
    if member.numel() != 256:
        raise UspaceHipError(f"member must have 256 entries, got {member.numel()}")
    B, H, W = labels.shape
    mask = torch.empty(B, max(int(S), 0), max(int(S), 0), dtype=torch.float32, device=labels.device)
    check(lib().uspace_mask_from_labels(ptr(labels), B, H, W, ptr(member), int(S), int(dilate), float(thr), 1 if soft else 0, ptr(mask),
                                        stream_ptr()), "uspace_mask_from_labels")
    return mask


def mask_from_maps(maps, block_w, cols, G, patch, thr=0.3, soft=False):
    """fp32 [R, G * patch, G * patch] from attention maps fp32 [n_blocks, R, G * G, nk], block weights fp32 [n_blocks] and token
    columns fp32 [R, nk]: the weighted maps summed over the chosen columns, 3 x 3 max-pooled, divided by the row's maximum,
    thresholded (``soft``: not), spread over patch x patch latent cells."""
    for t, name in ((maps, "maps"), (block_w, "block_w"), (cols, "cols")):
        require_device(t, name)
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise UspaceHipError(f"{name} must be a contiguous fp32 tensor, got {t.dtype} {tuple(t.shape)}")
    G, patch = int(G), int(patch)
    if maps.dim() != 4 or maps.shape[2] != G * G or tuple(block_w.shape) != (maps.shape[0],) or tuple(cols.shape) != (maps.shape[1], maps.shape[3]):
        raise UspaceHipError(f"expected maps [n_blocks, R, {G * G}, nk], block_w [n_blocks] and cols [R, nk], got {tuple(maps.shape)}, "
                             f"{tuple(block_w.shape)} and {tuple(cols.shape)}")
    n_blocks, R, _, nk = maps.shape
    side = max(G * patch, 0)
    mask = torch.empty(R, side, side, dtype=torch.float32, device=maps.device)
    check(lib().uspace_mask_from_maps(ptr(maps), n_blocks, R, G, nk, ptr(block_w), ptr(cols), patch, float(thr), 1 if soft else 0,
                                      ptr(mask), stream_ptr()), "uspace_mask_from_maps")
    return mask


def prof_gemm_begin(epi_flags, N, K, max_launches=8192):
    check(lib().uspace_prof_gemm_begin(epi_flags, N, K, max_launches), "uspace_prof_gemm_begin")


def prof_peaks(mfma_iters=20000, copy_bytes=1 << 30, copy_reps=10):
    """(dense bf16 MFMA TFLOP/s of a v_mfma_f32_32x32x16_bf16-only loop, stream-copy GB/s read + write, sustained shader
    clock in GHz under the MFMA loop) measured on the current device."""
    tf, gb, ghz = ctypes.c_double(0.0), ctypes.c_double(0.0), ctypes.c_double(0.0)
    check(lib().uspace_prof_mfma_peak_clock(mfma_iters, ctypes.byref(tf), ctypes.byref(ghz)), "uspace_prof_mfma_peak_clock")
    check(lib().uspace_prof_hbm_copy(copy_bytes, copy_reps, ctypes.byref(gb)), "uspace_prof_hbm_copy")
    return tf.value, gb.value, ghz.value


def prof_mfma_gemm_op(mfma_iters=20000):
    """(TFLOP/s, sustained shader GHz) of a v_mfma_f32_16x16x32_bf16-only loop on pseudo-random operands: the GEMM's instruction on
    data that toggles like real activations (prof_peaks() times v_mfma_f32_32x32x16_bf16 on near-constant operands)."""
    tf, ghz = ctypes.c_double(0.0), ctypes.c_double(0.0)
    check(lib().uspace_prof_mfma_peak_gemm_op(mfma_iters, ctypes.byref(tf), ctypes.byref(ghz)), "uspace_prof_mfma_peak_gemm_op")
    return tf.value, ghz.value


def prof_all_begin(max_launches=16384):
    check(lib().uspace_prof_all_begin(max_launches), "uspace_prof_all_begin")


def prof_dropped():
    """Launches the recorder could not take (it was full) since the last prof_*_begin()."""
    return int(lib().uspace_prof_dropped())


def prof_all_end(max_records=256):
    """-> list of dicts(kind, flags, M, N, K, launches, total_ms), one per distinct (kind, flags, M, N, K)."""
    keys = (ctypes.c_int * (6 * max_records))()
    ms = (ctypes.c_double * max_records)()
    n = ctypes.c_int(0)
    check(lib().uspace_prof_all_end(keys, ms, max_records, ctypes.byref(n)), "uspace_prof_all_end")
    return [dict(kind=keys[6 * i], flags=keys[6 * i + 1], M=keys[6 * i + 2], N=keys[6 * i + 3], K=keys[6 * i + 4],
                 launches=keys[6 * i + 5], total_ms=ms[i]) for i in range(n.value)]


def prof_gemm_end():
    ms, n = ctypes.c_double(0.0), ctypes.c_int(0)
    check(lib().uspace_prof_gemm_end(ctypes.byref(ms), ctypes.byref(n)), "uspace_prof_gemm_end")
    return ms.value, n.value
