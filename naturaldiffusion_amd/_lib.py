"""ctypes binding of libnatinf.so (include/natinf.h, include/natinf_ncsnpp.h).

The product path fails loudly: no library -> ImportError with the build command; a negative
return code -> RuntimeError naming the entry point.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

# The HIP runtime multiplexes a process's streams onto GPU_MAX_HW_QUEUES hardware queues (default 4); two streams that share a queue run one after the other.
# The engines count on concurrency between a few streams (the two lanes of the CIFAR10 pipeline, the MMDiT's text stream beside its image stream) next to whatever
# streams the host framework made: ask for eight unless the user chose.  It only takes effect when set before the process's first HIP call.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

_HERE = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ.get("NATINF_LIB", _HERE / "libnatinf.so"))

if not LIB_PATH.exists():
    raise ImportError(
        f"{LIB_PATH} not found: build it with `make -C {_HERE / 'csrc'}` "
        "(or `python -c 'import __graft_entry__ as g; g.build()'`). "
        "naturaldiffusion_amd has no CPU or eager-PyTorch fallback.")

lib = C.CDLL(str(LIB_PATH))

_p, _i32, _i64, _f32, _f64 = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_double

SIGNATURES = {
    "natinf_abi_version": (C.c_int, []),
    "natinf_strerror": (C.c_char_p, [_i32]),
    "natinf_probe": (C.c_int, []),
    "natinf_step_f64hist": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _i32, _f64, _i32, _f64, _f64, _f32, _f32, _i64, _p]),
    "natinf_step_f32hist": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _i32, _f32, _i32, _f32, _f32, _f32, _f32, _i64, _p]),
    "natinf_weighted_sum_f64": (C.c_int, [_p, _p, _p, _p, _i32, _i64, _p]),
    "natinf_randn_philox_f32": (C.c_int, [_p, _i64, _i64, _p, _i64, _i64, C.c_uint64, _p]),
    "natinf_randn_philox_col_f32": (C.c_int, [_p, _i64, _i64, _p, _i64, _i64, C.c_uint64, C.c_uint32, _p]),
    "natinf_step_f64hist_noise": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _i32, _f64, _p, _p, _i32, _i32, _f64, _f64, _f32,
                                            C.c_uint64, _p, _i64, _i64, _i64, _i64, _p]),
    "natinf_known_blend_f32": (C.c_int, [_p, _p, _p, _p, _i64, _i64, _f32, _f32, C.c_uint32, C.c_uint64, _p, _i64, _i64, _i64, _i64, _p]),
    "natinf_step_f64hist_inpaint": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _i32, _f64, _p, _p, _i32, _i32, _f64, _f64, _f32,
                                              C.c_uint64, _p, _i64, _i64, _i64, _i64, _p, _p, _i64, _i64, _f32, _f32, C.c_uint32, _p]),
    "natinf_x0_threshold_f64": (C.c_int, [_p, _p, _i64, _i64, _i32, _f64, _f64, _p]),
    "natinf_step_f64hist_x0fix": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _i32, _f64, _p, _p, _i32, _i32, _f64, _f64, _f32,
                                            C.c_uint64, _p, _i64, _i64, _i64, _i64, _p, _p, _i64, _i64, _f32, _f32, C.c_uint32,
                                            _i32, _f64, _f64, _p, _p]),
    "natinf_x0_project_f64": (C.c_int, [_p, _p, _p, _i64, _i32, _i32, _i32, _i32, _i64, _p]),
    "natinf_step_f64hist_project": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _i32, _f64, _p, _p, _i32, _i32, _f64, _f64, _f32,
                                              C.c_uint64, _p, _i64, _i64, _i64, _i64, _p, _i64, _i32, _i32, _i32, _i32, _p, _p]),
    "natinf_color_blend_f32": (C.c_int, [_p, _p, _p, _i64, _p, _p, _f32, _f32, C.c_uint32, C.c_uint64, _p, _i64, _i64, _i64, _i64, _p]),
    "natinf_step_f64hist_colorize": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _i32, _f64, _p, _p, _i32, _i32, _f64, _f64, _f32,
                                               C.c_uint64, _p, _i64, _i64, _i64, _i64, _p, _i64, _p, _p, _f32, _f32, C.c_uint32, _p]),
    "natinf_to_pixel_u8": (C.c_int, [_p, _p, _i32, _i32, _i32, _i32, _i32, _p]),
    "natinf_step_f32prod": (C.c_int, [_p, _p, _p, _f32, _i64, _i64, _p, _p, _p, _p, _p, _i32, _f32, _p, _p, _i32,
                                      _i32, _f32, _f32, _i64, _p]),
    "natinf_step_f32prod_noise": (C.c_int, [_p, _p, _p, _f32, _i64, _i64, _p, _p, _p, _p, _p, _i32, _f32, _p, _p, _i32,
                                            _i32, _f32, _f32, C.c_uint64, _p, _i64, _i64, _i64, _p]),
    "natinf_step_f32prod_noise_guided": (C.c_int, [_p, _p, _p, _p, _p, _i32, _i64, _i64, _p, _p, _p, _p, _p, _i32, _f32, _p, _p, _i32,
                                                   _i32, _f32, _f32, C.c_uint64, _p, _i64, _i64, _i64, _p]),
    "natinf_step_f32prod_inpaint": (C.c_int, [_p, _p, _p, _p, _p, _i32, _i64, _i64, _p, _p, _p, _p, _p, _i32, _f32, _p, _p, _i32,
                                              _i32, _f32, _f32, C.c_uint64, _p, _i64, _i64, _i64,
                                              _p, _p, _i64, _i64, _f32, _f32, C.c_uint32, _p]),
    "natinf_weighted_sum_f32prod": (C.c_int, [_p, _p, _p, _p, _i32, _i64, _p]),
    "natinf_step_f16chain": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _i32, _f32, _f32, _i32, _f32, _f32, _f32,
                                       _f32, _i32, _i64, _p]),
    "natinf_step_f16chain_guided": (C.c_int, [_p, _p, _p, _p, _p, _i32, _i64, _p, _p, _p, _p, _p, _p, _i32, _f32, _f32, _i32, _f32, _f32,
                                              _f32, _i32, _i64, _p]),
    "natinf_known_blend_f16": (C.c_int, [_p, _p, _p, _p, _p, _i64, _i64, _f32, _f32, C.c_uint32, C.c_uint64, _p, _i64, _i64, _i64, _i64, _p]),
    "natinf_step_f16chain_inpaint": (C.c_int, [_p, _p, _p, _p, _p, _i32, _i64, _p, _p, _p, _p, _p, _p, _i32, _f32, _f32, _i32, _f32, _f32,
                                               _f32, _i32, _i64, _p, _p, _i64, _i64, C.c_uint32, C.c_uint64, _p, _i64, _i64, _p]),
    "natinf_weighted_mean_f16": (C.c_int, [_p, _p, _p, _p, _i32, _f32, _i64, _p]),
    "natinf_flow_input_f16": (C.c_int, [_p, _p, _p, _f32, _f32, _i64, _p]),
    # include/natinf_ncsnpp.h
    "natinf_ncsnpp_param_count": (C.c_int64, []),
    "natinf_ncsnpp_workspace_bytes": (C.c_int64, [_p, _i32]),
    "natinf_ncsnpp_packed_bytes": (C.c_int64, []),
    "natinf_ncsnpp_handle_param_count": (_i64, [_p]),
    "natinf_ncsnpp_handle_packed_bytes": (_i64, [_p]),
    "natinf_ncsnpp_create": (C.c_int, [C.POINTER(_p), _i32]),
    "natinf_ncsnpp_describe": (C.c_int, [_p, C.c_char_p, _i32]),
    "natinf_ncsnpp_destroy": (C.c_int, [_p]),
    "natinf_ncsnpp_load": (C.c_int, [_p, _p, _i64, _p, _i64, _p]),
    "natinf_ncsnpp_share": (C.c_int, [_p, _p]),
    "natinf_ncsnpp_forward": (C.c_int, [_p, _p, _p, _p, _i32, _p, _i64, _p]),
    "natinf_ncsnpp_debug_tap": (C.c_int, [_p, _i32, _p, _i64, _p]),
    "natinf_ncsnpp_describe_gemms": (C.c_int, [_p, _i32, C.c_char_p, _i32]),
    "natinf_debug_gemm": (C.c_int, [_i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _p, _p, _p, _p, _p, _i32, _f32, _i32, _p]),
    "natinf_set_gemm_variant": (C.c_int, [_i32]),
    "natinf_debug_timestamps": (C.c_int, [_p]),
    "natinf_set_gemm_epilogue": (C.c_int, [_i32]),
    "natinf_debug_gemm_fused": (C.c_int, [_i32, _i32, _i32, _i32, _p, _p, _p, _p, _p, _p, _i32, _p, _p, _f32, _i32, _p, _i32, _p, _p, _i32, _p]),
    "natinf_set_gemm_pref512": (C.c_int, [_i32]),
    "natinf_set_gemm_half_issue": (C.c_int, [_i32]),
    "natinf_set_gemm_raster": (C.c_int, [_i32]),
    "natinf_set_gemm_round_model": (C.c_int, [_i32]),
    "natinf_set_gemm_w128": (C.c_int, [_i32]),
    "natinf_set_fuse_gn": (C.c_int, [_i32]),
    "natinf_set_conv_gn_wide": (C.c_int, [_i32]),
    "natinf_set_attn_block": (C.c_int, [_i32]),
    "natinf_set_conv_gn_w128": (C.c_int, [_i32]),
    "natinf_set_conv_gn_w128_min_k": (C.c_int, [_i32, _i32]),
    "natinf_set_conv_gn_regw": (C.c_int, [_i32]),
    "natinf_set_fuse_up": (C.c_int, [_i32]),
    "natinf_set_fuse_up_fold": (C.c_int, [_i32]),
    "natinf_debug_fold_up_weights": (C.c_int, [_p, _i32, _i32, _f32, _p, _p, _p]),
    "natinf_debug_conv_up_fold": (C.c_int, [_i32, _i32, _i32, _p, _p, _p, _p, _p, _p, _p, _p, _f32, _p, _p, _i32, _p]),
    "natinf_set_fuse_head": (C.c_int, [_i32]),
    "natinf_set_fuse_gn8": (C.c_int, [_i32]),
    "natinf_set_fuse_gn4": (C.c_int, [_i32]),
    "natinf_set_fuse_fin": (C.c_int, [_i32]),
    "natinf_set_attn_proj": (C.c_int, [_i32]),
    "natinf_set_attn_waves8": (C.c_int, [_i32]),
    "natinf_set_attn_qkv": (C.c_int, [_i32]),
    "natinf_set_conv_gn_warm": (C.c_int, [_i32]),
    "natinf_set_attn256": (C.c_int, [_i32]),
    "natinf_set_conv_gn8_tile": (C.c_int, [_i32]),
    "natinf_set_gemm_splitk": (C.c_int, [_i32]),
    "natinf_debug_set_splitk_workspace": (C.c_int, [_p, _i32]),
    "natinf_debug_set_conv_operand": (C.c_int, [_i32, _p, _i32]),
    "natinf_debug_conv_gn": (C.c_int, [_i32, _i32, _i32, _i32, _i32, _p, _p, _p, _p, _p, _p, _p, _p, _f32, _p, _p, _i32, _p]),
    "natinf_debug_conv_gn_up": (C.c_int, [_i32]),
    "natinf_debug_conv_gn_fin": (C.c_int, [_p, _p, _p, _p, _i32, _f32]),
    "natinf_debug_attn_block": (C.c_int, [_i32, _i32, _p, _i32, _p, _p, _p, _p, _p, _p, _p, _i32, _f32, _p, _p]),
    "natinf_debug_gn_stats": (C.c_int, [_p, _i32, _i32, _i32, _i32, _p, _p, _p, _p, _f32, _f32, _p]),
    "natinf_debug_gn_finalize": (C.c_int, [_p, _i32, _i32, _p, _i32, _i32, _i32, _i32, _i32, _p, _p, _p, _p, _f32, _f32, _p]),
    "natinf_debug_gn_fold": (C.c_int, [_p, _i32, _i32, _i32, _i32, _p, _p]),
    "natinf_debug_gn_apply": (C.c_int, [_p, _i32, _i32, _i32, _i32, _i32, _p, _p, _p, _p, _i32, _i32, _i32, _p]),
    "natinf_debug_head_conv": (C.c_int, [_p, _i32, _i32, _p, _p, _p, _p, _p, _p]),
    "natinf_debug_time_embed": (C.c_int, [_p, _p, _i32, _p]),
    "natinf_debug_stem_im2col": (C.c_int, [_p, _p, _i32, _p]),
    "natinf_debug_pack_conv": (C.c_int, [_p, _p, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _f32, _p]),
    "natinf_debug_pack_transpose": (C.c_int, [_p, _p, _i32, _i32, _i32, _p]),
    "natinf_debug_nhwc_to_nchw": (C.c_int, [_p, _i32, _i32, _i32, _i32, _p, _p]),
    "natinf_ncsnpp_profile": (C.c_int, [_p, _i32]),
    "natinf_ncsnpp_profile_read": (C.c_int, [_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "natinf_debug_quant_fp8_rows": (C.c_int, [_p, _p, _p, _i32, _i32, _p]),
    "natinf_debug_gemm_fp8": (C.c_int, [_i32, _i32, _i32, _p, _p, _p, _p, _p, _p, _p, _p, _i32, _i32, _p]),
    # include/natinf_dit.h
    "natinf_dit_create": (C.c_int, [C.POINTER(_p), _i32, _i32, _i32, _i32]),
    "natinf_dit_create_sized": (C.c_int, [C.POINTER(_p), _i32, _i32, _i32, _i32, _i32]),
    "natinf_dit_input_size": (C.c_int, [_p]),
    "natinf_dit_attention_bf16": (C.c_int, [_p, _p, _p, _i32, _p, _i32, _i32, _i32, _i32, _i32, _i32, _p]),
    "natinf_dit_destroy": (C.c_int, [_p]),
    "natinf_dit_param_count": (C.c_int64, [_p]),
    "natinf_dit_packed_bytes": (C.c_int64, [_p]),
    "natinf_dit_workspace_bytes": (C.c_int64, [_p, _i32]),
    "natinf_dit_load": (C.c_int, [_p, _p, _i64, _p, _i64, _p]),
    "natinf_dit_forward": (C.c_int, [_p, _p, _p, _p, _p, _i32, _p, _i64, _p]),
    "natinf_dit_stream_sites": (C.c_int, [_p]),
    "natinf_dit_stream_status_reset": (C.c_int, [_p, _p, _p]),
    "natinf_dit_stream_status": (C.c_int, [_p, _p, _p, _p]),
    "natinf_debug_ln_modulate": (C.c_int, [_p, _i32, _p, _p, _i32, _p, _p, _p, _i32, _i64, _i32, C.POINTER(_i32), _p]),
    "natinf_debug_softmax_rows": (C.c_int, [_i32, _p, _p, _i32, _i64, _p]),
    "natinf_debug_patch_embed": (C.c_int, [_p, _p, _p, _p, _p, _p, _i32, _p, _i32, _i32, _i32, _i32, _p]),
    "natinf_debug_dit_time_freq": (C.c_int, [_p, _p, _i32, _p]),
    "natinf_debug_dit_cond": (C.c_int, [_p, _p, _p, _p, _i32, _i32, _p]),
    "natinf_debug_silu_bf16": (C.c_int, [_p, _p, _i64, _p]),
    "natinf_debug_f32_to_bf16": (C.c_int, [_p, _p, _i64, _p]),
    "natinf_debug_unpatchify": (C.c_int, [_p, _p, _i32, _i32, _i32, _p]),
    # include/natinf_mmdit.h
    "natinf_mmdit_create": (C.c_int, [C.POINTER(_p), _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32]),
    "natinf_mmdit_destroy": (C.c_int, [_p]),
    "natinf_mmdit_param_count": (C.c_int64, [_p]),
    "natinf_mmdit_packed_bytes": (C.c_int64, [_p]),
    "natinf_mmdit_workspace_bytes": (C.c_int64, [_p, _i32]),
    "natinf_mmdit_load": (C.c_int, [_p, _p, _i64, _p, _i64, _p]),
    "natinf_mmdit_forward": (C.c_int, [_p, _p, _p, _p, _p, _p, _i32, _p, _i64, _p]),
    "natinf_mmdit_stream_sites": (C.c_int, [_p]),
    "natinf_mmdit_stream_status_reset": (C.c_int, [_p, _p, _p]),
    "natinf_mmdit_stream_status": (C.c_int, [_p, _p, _p, _p]),
    "natinf_attention_hd64_bf16": (C.c_int, [_p, _p, _i32, _i64, _p, _p, _i32, _i64, _i32, _i32, _i32, _i32, C.c_float, _p]),
    "natinf_debug_attention_hd64_fp8out": (C.c_int, [_p, _p, _i32, _i64, _p, _p, _p, _i32, _i32, _i32, _i32, C.c_float, _p]),
    "natinf_inception_create": (C.c_int, [_p, _i32, _i32]),
    "natinf_inception_destroy": (C.c_int, [_p]),
    "natinf_set_inception_conv": (C.c_int, [_i32]),
    "natinf_debug_conv_ring": (C.c_int, [_i32] * 14 + [_p, _p, _p, _p, _p, _p, _i32, _p]),
    "natinf_debug_inc_stem": (C.c_int, [_p, _i32, _i32, _i32, _i32, _i32, _i32, _p, _p]),
    "natinf_debug_inc_pool": (C.c_int, [_i32] * 8 + [_p, _i32, _p, _i32, _p]),
    "natinf_debug_inc_global_avg": (C.c_int, [_i32, _i32, _i32, _i32, _p, _p, _p]),
    "natinf_debug_inc_pack": (C.c_int, [_i32, _p, _p, _p, _p, _p] + [_i32] * 7 + [_p, _p, _p, _p]),
    "natinf_debug_inc_im2col": (C.c_int, [_i32] * 11 + [_p, _p, _p]),
    "natinf_inception_param_count": (_i64, [_p]),
    "natinf_inception_packed_bytes": (_i64, [_p]),
    "natinf_inception_workspace_bytes": (_i64, [_p, _i32]),
    "natinf_inception_load": (C.c_int, [_p, _p, _i64, _p, _i64, _p]),
    "natinf_inception_forward": (C.c_int, [_p, _p, _i32, _p, _i32, _p, _i64, _p]),
    "natinf_gemm_profile": (C.c_int, [_i32]),
    "natinf_gemm_profile_read": (C.c_int, [_p, _i32]),
    "natinf_set_mmdit_stream16": (C.c_int, [_i32]),
    "natinf_set_dit_stream16": (C.c_int, [_i32]),
    "natinf_set_mmdit_text_flat": (C.c_int, [_i32]),
    "natinf_attention_profile": (C.c_int, [_i32]),
    "natinf_set_mmdit_text_stream": (C.c_int, [_i32]),
    "natinf_set_flash_mode": (C.c_int, [_i32]),
    "natinf_attention_profile_read": (C.c_int, [_p, _p]),
    # include/natinf_vae.h
    "natinf_vae_create": (C.c_int, [C.POINTER(_p), _i32, _i32]),
    "natinf_vae_destroy": (C.c_int, [_p]),
    "natinf_vae_param_count": (C.c_int64, [_p]),
    "natinf_vae_packed_bytes": (C.c_int64, [_p]),
    "natinf_vae_workspace_bytes": (C.c_int64, [_p, _i32]),
    "natinf_vae_load": (C.c_int, [_p, _p, _i64, _p, _i64, _p]),
    "natinf_vae_decode": (C.c_int, [_p, _p, _p, _i32, _p, _i64, _p]),
    "natinf_vae_enc_create": (C.c_int, [C.POINTER(_p), _i32, _i32]),
    "natinf_vae_enc_destroy": (C.c_int, [_p]),
    "natinf_vae_enc_param_count": (C.c_int64, [_p]),
    "natinf_vae_enc_packed_bytes": (C.c_int64, [_p]),
    "natinf_vae_enc_workspace_bytes": (C.c_int64, [_p, _i32]),
    "natinf_vae_enc_load": (C.c_int, [_p, _p, _i64, _p, _i64, _p]),
    "natinf_vae_posterior_f32": (C.c_int, [_p, _p, _i64, _i32, _i64, _i32, _f32, _f32, C.c_uint64, _p, _i64, _i64, _p]),
    "natinf_vae_encode": (C.c_int, [_p, _p, _p, _p, _i32, _i32, _f32, _f32, C.c_uint64, _p, _i64, _i64, _p, _i64, _p]),
    "natinf_debug_vae_latents": (C.c_int, [_p, _p, _p, _p, _i32, _i32, _i32, _p]),
    "natinf_debug_vae_images": (C.c_int, [_p, _p, _i32, _i32, _p]),
    "natinf_debug_vae_quant": (C.c_int, [_p, _p, _p, _p, _i32, _i32, _i32, _p]),
    # include/natinf_posterior.h
    "natinf_posterior_workspace_bytes": (C.c_int64, [_i32, _i32]),
    "natinf_posterior_samples": (C.c_int, [_p, _p, _f32, _f32, C.c_uint64, _p, _i64, _i64, _i32, _i32, _p, _p]),
    "natinf_posterior_stats": (C.c_int, [_p, _f64, _i32, _i32, _p, _p, _p, _p]),
    "natinf_posterior_debug_planes": (C.c_int, [_p, _i32, _i32, _p]),
    # include/natinf_prdc.h
    "natinf_prdc_workspace_bytes": (C.c_int64, [_i64, _i64, _i32, _i32]),
    "natinf_prdc_planes": (C.c_int, [_p, _i64, _i32, _p, _p, _p]),
    "natinf_prdc_knn_radius": (C.c_int, [_p, _p, _i64, _p, _p, _i64, _i32, _i32, _i64, _p, _p, _i64, _p]),
    "natinf_prdc_ball_counts": (C.c_int, [_p, _p, _i64, _p, _p, _i64, _i32, _i64, _p, _p, _p, _p, _p]),
    "natinf_prdc_debug_dist2": (C.c_int, [_p, _p, _i64, _p, _p, _i64, _i32, _i64, _p, _p]),
    # include/natinf_nn.h
    "natinf_nn_workspace_bytes": (C.c_int64, [_i64, _i64, _i32, _i32]),
    "natinf_nn_nearest": (C.c_int, [_p, _p, _i64, _p, _p, _i64, _i32, _i32, _i64, _p, _p, _p, _i64, _p]),
    # include/natinf_kid.h
    "natinf_kid_workspace_bytes": (C.c_int64, [_i64, _i64, _i32]),
    "natinf_kid_row_sums": (C.c_int, [_p, _i64, _i64, _p, _i64, _i64, _i32, _i64, _f64, _f64, _p, _p, _i64, _p]),
    # include/natinf_is.h
    "natinf_is_workspace_bytes": (C.c_int64, [_i64, _i32, _i32]),
    "natinf_is_row_stats": (C.c_int, [_p, _i64, _i64, _p, _i64, _i32, _i32, _p, _p, _p, _p, _p, _p, _i64, _p]),
    # include/natinf_ideal.h
    "natinf_ideal_tplanes": (C.c_int, [_p, _i64, _i32, _p, _p]),
    "natinf_ideal_workspace_bytes": (C.c_int64, [_i64, _i64, _i32]),
    "natinf_ideal_posterior_mean": (C.c_int, [_p, _p, _i64, _p, _p, _p, _i64, _i32, _i64, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i64, _p]),
    "natinf_ideal_debug_weights": (C.c_int, [_p, _p, _i64, _p, _p, _i64, _i32, _i64, _p, _p, _p, _i64, _p]),
    # include/natinf_fit.h
    "natinf_fit_gram_f64": (C.c_int, [_p, _i64, C.POINTER(C.c_int32), _i32, _p, _p, _i64, _i64, _p, _p]),
}

for _name, (_res, _args) in SIGNATURES.items():
    try:
        _fn = getattr(lib, _name)
    except AttributeError as e:                       # header and library out of sync
        raise ImportError(f"{LIB_PATH} does not export {_name}; rebuild it") from e
    _fn.restype, _fn.argtypes = _res, _args

X0_CLIP, X0_DYNAMIC = 1, 2                              # include/natinf.h: mode of natinf_x0_threshold_f64 / natinf_step_f64hist_x0fix
SD3_CFG_ON_VELOCITY = 1
SD3_BLEND_MEAN = 2                                      # natinf_step_f16chain_inpaint only
DIT_UNFUSED_ATTENTION = 1                               # include/natinf_dit.h: flags of natinf_dit_create / natinf_dit_create_sized
DIT_FP8 = 2
DIT_STREAM_GUARD = 16
MMDIT_FP8 = 1                                           # include/natinf_mmdit.h: flags of natinf_mmdit_create
MMDIT_STREAM_GUARD = 2


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise RuntimeError(f"{what} failed: {lib.natinf_strerror(rc).decode()} ({rc})")


def stream_ptr(stream=None) -> int:
    import torch
    s = stream if stream is not None else torch.cuda.current_stream()
    return int(s.cuda_stream)


def ptr(t) -> int:
    return 0 if t is None else int(t.data_ptr())


class StreamGuardStatus:
    """The stream-guard side of a transformer engine wrapper (include/natinf_dit.h, NATINF_DIT_STREAM_GUARD): ``_guard_api`` names the C entries' prefix
    (``natinf_dit`` / ``natinf_mmdit``); the wrapper sets ``guard``, ``_h`` and ``_ws``."""
    _guard_api = ""
    guard = False

    def _guard_entry(self, name):
        if not self.guard:
            raise RuntimeError("this engine was created without guard=True: it keeps no stream status")
        return getattr(lib, f"{self._guard_api}_{name}")

    @property
    def site_names(self):
        """One name per site, in the status block's order: ``patch_embed``, ``blocks.0.attn``, ``blocks.0.mlp``, ..."""
        n = self._guard_entry("stream_sites")(self._h)
        check(min(n, 0), f"{self._guard_api}_stream_sites")
        return ["patch_embed"] + [f"blocks.{i // 2}.{'mlp' if i % 2 else 'attn'}" for i in range(n - 1)]

    def reset_stream_status(self) -> None:
        """Zero the status block (enqueued on the current stream; nothing else ever zeroes it: it accumulates over forwards)."""
        import torch
        with torch.cuda.device(self._ws.device):
            check(self._guard_entry("stream_status_reset")(self._h, ptr(self._ws), stream_ptr()), f"{self._guard_api}_stream_status_reset")

    def stream_status(self):
        """{"max_abs": float32 [sites], "clamped": uint32 [sites]} (numpy) accumulated since the last reset: the largest |v| an update of the site produced, before
        rounding (NaN if one was NaN), and how many values left the half range and were written as +-65504 (or were NaN).  The one call here that waits for the GPU."""
        import torch
        n = len(self.site_names)
        buf = torch.empty(2 * n, dtype=torch.int32, device=self._ws.device)
        with torch.cuda.device(self._ws.device):
            check(self._guard_entry("stream_status")(self._h, ptr(self._ws), ptr(buf), stream_ptr()), f"{self._guard_api}_stream_status")
        raw = buf.cpu().numpy().view("uint32").reshape(n, 2)
        return {"max_abs": raw[:, 0].copy().view("float32"), "clamped": raw[:, 1].copy()}


def require_gpu() -> None:
    """Raise unless a gfx950 device is visible and the code object loads on it."""
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("naturaldiffusion_amd needs an MI355X (gfx950) GPU: torch.cuda.is_available() is False "
                           "and there is no CPU fallback")
    check(lib.natinf_probe(), "natinf_probe")
