"""ctypes binding of libmpformer_hip.so — the C-ABI boundary (include/mpformer_hip.h).

The library is built in-tree by ``__graft_entry__.build()`` / ``make -C mp_former_amd/csrc`` and is
loaded lazily on first use.  A missing library is a hard error: there is no fallback path.

How a host wrapper reaches it:
  ``call(name, device, *args)``  every entry point that returns a status: makes ``device`` current, runs it, raises on failure
  ``lib().mpf_*_bytes(...)``     size queries (and the other calls that return a value, not a status): they launch nothing
  ``stream_ptr(device)``         the stream argument, passed by the caller where the signature wants it
  ``scratch(...)``               workspace; ``ptr(t)`` for an optional tensor; ``DTYPE[t.dtype]`` for the MPF_* dtype code
"""
import ctypes

import torch
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmpformer_hip.so")
# development only: A/B a second build of the library in one process run (tools/ab_lib.sh)
LIB_PATH = os.environ.get("MPF_LIB_PATH", LIB_PATH)
ABI_VERSION = 1

MPF_F32, MPF_F64, MPF_BF16, MPF_U8, MPF_BITS = 0, 1, 2, 3, 4
# torch dtype -> MPF_* code (bool tensors are read as bytes)
DTYPE = {torch.float32: MPF_F32, torch.float64: MPF_F64, torch.bfloat16: MPF_BF16, torch.uint8: MPF_U8, torch.bool: MPF_U8}

_lib = None
_status_fns = {}  # name -> bound function, for the symbols that return a status (restype c_int): what `call` may run

_c_int = ctypes.c_int
_c_vp = ctypes.c_void_p

# name -> (restype, argtypes); every symbol declared in include/mpformer_hip.h
SIGNATURES = {
    "mpf_abi_version": (_c_int, []),
    "mpf_last_error": (ctypes.c_char_p, []),
    "mpf_last_kernel": (ctypes.c_char_p, []),
    "mpf_set_option": (_c_int, [ctypes.c_char_p, _c_int]),
    "mpf_match_cost_fused_workspace_bytes": (ctypes.c_size_t, [_c_int] * 5),
    "mpf_match_cost_fused": (_c_int, [_c_vp, _c_vp, ctypes.c_int64, _c_vp, ctypes.c_int64, _c_vp, _c_int, _c_int, _c_int, _c_vp, _c_vp, _c_int,
                                      _c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_int, _c_int, ctypes.c_float, ctypes.c_float, _c_vp,
                                      ctypes.c_size_t, _c_vp]),
    "mpf_match_cost_fused_clip_workspace_bytes": (ctypes.c_size_t, [_c_int] * 6),
    "mpf_match_cost_fused_clip": (_c_int, [_c_vp, _c_vp, ctypes.c_int64, _c_vp, ctypes.c_int64, ctypes.c_int64, _c_vp, _c_int, _c_int, _c_int,
                                           _c_vp, _c_vp, _c_int, _c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_int, _c_int, _c_int, ctypes.c_float,
                                           ctypes.c_float, _c_vp, ctypes.c_size_t, _c_vp]),
    "mpf_pair_planes_forward": (_c_int, [_c_vp] * 6 + [ctypes.c_int64, _c_vp, _c_int, _c_int, _c_int, _c_vp]),
    "mpf_pair_planes_backward_workspace_bytes": (ctypes.c_size_t, [_c_int] * 4),
    "mpf_pair_planes_backward": (_c_int, [_c_vp] * 7 + [ctypes.c_int64, _c_vp, ctypes.c_int64, _c_vp, _c_int, _c_int, _c_int, _c_int, _c_int,
                                          _c_int, _c_vp, ctypes.c_size_t, _c_vp]),
    "mpf_msda_dev_workspace_bytes": (ctypes.c_size_t, [_c_int] * 7),
    "mpf_msda_forward_dev": (_c_int, [_c_vp] * 6 + [_c_int] * 8 + [_c_vp, ctypes.c_size_t, _c_vp]),
    "mpf_msda_backward_dev": (_c_int, [_c_vp] * 9 + [_c_int] * 8 + [_c_vp, ctypes.c_size_t, _c_vp]),
    "mpf_msda_dev_geometry": (_c_int, [_c_vp, ctypes.POINTER(_c_int), _c_int]),
    "mpf_msda_stats": (_c_int, [ctypes.POINTER(ctypes.c_ulonglong), _c_int, _c_int]),
    "mpf_profile_enable": (_c_int, [_c_int]),
    "mpf_profile_get_flops": (_c_int, [ctypes.c_char_p, ctypes.POINTER(ctypes.c_double)]),
    "mpf_profile_get": (_c_int, [ctypes.c_char_p, ctypes.POINTER(_c_int), ctypes.POINTER(ctypes.c_double),
                                 ctypes.POINTER(ctypes.c_double)]),
    "mpf_point_sample": (_c_int, [_c_vp, _c_int, _c_int, _c_int, _c_vp, _c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_vp]),
    "mpf_mask_loss_forward": (_c_int, [_c_vp, _c_int, _c_int, _c_int, _c_vp, _c_vp, _c_int, _c_int, _c_int, _c_vp, _c_vp,
                                       _c_vp, _c_int, _c_int, _c_int, _c_vp]),
    "mpf_pack_mask_bits": (_c_int, [_c_vp, _c_vp, ctypes.c_int64, _c_vp]),
    "mpf_mask_loss_backward": (_c_int, [_c_vp, _c_int, _c_int, _c_int, _c_vp, _c_vp, _c_int, _c_int, _c_vp, _c_vp,
                                        _c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_vp]),
    "mpf_select_uncertain": (_c_int, [_c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_int, _c_int, _c_vp]),
    "mpf_sample_select_uncertain": (_c_int, [_c_vp, _c_int, _c_int, _c_int, _c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_int, _c_int, _c_vp]),
    "mpf_match_cost": (_c_int, [_c_vp, _c_int, _c_int, _c_int, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp,
                                _c_int, _c_int, _c_int, ctypes.c_float, ctypes.c_float, _c_int, _c_vp]),
    "mpf_match_cost_clip_workspace_bytes": (ctypes.c_size_t, [_c_int] * 3),
    "mpf_match_cost_clip": (_c_int, [_c_vp, _c_int, _c_int, _c_int, _c_vp, _c_int, ctypes.c_int64, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp,
                                     _c_int, _c_int, _c_int, ctypes.c_float, ctypes.c_float, _c_int, _c_vp, ctypes.c_size_t, _c_vp]),
    "mpf_attn_mask": (_c_int, [_c_vp, _c_int, ctypes.c_int64, ctypes.c_int64, _c_int, _c_int, _c_vp, _c_int, _c_vp,
                               _c_int, _c_int, _c_int, _c_int, _c_vp]),
    "mpf_attn_workspace_bytes": (ctypes.c_size_t, [_c_int] * 4),
    "mpf_attn_forward": (_c_int, [_c_vp, _c_vp, _c_vp, _c_vp, _c_int, _c_vp, _c_vp, _c_int, _c_int, _c_int, _c_int, _c_int,
                                  ctypes.c_float, _c_vp, ctypes.c_size_t, _c_vp]),
    "mpf_attn_backward": (_c_int, [_c_vp] * 8 + [_c_int] + [_c_vp] * 5 + [_c_int] * 6 + [ctypes.c_float, _c_vp, ctypes.c_size_t, _c_vp]),
    "mpf_attn_transpose2": (_c_int, [_c_vp] * 4 + [_c_int] * 4 + [_c_vp]),
    "mpf_attn_transpose2_strided": (_c_int, [_c_vp] * 2 + [ctypes.c_int64] * 2 + [_c_vp] * 2 + [_c_int] * 4 + [_c_vp]),
    "mpf_attn_forward_kv": (_c_int, [_c_vp, _c_vp, ctypes.c_int64, ctypes.c_int64, _c_vp, _c_vp, _c_int, _c_vp, _c_vp, _c_int, _c_int,
                                     _c_int, _c_int, _c_int, ctypes.c_float, _c_vp, ctypes.c_size_t, _c_vp]),
    "mpf_attn_backward_kv": (_c_int, [_c_vp] * 3 + [ctypes.c_int64] * 2 + [_c_vp] * 5 + [_c_int] + [_c_vp] * 5 + [ctypes.c_int64] * 2
                             + [_c_int] * 6 + [ctypes.c_float, _c_vp, ctypes.c_size_t, _c_vp]),
    "mpf_attn_backward_kv_aux": (_c_int, [_c_vp] * 3 + [ctypes.c_int64] * 2 + [_c_vp] * 5 + [_c_int] + [_c_vp] * 5 + [ctypes.c_int64] * 2
                                 + [_c_int] * 6 + [ctypes.c_float, _c_vp, ctypes.c_size_t, _c_vp, _c_vp]),
    "mpf_attn_bwd_aux_bytes": (ctypes.c_size_t, [_c_int] * 5),
    "mpf_attn_bwd_prep_aux": (_c_int, [_c_vp] * 5 + [_c_int] * 2 + [_c_vp] * 4 + [ctypes.c_size_t] + [_c_int] * 4 + [_c_vp]),
    "mpf_attn_delta": (_c_int, [_c_vp] * 3 + [_c_int] * 3 + [_c_vp]),
    "mpf_attn_bwd_prep": (_c_int, [_c_vp] * 6 + [_c_int] * 4 + [_c_vp]),
    "mpf_win_attn_workspace_bytes": (ctypes.c_size_t, [_c_int] * 5),
    "mpf_win_attn_forward": (_c_int, [_c_vp] * 3 + [_c_int] * 7 + [ctypes.c_float, _c_vp]),
    "mpf_win_attn_backward": (_c_int, [_c_vp] * 6 + [_c_int] * 7 + [ctypes.c_float, _c_vp, ctypes.c_size_t, _c_vp]),
    "mpf_gemm3_split": (_c_int, [_c_vp, _c_int, _c_int, _c_int, _c_vp, _c_vp]),
    "mpf_gemm3_tn": (_c_int, [_c_vp, ctypes.c_int64, _c_vp, _c_int, _c_vp, _c_vp, _c_vp, ctypes.c_int64, _c_vp, ctypes.c_int64,
                           _c_vp, ctypes.c_int64, _c_vp, ctypes.c_int64, _c_int, _c_int, _c_int, _c_int, _c_vp]),
    "mpf_gemm3_nt": (_c_int, [_c_vp, ctypes.c_int64, _c_vp, ctypes.c_int64, _c_vp, ctypes.c_int64, _c_int, _c_vp, _c_vp, _c_vp,
                           _c_int, _c_int, _c_int, _c_int, _c_int, _c_vp]),
    "mpf_amax_f32": (_c_int, [_c_vp, ctypes.c_int64, _c_vp, _c_vp]),
    "mpf_amax_f32_grouped": (_c_int, [_c_vp, _c_int, ctypes.c_int64, _c_vp]),
    "mpf_h2_range_stats": (_c_int, [_c_vp, _c_int, _c_int, ctypes.c_int64, _c_vp, _c_int, _c_vp, _c_vp]),
    "mpf_gemm3_split_grouped_h2": (_c_int, [_c_vp, _c_int, ctypes.c_int64, _c_vp]),
    "mpf_gemm3_tn_h2": (_c_int, [_c_vp, ctypes.c_int64, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, ctypes.c_int64, _c_vp, ctypes.c_int64,
                              _c_vp, ctypes.c_int64, _c_vp, ctypes.c_int64, _c_vp, _c_int, _c_int, _c_int, _c_int, _c_vp]),
    "mpf_gemm3_tn_h2_bits": (_c_int, [_c_vp, ctypes.c_int64, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, ctypes.c_int64, _c_vp, ctypes.c_int64,
                                   _c_vp, ctypes.c_int64, _c_vp, ctypes.c_int64, _c_vp, _c_vp, ctypes.c_int64,
                                   _c_int, _c_int, _c_int, _c_int, _c_vp]),
    "mpf_gemm3_nt_h2": (_c_int, [_c_vp, ctypes.c_int64, _c_vp, _c_vp, ctypes.c_int64, _c_vp, _c_vp, _c_vp, _c_vp,
                              _c_int, _c_int, _c_int, _c_int, _c_int, _c_vp]),
    "mpf_gemm3_nt_grouped_h2": (_c_int, [_c_vp, _c_int, _c_int, _c_int, ctypes.c_int64, _c_vp]),
    "mpf_gemm3_conv3x3_h2": (_c_int, [_c_vp] * 7 + [_c_int] * 6 + [_c_vp]),
    "mpf_gemm3_conv3x3_wgrad_h2": (_c_int, [_c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_vp]),
    "mpf_gemm3_nt_grouped": (_c_int, [_c_vp, _c_int, _c_int, _c_int, ctypes.c_int64, _c_vp]),
    "mpf_conv_wgrad_group_max": (_c_int, []),
    "mpf_conv_wgrad_plan": (_c_int, [_c_vp, _c_int, _c_int, _c_vp, ctypes.POINTER(ctypes.c_size_t)]),
    "mpf_conv_wgrad_bf16_grouped": (_c_int, [_c_vp, _c_int, _c_vp, ctypes.c_size_t, _c_vp]),
    "mpf_small_gemm_bf16": (_c_int, [_c_vp, ctypes.c_int64, ctypes.c_int64, _c_vp, _c_vp, ctypes.c_int64, ctypes.c_int64, _c_vp, _c_vp,
                                     ctypes.c_int64, _c_vp, ctypes.c_int64, _c_vp, _c_int, _c_int, _c_int, _c_int, _c_vp]),
    "mpf_encoder_fields": (_c_int, []),
    "mpf_encoder_forward": (_c_int, [_c_vp, _c_vp]),
    "mpf_encoder_bwd_fields": (_c_int, []),
    "mpf_encoder_backward": (_c_int, [_c_vp, _c_vp]),
    "mpf_decoder_layer_struct_bytes": (ctypes.c_uint64, [_c_int]),
    "mpf_decoder_layer_scratch_bytes": (ctypes.c_uint64, [_c_int] * 6),
    "mpf_decoder_layer_forward": (_c_int, [_c_vp, _c_vp]),
    "mpf_next_attn_mask_scratch_bytes": (ctypes.c_size_t, [_c_int, _c_int]),
    "mpf_next_attn_mask": (_c_int, [_c_vp, _c_vp]),
    "mpf_lin256_res_ln_forward": (_c_int, [_c_vp] * 11 + [_c_int, ctypes.c_float, _c_vp]),
    "mpf_ln256_mlp3_forward": (_c_int, [_c_vp] * 10 + [_c_int, ctypes.c_float, _c_vp]),
    "mpf_decoder_layer_backward": (_c_int, [_c_vp, _c_vp, _c_vp]),
    "mpf_qpos_operand_forward": (_c_int, [_c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_vp]),
    "mpf_qpos_backward": (_c_int, [_c_vp, _c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_vp]),
    "mpf_decoder_layer_pos_struct_bytes": (ctypes.c_uint64, []),
    "mpf_decoder_layer_pos_scratch_bytes": (ctypes.c_uint64, [_c_int] * 6),
    "mpf_decoder_layer_pos_forward": (_c_int, [_c_vp, _c_vp, _c_vp]),
    "mpf_decoder_layer_pos_backward": (_c_int, [_c_vp, _c_vp, _c_vp, _c_vp]),
    "mpf_pool_features": (_c_int, [_c_vp, _c_int, _c_vp] + [_c_int] * 6 + [_c_vp]),
    "mpf_pool_features_cl": (_c_int, [_c_vp, ctypes.c_int64, _c_int, _c_vp, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_vp]),
    "mpf_mask_head_bits": (_c_int, [_c_vp, ctypes.c_int64, ctypes.c_int64, _c_vp, _c_vp, _c_int, _c_vp, _c_vp] + [_c_int] * 3 + [_c_vp]),
    "mpf_lsa_assign": (_c_int, [_c_vp, _c_vp, _c_int, _c_int, ctypes.c_int64] + [_c_vp] * 7),
    "mpf_lsa_assign_status": (_c_int, [_c_vp, _c_vp, _c_int, _c_int, ctypes.c_int64] + [_c_vp] * 8),
    "mpf_mask_block_empty": (_c_int, [_c_vp, _c_vp] + [_c_int] * 5 + [_c_vp]),
    "mpf_mp_open_counts": (_c_int, [_c_vp, _c_int, _c_int, _c_vp, _c_vp]),
    "mpf_mp_noise_rows": (_c_int, [_c_vp] * 3 + [_c_int] * 4 + [ctypes.c_double, ctypes.c_uint64, ctypes.c_uint64, _c_vp, _c_vp]),
    "mpf_gemm_nt_bf16_workspace_bytes": (ctypes.c_size_t, [_c_int] * 4),
    "mpf_gemm_nt_bf16": (_c_int, [_c_vp, ctypes.c_int64, _c_vp, ctypes.c_int64, _c_vp, _c_vp, _c_int, _c_int, _c_int, _c_int, _c_vp,
                                  ctypes.c_size_t, _c_vp]),
    "mpf_gemm3_nt_reduce": (_c_int, [_c_vp, ctypes.c_int64, _c_vp, ctypes.c_int64, _c_int, _c_vp, _c_vp, _c_vp]),
    "mpf_grouped_scale_cast": (_c_int, [_c_vp, _c_int, ctypes.c_int64, _c_int, _c_int, _c_vp]),
    "mpf_gemm3_split_grouped": (_c_int, [_c_vp, _c_int, ctypes.c_int64, _c_vp]),
    "mpf_decoder_inputs_forward": (_c_int, [_c_vp, ctypes.c_int64, ctypes.c_int64, _c_vp, _c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_int, _c_int,
                                            _c_vp]),
    "mpf_decoder_inputs_backward": (_c_int, [_c_vp, _c_vp, _c_int, _c_vp, ctypes.c_int64, ctypes.c_int64, _c_int, _c_int, _c_int, _c_vp]),
    "mpf_clip_inputs_forward": (_c_int, [_c_vp, ctypes.c_int64, ctypes.c_int64, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_int, _c_int,
                                         _c_int, _c_vp]),
    "mpf_clip_inputs_backward": (_c_int, [_c_vp, _c_vp, _c_int, _c_vp, ctypes.c_int64, ctypes.c_int64, _c_int, _c_int, _c_int, _c_int, _c_vp]),
    "mpf_clip_adamw_step": (_c_int, [_c_vp, _c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                     _c_vp, _c_vp, _c_vp]),
    "mpf_transpose_f32": (_c_int, [_c_vp, ctypes.c_int64, _c_vp, ctypes.c_int64, _c_int, _c_int, _c_int, _c_vp]),
    "mpf_small_gemm_bf16_blocked": (_c_int, [_c_vp, ctypes.c_int64, ctypes.c_int64, _c_int, ctypes.c_int64, _c_vp, _c_vp, ctypes.c_int64,
                                             ctypes.c_int64, _c_vp, _c_vp, ctypes.c_int64, _c_vp, ctypes.c_int64, _c_int, ctypes.c_int64,
                                             _c_vp, _c_int, _c_int, _c_int, _c_int, _c_vp]),
    "mpf_small_gemm_bf16_group": (_c_int, [_c_vp, _c_int, _c_vp]),
    "mpf_transpose_group_bf16": (_c_int, [_c_vp, _c_int, _c_int, _c_vp]),
    "mpf_class_loss_forward": (_c_int, [_c_vp, _c_int, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, _c_vp, _c_int, _c_vp, _c_int, _c_int,
                                        _c_int, _c_int, _c_vp, _c_vp, _c_vp, _c_vp]),
    "mpf_class_loss_backward": (_c_int, [_c_vp, _c_int, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, _c_vp, _c_int, _c_vp, _c_int, _c_int,
                                         _c_int, _c_int, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp]),
    "mpf_mask_loss_finalize": (_c_int, [_c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_int, _c_vp, _c_vp]),
    "mpf_mask_loss_finalize_backward": (_c_int, [_c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_int, _c_vp, _c_vp, _c_vp]),
    "mpf_bias_act": (_c_int, [_c_vp, _c_vp, _c_vp, _c_vp, ctypes.c_int64, _c_int, _c_int, _c_int, _c_vp]),
    "mpf_relu_bwd_add": (_c_int, [_c_vp, _c_vp, _c_vp, _c_vp, ctypes.c_int64, _c_int, _c_vp]),
    "mpf_maxpool3x3s2_forward": (_c_int, [_c_vp] * 3 + [_c_int] * 4 + [_c_vp]),
    "mpf_maxpool3x3s2_backward": (_c_int, [_c_vp] * 3 + [_c_int] * 4 + [_c_vp]),
    "mpf_upload_small": (_c_int, [_c_vp, _c_vp, ctypes.c_int64, _c_vp]),
    "mpf_tall_gemm_bf16": (_c_int, [_c_vp, ctypes.c_int64, _c_vp, ctypes.c_int64, _c_vp, _c_vp, ctypes.c_int64, _c_int, _c_int, _c_int, _c_vp]),
    "mpf_res_ln256_forward": (_c_int, [_c_vp, _c_vp, _c_int, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_int, ctypes.c_float,
                                       _c_vp, _c_int, _c_vp, _c_vp]),
    "mpf_res_ln256_forward_b": (_c_int, [_c_vp, _c_vp, _c_int, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_int, ctypes.c_float,
                                         _c_vp, _c_int, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp]),
    "mpf_res_ln256_backward_ws_amax": (_c_int, [_c_vp] * 11 + [_c_int, _c_vp, ctypes.c_size_t, _c_vp, _c_vp]),
    "mpf_res_ln256_backward": (_c_int, [_c_vp] * 11 + [_c_int, _c_vp]),
    "mpf_mask_loss_backward_dense": (_c_int, [_c_vp, _c_int, _c_int, _c_int, _c_vp, _c_vp, _c_int, _c_int, _c_int, _c_vp, _c_vp, _c_vp,
                                              _c_vp, _c_int, _c_vp, _c_int, _c_int, _c_vp]),
    "mpf_gn_cl_supported": (_c_int, [_c_int, _c_int, _c_int]),
    "mpf_gn_cl_workspace_bytes": (ctypes.c_size_t, [_c_int, _c_int, _c_int, _c_int]),
    "mpf_gn_cl_forward": (_c_int, [_c_vp, ctypes.c_int64, _c_vp, _c_vp, _c_int, _c_int, _c_int, _c_int, ctypes.c_float, _c_int,
                                   _c_vp, ctypes.c_int64, _c_int, _c_vp, ctypes.c_int64, _c_vp, _c_vp, _c_vp, ctypes.c_size_t, _c_vp]),
    "mpf_gn_cl_backward": (_c_int, [_c_vp, ctypes.c_int64, _c_vp, ctypes.c_int64, _c_vp, _c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_int,
                                    _c_int, _c_int, _c_vp, ctypes.c_int64, _c_vp, _c_vp, _c_vp, ctypes.c_size_t, _c_vp]),
    "mpf_upsample2x_cl_backward": (_c_int, [_c_vp, ctypes.c_int64, _c_int, _c_int, _c_int, _c_int, _c_vp, ctypes.c_int64, _c_vp]),
    "mpf_gemm3_conv3x3": (_c_int, [_c_vp, _c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_vp]),
    "mpf_gemm3_conv3x3_wgrad": (_c_int, [_c_vp, _c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_vp]),
    "mpf_gemm3_nt_reduce_levels": (_c_int, [_c_vp, ctypes.c_int64, _c_vp, ctypes.c_int64, _c_int, _c_vp, _c_int, _c_vp, _c_vp, _c_vp, _c_vp]),
    "mpf_gemm3_tn_ex": (_c_int, [_c_vp, _c_int, ctypes.c_int64, _c_vp, _c_vp, _c_vp, ctypes.c_int64, _c_vp, _c_int, ctypes.c_int64,
                                 _c_int, _c_int, _c_int, _c_int, _c_vp]),
    "mpf_gemm3_nt_ex": (_c_int, [_c_vp, _c_int, ctypes.c_int64, _c_vp, _c_int, ctypes.c_int64, _c_vp, _c_vp, _c_int, _c_int, _c_int, _c_int, _c_vp]),
    "mpf_res_ln256_backward_workspace_bytes": (ctypes.c_size_t, [_c_int]),
    "mpf_res_ln256_backward_partial": (_c_int, [_c_vp] * 9 + [_c_int, _c_vp, ctypes.c_size_t, _c_vp]),
    "mpf_res_ln256_backward_partial_amax": (_c_int, [_c_vp] * 9 + [_c_int, _c_vp, ctypes.c_size_t, _c_vp, _c_vp]),
    "mpf_ln_partial_reduce": (_c_int, [_c_vp, ctypes.c_size_t, _c_int, _c_int, _c_vp, _c_vp]),
    "mpf_res_ln256_backward_det_workspace_bytes": (ctypes.c_size_t, [_c_int]),
    "mpf_res_ln256_backward_det": (_c_int, [_c_vp] * 10 + [_c_int, _c_vp, ctypes.c_size_t, _c_vp]),
    "mpf_res_ln256_backward_ws": (_c_int, [_c_vp] * 11 + [_c_int, _c_vp, ctypes.c_size_t, _c_vp]),
    "mpf_group_stats_workspace_bytes": (ctypes.c_size_t, [_c_int, ctypes.c_int64]),
    "mpf_group_stats": (_c_int, [_c_vp, _c_int, ctypes.c_int64, ctypes.c_float, _c_vp, _c_vp, _c_vp, ctypes.c_size_t, _c_vp]),
    "mpf_msda_forward": (_c_int, [_c_vp] * 6 + [_c_int] * 8 + [_c_vp]),
    "mpf_msda_backward": (_c_int, [_c_vp] * 9 + [_c_int] * 8 + [_c_vp]),
    "mpf_msda_forward_hs": (_c_int, [_c_vp] * 7 + [_c_int] * 8 + [_c_vp]),
    "mpf_msda_forward_raw_hs": (_c_int, [_c_vp] * 9 + [_c_int] * 8 + [_c_vp]),
    "mpf_msda_forward_raw": (_c_int, [_c_vp] * 8 + [_c_int] * 8 + [_c_vp]),
    "mpf_msda_backward_ws_raw": (_c_int, [_c_vp] * 7 + [_c_int] * 8 + [_c_vp, ctypes.c_size_t, _c_vp]),
    "mpf_msda_backward_ws_raw_o": (_c_int, [_c_vp] * 8 + [_c_int] * 8 + [_c_vp, ctypes.c_size_t, _c_vp, _c_vp, _c_vp]),
    "mpf_msda_backward_workspace_bytes": (ctypes.c_size_t, [_c_int] * 5 + [_c_vp]),
    "mpf_msda_backward_ws": (_c_int, [_c_vp] * 8 + [_c_int] * 8 + [_c_vp, ctypes.c_size_t, _c_vp]),
    "mpf_seg_softmax": (_c_int, [_c_vp, _c_int, _c_int, ctypes.c_float] + [_c_vp] * 6),
    "mpf_seg_semantic": (_c_int, [_c_vp, ctypes.c_int64] + [_c_int] * 10 + [_c_vp, _c_int, _c_vp, _c_vp]),
    "mpf_seg_instance_workspace_bytes": (ctypes.c_size_t, [_c_int] * 3),
    "mpf_seg_instance_scores": (_c_int, [_c_vp, ctypes.c_int64] + [_c_int] * 10 + [_c_vp, _c_vp, _c_int, _c_vp, _c_vp, ctypes.c_size_t,
                                                                                   _c_vp]),
    "mpf_seg_instance_masks": (_c_int, [_c_vp, ctypes.c_int64] + [_c_int] * 10 + [_c_vp, _c_int, _c_vp, _c_vp]),
    "mpf_seg_panoptic_areas": (_c_int, [_c_vp, ctypes.c_int64] + [_c_int] * 10 + [_c_vp] * 5),
    "mpf_seg_panoptic_paint": (_c_int, [_c_vp, _c_int, _c_int, _c_vp, _c_vp, _c_vp]),
    "mpf_seg_semantic_labels": (_c_int, [_c_vp, ctypes.c_int64] + [_c_int] * 10 + [_c_vp, _c_int, _c_vp, _c_vp]),
    "mpf_seg_labels_resize": (_c_int, [_c_vp] + [_c_int] * 5 + [_c_vp, _c_vp]),
    "mpf_seg_confusion_add": (_c_int, [_c_vp, _c_vp, ctypes.c_int64, _c_int, _c_int, _c_vp, _c_vp]),
    "mpf_seg_instance_rle_workspace_bytes": (ctypes.c_size_t, [_c_int] * 3),
    "mpf_seg_instance_rle_count": (_c_int, [_c_vp, ctypes.c_int64] + [_c_int] * 10 + [_c_vp, _c_int, _c_vp, _c_vp, ctypes.c_size_t, _c_vp]),
    "mpf_seg_instance_rle_write": (_c_int, [_c_vp, ctypes.c_size_t, _c_int, _c_int, _c_int, _c_vp, ctypes.c_int64, _c_vp, _c_vp, _c_vp]),
    "mpf_seg_tta_accumulate": (_c_int, [_c_vp, ctypes.c_int64] + [_c_int] * 10 + [_c_vp, _c_int, _c_int, _c_vp, _c_vp]),
    "mpf_seg_tta_resize_add": (_c_int, [_c_vp] + [_c_int] * 6 + [_c_vp, _c_vp]),
    "mpf_seg_tta_finish": (_c_int, [_c_vp] + [_c_int] * 4 + [_c_vp, _c_vp]),
    "mpf_seg_pq_workspace_bytes": (ctypes.c_size_t, [_c_int] * 2),
    "mpf_seg_pq_pairs": (_c_int, [_c_vp, _c_vp, _c_int, ctypes.c_int64, _c_vp, _c_int, _c_int, _c_vp, _c_int, _c_int, _c_int, _c_vp,
                                  ctypes.c_size_t, _c_vp]),
    "mpf_seg_pq_match": (_c_int, [_c_vp, ctypes.c_size_t, _c_int, _c_int, _c_int, _c_vp, _c_vp, _c_vp, _c_int] + [_c_vp] * 6),
    "mpf_seg_instance_bits": (_c_int, [_c_vp, ctypes.c_int64] + [_c_int] * 10 + [_c_vp, _c_int, _c_vp, _c_vp]),
    "mpf_seg_pack_masks": (_c_int, [_c_vp, _c_int, _c_int, _c_int, _c_int, _c_vp, _c_vp]),
    "mpf_seg_mask_pairs": (_c_int, [_c_vp, _c_int, _c_vp, _c_int, ctypes.c_int64, _c_vp, _c_vp, _c_vp, _c_vp]),
    "mpf_seg_ap_workspace_bytes": (ctypes.c_size_t, [_c_int] * 3),
    "mpf_seg_ap_match": (_c_int, [_c_vp, _c_vp, _c_vp, _c_int, _c_int] + [_c_vp] * 6 + [_c_int, _c_vp] + [_c_int] * 5
                         + [_c_vp, _c_vp, _c_vp, ctypes.c_size_t, _c_vp]),
    "mpf_seg_mask_boundary": (_c_int, [_c_vp, _c_int, _c_int, _c_int, _c_int, _c_vp, _c_vp]),
    "mpf_seg_ap_match_boundary": (_c_int, [_c_vp] * 6 + [_c_int, _c_int] + [_c_vp] * 6 + [_c_int, _c_vp] + [_c_int] * 5
                                  + [_c_vp, _c_vp, _c_vp, ctypes.c_size_t, _c_vp]),
    "mpf_seg_bits_boxes": (_c_int, [_c_vp, _c_int, _c_int, _c_int, _c_vp, _c_vp]),
    "mpf_seg_ap_match_box": (_c_int, [_c_vp, _c_vp, _c_int, _c_int] + [_c_vp] * 6 + [_c_int, _c_vp] + [_c_int] * 5
                             + [_c_vp, _c_vp, _c_vp, ctypes.c_size_t, _c_vp]),
    "mpf_seg_video_bits": (_c_int, [_c_vp, ctypes.c_int64, ctypes.c_int64] + [_c_int] * 11 + [_c_vp, _c_int, _c_vp, _c_vp, _c_vp, _c_vp]),
    "mpf_seg_tube_areas": (_c_int, [_c_vp, _c_int, _c_int, _c_vp, _c_vp]),
    "mpf_seg_ap_match_tube": (_c_int, [_c_vp, _c_vp, _c_vp, _c_int, _c_int] + [_c_vp] * 7 + [_c_int, _c_vp] + [_c_int] * 5
                              + [_c_vp, _c_vp, _c_vp, ctypes.c_size_t, _c_vp]),
    "mpf_seg_bits_rle_workspace_bytes": (ctypes.c_size_t, [_c_int] * 3),
    "mpf_seg_bits_rle_count": (_c_int, [_c_vp, _c_int, _c_int, _c_int, _c_vp, _c_vp, ctypes.c_size_t, _c_vp]),
    "mpf_seg_bits_rle_write": (_c_int, [_c_vp, _c_vp, ctypes.c_size_t, _c_int, _c_int, _c_int, _c_vp, ctypes.c_int64, _c_vp, _c_vp, _c_vp]),
    "mpf_seg_poly_stage_edges": (_c_int, []),
    "mpf_seg_poly_toggles": (_c_int, [_c_vp, _c_vp, _c_int, _c_int, _c_int, _c_vp, _c_vp]),
    "mpf_seg_rle_toggles": (_c_int, [_c_vp, _c_vp, _c_int, _c_int, _c_int, _c_vp, _c_vp]),
    "mpf_seg_toggles_fill": (_c_int, [_c_vp, _c_vp, _c_int, _c_int, _c_int, _c_int, _c_vp, _c_vp]),
    "mpf_seg_unpack_masks": (_c_int, [_c_vp, _c_int, _c_int, _c_int, _c_vp, _c_vp]),
    "mpf_img_resample_ksize": (_c_int, [_c_int, _c_int]),
    "mpf_img_resample_tables": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_vp, _c_vp]),
    "mpf_img_resample_span_rows": (_c_int, []),
    "mpf_img_resample_max_ratio": (_c_int, []),
    "mpf_img_resample": (_c_int, [_c_vp, _c_vp, _c_vp, _c_vp, ctypes.c_int64, _c_int, _c_vp, _c_int, _c_int, _c_int, _c_int,
                                  ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float), _c_vp]),
    "mpf_label_counts_max_classes": (_c_int, []),
    "mpf_label_counts_max_tries": (_c_int, []),
    "mpf_label_bits_max_ids": (_c_int, []),
    "mpf_label_resample": (_c_int, [_c_vp, _c_vp, _c_vp, _c_vp, ctypes.c_int64, _c_int, _c_vp, _c_int, _c_int, _c_int, _c_vp]),
    "mpf_label_window_counts": (_c_int, [_c_vp, _c_vp, _c_vp, _c_vp, ctypes.c_int64, _c_vp, _c_vp, _c_int, _c_int, _c_int, _c_int, _c_vp,
                                         _c_vp]),
    "mpf_label_bits": (_c_int, [_c_vp, ctypes.c_int64, _c_int, _c_int, _c_vp, _c_int, _c_vp, _c_vp, _c_vp]),
    "mpf_mask_bits_resample": (_c_int, [_c_vp, _c_vp, _c_vp, _c_vp, ctypes.c_int64, _c_int, _c_vp, _c_vp, _c_int, _c_int, _c_vp]),
}


class NativeLibraryError(RuntimeError):
    pass


def lib():
    """The loaded library (raises NativeLibraryError if it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NativeLibraryError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C mp_former_amd/csrc`.  mp_former_amd has no CPU / eager fallback.")
        l = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            try:
                fn = getattr(l, name)
            except AttributeError as e:
                raise NativeLibraryError(f"{LIB_PATH} does not export {name}") from e
            fn.restype = res
            fn.argtypes = args
            if res is _c_int:
                _status_fns[name] = fn
        v = l.mpf_abi_version()
        if v != ABI_VERSION:
            raise NativeLibraryError(f"ABI mismatch: library {v}, binding {ABI_VERSION}")
        _lib = l
        # MPF_OPTIONS="key=value,key=value": mpf_set_option at load (A/B runs of a kernel switch without code changes)
        for kv in filter(None, os.environ.get("MPF_OPTIONS", "").split(",")):
            k, _, v = kv.partition("=")
            set_option(k.strip(), int(v))
    return _lib


def check(code, what):
    if code != 0:
        msg = lib().mpf_last_error().decode()
        raise RuntimeError(f"{what} failed with code {code}: {msg}")


def _status_fn(name):
    lib()
    fn = _status_fns.get(name)
    if fn is None:
        raise TypeError(f"{name} does not return a status: call() is for the int-returning entry points, sizes go through lib()")
    return fn


def call(name, device, *args):
    """Run the int-returning entry point `name` with `device` current; raise RuntimeError naming `name` with mpf_last_error() if
    it fails.  The stream is an argument like any other (it is not last in every signature): pass ``stream_ptr(device)``."""
    fn = _status_fns.get(name) or _status_fn(name)
    idx = device.index
    if idx is None or idx == torch.cuda.current_device():  # as device_guard
        code = fn(*args)
    else:
        with torch.cuda.device(device):
            code = fn(*args)
    if code != 0:
        check(code, name)  # mpf_last_error is thread-local: read here, on the calling thread


def ptr(t):
    """data_ptr of an optional tensor (None -> NULL)"""
    return None if t is None else t.data_ptr()


_option_gen = 0


def option_generation():
    """advanced by every set_option: caches of option-dependent sizes (workspace bytes) key on it"""
    return _option_gen


def set_option(key, value):
    global _option_gen
    check(lib().mpf_set_option(key.encode(), int(value)), f"mpf_set_option({key})")
    _option_gen += 1


def msda_stats(reset=True):
    """Route counters of the blocked MSDA kernels (tests; enable with set_option("msda_stats", 1)) -> dict."""
    out = (ctypes.c_ulonglong * 9)()
    check(lib().mpf_msda_stats(out, 9, 1 if reset else 0), "mpf_msda_stats")
    keys = ("fwd_lds", "fwd_gather", "push_lds", "push_gather", "push_direct", "push_hash", "spill_entries", "pull_split", "pull_single")
    return dict(zip(keys, (int(v) for v in out)))


def last_kernel():
    return lib().mpf_last_kernel().decode()


def profile_enable(on=True):
    check(lib().mpf_profile_enable(1 if on else 0), "mpf_profile_enable")


def profile_get_flops(name_substr):
    """-> summed algorithmic flops of the logged launches matching the name."""
    fl = ctypes.c_double(0)
    check(lib().mpf_profile_get_flops(name_substr.encode(), ctypes.byref(fl)), "mpf_profile_get_flops")
    return fl.value


def profile_get(name_substr):
    """-> (launch count, total ms, total algorithmic bytes) of the logged launches matching the name."""
    n, ms, by = _c_int(0), ctypes.c_double(0), ctypes.c_double(0)
    check(lib().mpf_profile_get(name_substr.encode(), ctypes.byref(n), ctypes.byref(ms), ctypes.byref(by)),
          "mpf_profile_get")
    return n.value, ms.value, by.value


# ---- native scratch ---------------------------------------------------------------------------------------------------------
_scratch = {}


def scratch(owner, device, stream, nbytes, zeroed=False):
    """Grow-on-demand device scratch of the native ops -> uint8 tensor of at least ``nbytes`` (pass its ``numel()`` on).

    One buffer per (owner, device, stream).  ``owner`` is a literal naming ONE buffer layout: a layout may keep state between
    calls (the MSDA geometry record, the res-LN ticket, the mask-head flags) that another layout would overwrite.  ``stream`` is
    the raw stream of the native call (`stream_ptr`): ops running at once on two streams never share scratch.  ``zeroed``: a new
    or grown buffer starts zero, for layouts whose kernels leave it zero between calls (ticket, flags) or that must not find a
    stale geometry key in fresh memory.  A buffer whose address a HIP graph has baked in must never be resized: if graph capture
    returns, put the capture in the key here."""
    key = (owner, device, stream)
    w = _scratch.get(key)
    if w is None or w.numel() < nbytes:
        n = int(nbytes * 1.25) + 1024
        w = _scratch[key] = (torch.zeros if zeroed else torch.empty)(n, dtype=torch.uint8, device=device)
    return w


def stream_ptr(device):
    """Raw hipStream_t (as an int) of torch's current stream on ``device``.  ``torch.cuda.current_stream(device).cuda_stream`` builds
    a Stream object through two python-level device-index normalisations (~4.5 us; ~500 calls per training step)."""
    idx = device.index
    return torch._C._cuda_getCurrentRawStream(torch.cuda.current_device() if idx is None else idx)


class _NullGuard:
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


_NULL_GUARD = _NullGuard()


def device_guard(device):
    """``with torch.cuda.device(device)`` only when ``device`` is not the current one (the common single-device-per-process case
    costs one C call instead of a context manager with two index normalisations)."""
    idx = device.index
    if idx is None or idx == torch.cuda.current_device():
        return _NULL_GUARD
    return torch.cuda.device(device)
