"""ctypes binding of libsed_hip.so (include/sed_hip.h).  There is NO fallback: if the shared library
is missing or a call fails, a RuntimeError is raised -- the product path never computes on the CPU."""
from __future__ import annotations

import ctypes as C
import os

SED_F32, SED_BF16, SED_F32X3, SED_F32H3 = 0, 1, 2, 3
SED_ACT_RELU, SED_ACT_GELU = 0, 1
FFN_ACT = {"relu": SED_ACT_RELU, "gelu": SED_ACT_GELU}      # sed_ffn_fwd / sed_ffn_act_bwd
PRO_NONE, PRO_BNRELU = 0, 1
EPI_STORE, EPI_STATS, EPI_RELUBWD, EPI_POOLSTATS = 0, 1, 2, 4
DZ_POOL, DZ_BN = 1, 2
PCM_I16, PCM_I32, PCM_F32 = 0, 1, 2
POOL_MAX, POOL_MEAN, POOL_LINEAR, POOL_EXP = 0, 1, 2, 3
POOL_MODES = {"max": POOL_MAX, "mean": POOL_MEAN, "linear": POOL_LINEAR, "exp": POOL_EXP}
CRIT_BCE, CRIT_MSE = 0, 1
OPT_TILE4, OPT_MAX_GROUPS = 1024, 64     # SED_OPT_TILE4 / SED_OPT_MAX_GROUPS: the grouped optimizer step's tile size and group limit
SCHED_KINDS = {"const": 0, "step": 1, "cosine": 2, "linear": 3, "invsqrt": 4}       # SED_SCHED_*
WIN_UNBOUNDED = 0x7FFFFFFF          # SED_WIN_UNBOUNDED: a side of sed_mhsa_fwd_win / _bwd_win that reaches the clip's end

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsed_hip.so")

_P, _I, _Z, _F, _D = C.c_void_p, C.c_int, C.c_size_t, C.c_float, C.c_double
_U32 = C.c_uint32



class GemmTnDesc(C.Structure):
    """struct sed_gemm_tn_desc (include/sed_hip.h): one problem of sed_gemm_tn_batch"""
    _fields_ = [("A", _P), ("B", _P), ("C", _P), ("colsum", _P), ("workspace", _P), ("lda", _I), ("ldb", _I), ("ldc", _I), ("M", _I),
                ("N", _I), ("K", _I), ("seq", _I), ("shift", _I), ("ksplit", _I)]


# name -> (restype, argtypes); mirrors include/sed_hip.h one to one
PROTOTYPES = {
    "sed_abi_version": (_I, []),
    "sed_last_error": (C.c_char_p, []),
    "sed_build_flags": (_I, []),
    "sed_device_cu_count": (_I, []),
    "sed_config_reload": (None, []),
    "sed_pack_conv_weight": (_I, [_I, _P, _P, _I, _I, _I, _I, _I, _P]),
    "sed_unpack_conv_wgrad": (_I, [_P, _P, _I, _I, _I, _I, _P]),
    "sed_conv_c1_nparts": (_I, [_I, _I, _I]),
    "sed_conv3x3_c1_fwd": (_I, [_I, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "sed_conv3x3_c1_wgrad": (_I, [_I, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "sed_conv3x3_c1_wgrad_fused": (_I, [_I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "sed_conv_c1_gram_nparts": (_I, [_I, _I, _I]),
    "sed_conv3x3_c1_gram": (_I, [_P, _P, _P, _P, _I, _I, _I, _P]),
    "sed_conv3x3_c1_wgrad_combine": (_I, [_P, _P, _I, _P, _P, _P, _P, _P, _I, _I, _P]),
    "sed_c1_mode_supported": (_I, [_I, _I, _I, _I]),
    "sed_bn_train_finalize_c1": (_I, [_P, _I, _D, _P, _P, _P, _P, _P, _F, _F, _P, _P, _P, _P, _I, _I, _P]),
    "sed_bn_train_finalize_c1_g": (_I, [_P, _I, _D, _P, _P, _P, _P, _P, _F, _F, _P, _P, _P, _P, _I, _I, _P, _P]),
    "sed_c1_bwd_tail": (_I, [_P, _I, _P, _D, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P, _P]),
    "sed_conv3x3_fwd_c1": (_I, [_I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "sed_conv3x3_dgrad_c1": (_I, [_I, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "sed_conv_dgrad_c1_nparts": (_I, []),
    "sed_conv3x3_dgrad_c1_stats": (_I, [_I, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "sed_conv3x3_dgrad_c1_stats_g": (_I, [_I, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "sed_bn_bwd_finalize_c1": (_I, [_P, _I, _D, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P]),
    "sed_conv3x3_c1_dgrad": (_I, [_I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "sed_absmax": (_I, [_P, _Z, _P, _P]),
    "sed_bn_eval_stats": (_I, [_P, _P, _F, _P, _P, _I, _I, _P]),
    "sed_bn_eval_bwd_finalize": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P]),
    "sed_bn_eval_bwd_finalize_c1": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P]),
    "sed_conv3x3_wgrad_fused_c1": (_I, [_I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _I, _I,
                                        _I, _I, _P]),
    "sed_pack_conv_weights_batch": (_I, [_I, _P, _I, _I, _P]),
    "sed_conv3x3_bwd_fused_c1_supported": (_I, [_I, _I, _I, _I]),
    "sed_conv3x3_bwd_fused_c1": (_I, [_I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _I, _I, _I, _I,
                                      _P, _I, _I, _P]),
    "sed_conv3x3_bwd_fused_supported": (_I, [_I, _I, _I, _I, _I, _I, _I]),
    "sed_conv3x3_dgrad_dz_supported": (_I, [_I, _I, _I, _I, _I, _I, _I]),
    "sed_conv3x3_dgrad_dz": (_I, [_I, _I, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _I, _P, _I, _I, _I,
                                  _I, _I, _P]),
    "sed_conv3x3_wgrad_u": (_I, [_I, _I, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _I, _I, _P]),
    "sed_conv3x3_bwd_fused_supported_pool": (_I, [_I, _I, _I, _I, _I, _I, _I, _I]),
    "sed_conv3x3_bwd_fused": (_I, [_I, _I, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _I,
                                   _P, _P, _P, _I, _I, _I, _I, _I, _P, _I, _I, _P]),
    "sed_conv3x3_wgrad_fused_u": (_I, [_I, _I, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _I, _I, _I,
                                       _I, _I, _P, _I, _I, _P]),
    "sed_conv3x3_wgrad_fused_c1_u": (_I, [_I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _I, _I,
                                          _I, _I, _P, _I, _I, _P]),
    "sed_conv3x3_c1_wgrad_combine_u": (_I, [_P, _P, _I, _P, _P, _P, _P, _P, _I, _I, _P, _P]),
    "sed_conv_nparts": (_I, [_I, _I, _I]),
    "sed_conv3x3_fwd": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "sed_conv3x3_fwd_col": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "sed_conv_wgrad_ws_floats": (_Z, [_I, _I, _I, _I, _I]),
    "sed_conv3x3_wgrad": (_I, [_I, _I, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "sed_conv3x3_fwd_anyw": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "sed_conv3x3_wgrad_anyw": (_I, [_I, _I, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "sed_conv3x3_wgrad_fused": (_I, [_I, _I, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _I, _I, _I,
                                     _I, _I, _P]),
    "sed_bn_train_finalize": (_I, [_P, _I, _D, _P, _P, _P, _P, _F, _F, _P, _P, _P, _P, _I, _I, _P]),
    "sed_bn_eval_coeffs": (_I, [_P, _P, _P, _P, _F, _P, _P, _I, _I, _P]),
    "sed_bn_bwd_finalize": (_I, [_P, _I, _D, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P]),
    "sed_bn_relu_pool_fwd": (_I, [_I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "sed_pool_bwd_nparts": (_I, [_I, _I, _I, _I]),
    "sed_pool_relu_bwd_stats": (_I, [_I, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "sed_bn_relu_pool_cnt_fwd": (_I, [_I, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "sed_dgrad_poolstats_supported": (_I, [_I, _I, _I, _I]),
    "sed_conv3x3_dgrad_poolstats": (_I, [_I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _I, _I, _I, _I, _I, _P]),
    "sed_pool_relu_bwd_stats_if": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "sed_pool_relu_bn_bwd_apply": (_I, [_I, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "sed_bn_bwd_apply": (_I, [_I, _P, _P, _P, _P, _P, _P, _Z, _I, _P]),
    "sed_head_fwd": (_I, [_I, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "sed_interpolate": (_I, [_P, _P, _I, _I, _I, _I, _P]),
    "sed_bce_fwd_bwd": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _F, _F, _P]),
    "sed_clip_pool_fwd": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "sed_weak_bce_ws_bytes": (_Z, [_I, _I, _I]),
    "sed_weak_bce_fwd_bwd": (_I, [_P, _P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _F, _F, _F, _P, _P]),
    "sed_bce_sel_ws_bytes": (_Z, [_I, _I, _I]),
    "sed_bce_sel_fwd_bwd": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _F, _F, _F, _P, _P]),
    "sed_weak_bce_fwd_bwd_ex": (_I, [_P, _P, _I, _P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _F, _F, _F, _P, _P]),
    "sed_frame_mse_ws_bytes": (_Z, [_I, _I, _I]),
    "sed_frame_mse_fwd_bwd": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _F, _F, _P, _P]),
    "sed_ema_update": (_I, [_P, _P, _Z, _D, _P]),
    "sed_head_bwd_ws_floats": (_Z, [_I, _I, _I, _I]),
    "sed_head_bwd": (_I, [_I, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "sed_adam_amsgrad_step": (_I, [_P, _P, _P, _P, _P, _Z, _F, _F, _F, _F, _I, _F, _P]),
    "sed_adam_amsgrad_step_dev": (_I, [_P, _P, _P, _P, _P, _Z, _P, _P, _F, _F, _F, _F, _F, _I, _P]),
    "sed_grad_norm_nparts": (_I, [_Z]),
    "sed_grad_norm": (_I, [_P, _Z, _F, _F, _P, _I, _P, _P]),
    "sed_adam_step_ex": (_I, [_P, _P, _P, _P, _P, _Z, _F, _F, _F, _F, _I, _F, _F, _I, _P, _P]),
    "sed_adam_step_ex_dev": (_I, [_P, _P, _P, _P, _P, _Z, _P, _P, _F, _F, _F, _F, _F, _I, _F, _I, _P, _P]),
    "sed_opt_tile4": (_I, []),
    "sed_adam_groups_step": (_I, [_P, _P, _P, _P, _P, _Z, _P, _I, _P, _I, _P, _P, _P, _D, _I, _I, _I, _I, _D, _D, _F, _F, _F, _F, _I,
                                  _P, _P]),
    "sed_grad_norm_groups": (_I, [_P, _Z, _P, _I, _P, _F, _F, _P, _P, _P]),
    "sed_logmel_ws_bytes": (_Z, [_I, _I, _I, _I]),
    "sed_logmel_fwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "sed_stft_fwd": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "sed_complex_to_logmel": (_I, [_P, _P, _P, _P, _P, _P, _P, _Z, _I, _I, _P]),
    "sed_complex_augment_logmel": (_I, [_P, _Z, _P, _P, _P, _P, _P, _P, C.c_ulonglong, _P, _P, _P, _P, _P, _P, _I, _I,
                                        _I, _I, _P]),
    "sed_logmel_crops": (_I, [_P, _Z, _P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "sed_logmel_augment_row_ints": (_I, [_I, _I]),
    "sed_logmel_augment": (_I, [_P, _Z, _P, _I, _P, _P, _P, _P, _P, _F, _I, _P, _P, _I, _I, _I, _I, _I, _P]),
    "sed_resample_plan": (_I, [_I, _I, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "sed_resample_poly": (_I, [_I, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "sed_mel_mean_fwd": (_I, [_I, _P, _P, _Z, _I, _I, _I, _P]),
    "sed_mel_mean_bwd": (_I, [_I, _P, _P, _Z, _I, _I, _I, _P]),
    "sed_gemm_nt_ws_floats": (_Z, [_I, _I, _I]),
    "sed_gemm_nt": (_I, [_I, _P, _I, _P, _I, _P, _P, _I, _I, _I, _I, _I, _P, _P]),
    "sed_gemm_tn_ws_floats": (_Z, [_I, _I, _I]),
    "sed_gemm_tn": (_I, [_I, _P, _I, _P, _I, _P, _I, _P, _I, _I, _I, _I, _I, _I, _P, _P]),
    "sed_gemm_tn_batch": (_I, [_I, _P, _I, _P]),
    "sed_transpose_shift": (_I, [_P, _I, _P, _I, _I, _I, _I, _I, _P]),
    "sed_row_sums": (_I, [_P, _I, _P, _I, _I, _P]),
    "sed_gru_pack_elems": (_Z, [_I]),
    "sed_gru_pack_weights": (_I, [_I, _P, _P, _P, _P, _I, _P]),
    "sed_gru_seq_fwd": (_I, [_I, _P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "sed_gru_seq_bwd": (_I, [_I, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "sed_metric_counts_ws_bytes": (_Z, [_I]),
    "sed_metric_counts": (_I, [_P, _P, _P, _P, _I, _I, _P, _P, _P, _Z, _Z, _I, _P]),
    "sed_median_time_tile": (_I, []),
    "sed_median_time": (_I, [_P, _P, _I, _I, _I, _I, _P]),
    "sed_decode_events_chunk": (_I, []),
    "sed_decode_events_ws_bytes": (_Z, [_I, _I, _I]),
    "sed_decode_events": (_I, [_P, _I, _I, _I, _F, _F, _I, _I, _P, _P, _I, _P, _P, _P, _P]),
    "sed_segment_counts": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _P]),
    "sed_rank_tile": (_I, []),
    "sed_rank_ws_bytes": (_Z, [_I, _Z]),
    "sed_rank_pack": (_I, [_P, _P, _Z, _Z, _I, _P, _Z, _Z, _P, _P]),
    "sed_rank_sort": (_I, [_P, _I, _Z, _Z, _P, _P]),
    "sed_rank_curve": (_I, [_P, _I, _Z, _Z, _P, _P, _P, _P, _P]),
    "sed_psds_max_frames": (_I, [_I, _I]),
    "sed_psds_counts": (_I, [_P, _P, _I, _I, _I, _I, C.POINTER(C.c_float), _I, _I, _I, _I, _I, _I, _I, _P, _P, _P]),
    "sed_pcen_chunk": (_I, []),
    "sed_pcen_ws_bytes": (_Z, [_I, _I, _I]),
    "sed_pcen_fwd": (_I, [_P, _P, _P, _P, _I, _D, _D, _P, _P, _I, _I, _I, _P]),
    "sed_pcen_bwd": (_I, [_P, _P, _P, _P, _I, _D, _D, _P, _P, _P, _P, _I, _I, _I, _P]),
    "sed_att_logits_fwd": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "sed_att_pool_fwd": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "sed_att_loss_ws_bytes": (_Z, [_I, _I, _I]),
    "sed_att_loss_fwd_bwd": (_I, [_P, _P, _P, _I, _P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _F, _F, _F, _P, _P]),
    "sed_att_bwd_pack": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "sed_att_bwd_split": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _P]),
    "sed_mhsa_fwd": (_I, [_I, _P, _P, _P, _I, _I, _I, _I, _P]),
    "sed_mhsa_bwd_ws_floats": (_Z, [_I, _I, _I, _I]),
    "sed_mhsa_bwd": (_I, [_I, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "sed_add_layernorm_fwd": (_I, [_P, _P, _P, _P, _P, _P, _Z, _I, _F, _P]),
    "sed_add_layernorm_bwd_ws_floats": (_Z, [_Z, _I]),
    "sed_add_layernorm_bwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _Z, _I, _P]),
    "sed_ffn_fwd": (_I, [_I, _I, _P, _P, _P, _P, _P, _P, _P, _Z, _I, _I, _P]),
    "sed_ffn_act_bwd": (_I, [_I, _P, _P, _P, _P, _Z, _P]),
    # the dropout twins: the plain entry's arguments + (float p, const uint32_t* rng, uint32_t stream_id)
    "sed_mhsa_fwd_drop": (_I, [_I, _P, _P, _P, _I, _I, _I, _I, _F, _P, _U32, _P]),
    "sed_mhsa_bwd_drop": (_I, [_I, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _F, _P, _U32, _P]),
    "sed_add_layernorm_fwd_drop": (_I, [_P, _P, _P, _P, _P, _P, _Z, _I, _F, _F, _P, _U32, _P]),
    "sed_add_layernorm_bwd_drop": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _Z, _I, _F, _P, _U32, _P]),
    "sed_ffn_fwd_drop": (_I, [_I, _I, _P, _P, _P, _P, _P, _P, _P, _Z, _I, _I, _F, _P, _U32, _P]),
    "sed_ffn_act_bwd_drop": (_I, [_I, _P, _P, _P, _P, _Z, _I, _F, _P, _U32, _P]),
    "sed_dropout_mask": (_I, [_P, _I, _Z, _I, _I, _F, _P, _U32, _P]),
    # the local attention window: the plain entry's arguments + (int left, int right, float p, const uint32_t* rng, uint32_t stream_id)
    "sed_mhsa_fwd_win": (_I, [_I, _P, _P, _P, _I, _I, _I, _I, _I, _I, _F, _P, _U32, _P]),
    "sed_mhsa_bwd_win": (_I, [_I, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _F, _P, _U32, _P]),
    "sed_mhsa_win_tiles": (C.c_longlong, [_I, _I, _I, _I]),
    # the relative-position bias: the windowed entry's arguments + (const float* rel[, float* drel]) before the stream
    "sed_mhsa_fwd_rel": (_I, [_I, _P, _P, _P, _I, _I, _I, _I, _I, _I, _F, _P, _U32, _P, _P]),
    "sed_mhsa_bwd_rel_ws_floats": (_Z, [_I, _I, _I, _I, _I, _I]),
    "sed_mhsa_bwd_rel": (_I, [_I, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _F, _P, _U32, _P, _P, _P]),
    "sed_relpos_map_check": (_I, [_P, _I, _I]),
    "sed_relpos_expand": (_I, [_P, _P, _P, _I, _I, _I, _P]),
    "sed_relpos_fold": (_I, [_P, _P, _P, _I, _I, _I, _P]),
    # the pre-LN pair: (x, a, s, gamma, beta, xsum, y, stats, rows, C, eps, p, rng, stream_id) and
    # (dy, dres_in, xsum, gamma, stats, s, dxsum, da, dgamma, dbeta, workspace, rows, C, p, rng, stream_id)
    "sed_resid_layernorm_fwd": (_I, [_P, _P, _F, _P, _P, _P, _P, _P, _Z, _I, _F, _F, _P, _U32, _P]),
    "sed_resid_layernorm_bwd_ws_floats": (_Z, [_Z, _I]),
    "sed_resid_layernorm_bwd": (_I, [_P, _P, _P, _P, _P, _F, _P, _P, _P, _P, _P, _Z, _I, _F, _P, _U32, _P]),
    "sed_dwconv_tile": (_I, []),
    "sed_dwconv_nparts": (_I, [_I, _I]),
    "sed_dwconv_glu_fwd_ws_floats": (_Z, [_I, _I, _I]),
    "sed_dwconv_glu_fwd": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "sed_bn_silu_fwd": (_I, [_P, _P, _P, _P, _Z, _I, _P]),
    "sed_bn_silu_bwd_nparts": (_I, [_Z]),
    "sed_bn_silu_bwd_reduce": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _Z, _I, _P]),
    "sed_dwconv_glu_bwd_ws_floats": (_Z, [_I, _I, _I, _I]),
    "sed_dwconv_glu_bwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "sed_m5_conv1_len": (_I, [_I]),
    "sed_m5_conv1_nparts": (_I, [_I, _I]),
    "sed_m5_conv1_fwd": (_I, [_I, _P, _P, _P, _P, _I, _I, _P]),
    "sed_m5_conv1_wgrad": (_I, [_I, _P, _P, _P, _I, _I, _P]),
    "sed_m5_conv1_wgrad_fused": (_I, [_I, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P]),
    "sed_m5_conv1_wgrad_fused_pool": (_I, [_I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P]),
    "sed_m5_conv1_dgrad": (_I, [_I, _P, _P, _P, _I, _I, _P]),
    "sed_m5_conv1_dgrad_fused_pool": (_I, [_I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P]),
    "sed_m5_conv1_stats": (_I, [_I, _P, _P, _P, _I, _I, _P]),
    "sed_m5_conv1_bn_relu_pool_fwd": (_I, [_I, _P, _P, _P, _P, _P, _P, _I, _I, _P]),
    "sed_m5_fwd2_supported": (_I, [_I]),
    "sed_bn_relu_maxpool4_fwd": (_I, [_I, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "sed_maxpool4_bwd_nparts": (_I, [_I, _I, _I, _I]),
    "sed_maxpool4_relu_bwd": (_I, [_I, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "sed_maxpool4_pooled_stats": (_I, [_I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "sed_maxpool4_relu_bwd_if": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "sed_m5_head_fwd": (_I, [_I, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "sed_m5_head_bwd": (_I, [_I, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "sed_sum_partials": (_I, [_P, _I, _Z, _P, _P]),
    "sed_cast": (_I, [_I, _P, _I, _P, _Z, _P]),
    "sed_nchw_to_nhwc": (_I, [_I, _P, _P, _I, _I, _I, _I, _I, _P]),
    "sed_nhwc_to_nchw": (_I, [_I, _P, _P, _I, _I, _I, _I, _I, _P]),
    "sed_peak_mfma_bf16": (_I, [_I, _P, _P, _P]),
    "sed_peak_stream_copy": (_I, [_P, _P, _Z, _P]),
    "sed_peak_stream_read": (_I, [_P, _Z, _P, _P]),
}

_lib = None


def lib():
    """Load (once) and return the CDLL.  Raises if the HIP library has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: the MI355X kernels are not built. Run "
                "`python -c 'import __graft_entry__ as g; g.build()'` (or `make -C "
                f"{os.path.join(_HERE, 'csrc')}`). There is no CPU fallback.")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in PROTOTYPES.items():
            fn = getattr(L, name)          # AttributeError if a declared symbol is not exported
            fn.restype, fn.argtypes = res, args
        if L.sed_abi_version() != 1:
            raise RuntimeError("libsed_hip.so ABI version mismatch")
        _lib = L
    return _lib


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = lib().sed_last_error()
        raise RuntimeError(f"libsed_hip {what} failed (rc={rc}): {msg.decode() if msg else '?'}")


def ptr(t):
    """Device pointer of a torch tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()
