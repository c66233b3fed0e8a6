"""ctypes binding of libtmdiff_hip.so (include/tmdiff_hip.h).

The library is the product: if it is missing or fails to load, importing this module
raises -- there is no CPU or PyTorch fallback behind it.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TMDIFF_HIP_LIB") or os.path.join(_HERE, "libtmdiff_hip.so")   # override: diagnostic builds

c_float_p = C.POINTER(C.c_float)
vp = C.c_void_p


class Conv3dDesc(C.Structure):
    """struct tmdiff_conv3d_desc"""
    _fields_ = [
        ("B", C.c_int32), ("N", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
        ("Cin", C.c_int32), ("Cout", C.c_int32),
        ("groups", C.c_int32), ("ksize", C.c_int32), ("nseg", C.c_int32),
        ("seg_c", C.c_int32 * 3),
        ("seg_x", vp * 3),
        ("w_packed", vp), ("bias", vp), ("bias_scale", C.c_float),
        ("in_shift", vp), ("in_scale", vp), ("in_shift_stride", C.c_int32), ("in_scale_stride", C.c_int32),
        ("in_mask", vp), ("in_act", C.c_int32),
        ("residual", vp), ("out_scale", C.c_float),
        ("y", vp),
        ("y2", vp), ("y2_shift", vp), ("y2_scale", vp), ("y2_shift_stride", C.c_int32), ("y2_scale_stride", C.c_int32),
        ("y2_act", C.c_int32), ("y2_bf16", C.c_int32), ("x_bf16", C.c_int32),
        ("splitk_ws", vp), ("splitk_ws_bytes", C.c_int64),
        ("drop_seed", C.c_uint64), ("drop_p", C.c_float), ("drop_seed_dev", vp), ("rc_x", vp), ("rc_w", vp), ("rc_cin", C.c_int32), ("y_ll", vp), ("y_hi", vp * 3), ("xp_out", vp), ("xp_shift", vp), ("xp_shift_stride", C.c_int32), ("xp_act", C.c_int32),
        ("y2_s2d", C.c_int32),
    ]


# name -> (restype, argtypes); mirrors include/tmdiff_hip.h one to one
SIGNATURES = {
    "tmdiff_version": (C.c_int, []),
    "tmdiff_last_error_string": (C.c_char_p, []),
    "tmdiff_conv3d_pack_weights": (C.c_int, [vp, vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp]),
    "tmdiff_conv3d_pack_weights_multi_chunks": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]),
    "tmdiff_conv3d_pack_weights_multi": (C.c_int, [vp, vp, vp, C.c_int32, vp]),
    "tmdiff_conv3d_fwd": (C.c_int, [C.POINTER(Conv3dDesc), vp]),
    "tmdiff_conv3d_fwd_splitk_workspace_bytes": (C.c_size_t, [C.POINTER(Conv3dDesc)]),
    "tmdiff_conv3d_fwd_xp_supported": (C.c_int, [C.POINTER(Conv3dDesc)]),
    "tmdiff_conv3d_fwd_staged_supported": (C.c_int, [C.POINTER(Conv3dDesc)]),
    "tmdiff_conv3d_fwd_staged_workspace_bytes": (C.c_size_t, [C.POINTER(Conv3dDesc)]),
    "tmdiff_conv3d_fwd_staged": (C.c_int, [C.POINTER(Conv3dDesc), vp, vp]),
    "tmdiff_conv3d_wino_supported": (C.c_int, [C.POINTER(Conv3dDesc)]),
    "tmdiff_conv3d_wino_blocks": (C.c_int64, [C.POINTER(Conv3dDesc)]),
    "tmdiff_conv3d_wino_workspace_bytes": (C.c_size_t, [C.POINTER(Conv3dDesc)]),
    "tmdiff_conv3d_wino_planes": (C.c_int32, [C.c_int32]),
    "tmdiff_conv3d_wino_packed_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "tmdiff_conv3d_wino_pack_weights": (C.c_int, [vp, vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp]),
    "tmdiff_conv3d_wino_pack_weights_multi_chunk": (C.c_int32, []),
    "tmdiff_conv3d_wino_pack_weights_multi": (C.c_int, [vp, vp, vp, C.c_int32, vp]),
    "tmdiff_conv3d_wf_supported": (C.c_int, [C.POINTER(Conv3dDesc)]),
    "tmdiff_conv3d_wf_blocks": (C.c_int64, [C.POINTER(Conv3dDesc)]),
    "tmdiff_conv3d_wf_workspace_bytes": (C.c_size_t, [C.POINTER(Conv3dDesc)]),
    "tmdiff_conv3d_wf_splitk_workspace_bytes": (C.c_size_t, [C.POINTER(Conv3dDesc)]),
    "tmdiff_conv3d_wf_fwd": (C.c_int, [C.POINTER(Conv3dDesc), vp, vp]),
    "tmdiff_conv3d_w2_supported": (C.c_int, [C.POINTER(Conv3dDesc)]),
    "tmdiff_conv3d_w2_epilogue_supported": (C.c_int, [C.POINTER(Conv3dDesc)]),
    "tmdiff_conv3d_w2_workspace_bytes": (C.c_size_t, [C.POINTER(Conv3dDesc)]),
    "tmdiff_conv3d_w2_packed_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "tmdiff_conv3d_w2_pack_weights": (C.c_int, [vp, vp, C.c_int32, C.c_int32, vp]),
    "tmdiff_conv3d_w2_fwd": (C.c_int, [C.POINTER(Conv3dDesc), vp, C.c_int32, vp]),
    "tmdiff_conv3d_wino_fwd": (C.c_int, [C.POINTER(Conv3dDesc), vp, vp]),
    "tmdiff_conv3d_wino_fwd_planes": (C.c_int, [C.POINTER(Conv3dDesc), vp, C.c_int32, vp, C.c_int32, vp]),
    "tmdiff_conv3d_wino_fwd_xp": (C.c_int, [C.POINTER(Conv3dDesc), vp, C.c_int32, vp, vp]),
    "tmdiff_conv3d_wino_fwd_stage": (C.c_int, [C.POINTER(Conv3dDesc), vp, C.c_int32, vp]),
    "tmdiff_conv3d_prologue_fwd": (C.c_int, [C.POINTER(Conv3dDesc), vp, vp]),
    "tmdiff_conv3d_ll_supported": (C.c_int, [C.POINTER(Conv3dDesc)]),
    "tmdiff_conv3d_ll_splitk_workspace_bytes": (C.c_size_t, [C.POINTER(Conv3dDesc)]),
    "tmdiff_conv3d_ll_packed_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "tmdiff_conv3d_ll_pack_weights": (C.c_int, [vp, vp, C.c_int32, C.c_int32, C.c_float, vp]),
    "tmdiff_conv3d_ll_fwd": (C.c_int, [C.POINTER(Conv3dDesc), C.c_float, vp]),
    "tmdiff_conv3d_packed_bf16_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "tmdiff_conv3d_pack_weights_bf16": (C.c_int, [vp, vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp]),
    "tmdiff_conv3d_bf16_workspace_bytes": (C.c_size_t, [C.POINTER(Conv3dDesc)]),
    "tmdiff_conv3d_fwd_bf16": (C.c_int, [C.POINTER(Conv3dDesc), vp, vp]),
    "tmdiff_conv3d_wgrad_workspace_bytes": (C.c_size_t, [C.POINTER(Conv3dDesc)]),
    "tmdiff_conv3d_wgrad": (C.c_int, [C.POINTER(Conv3dDesc), vp, vp, vp, vp]),
    "tmdiff_conv3d_wgrad_bias": (C.c_int, [C.POINTER(Conv3dDesc), vp, vp, vp, vp, vp]),
    "tmdiff_conv3d_wf_plan": (C.c_int32, [C.c_int32] * 8 + [C.POINTER(C.c_int64)]),
    "tmdiff_conv3d_wfll_supported": (C.c_int, [C.POINTER(Conv3dDesc)]),
    "tmdiff_conv3d_wfll_packed_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "tmdiff_conv3d_wfll_pack_weights": (C.c_int, [vp, vp, C.c_int32, C.c_int32, C.c_float, vp]),
    "tmdiff_conv3d_wfll_splitk_workspace_bytes": (C.c_size_t, [C.POINTER(Conv3dDesc)]),
    "tmdiff_conv3d_wfll_fwd": (C.c_int, [C.POINTER(Conv3dDesc), C.c_float, vp]),
    "tmdiff_conv3d_wgrad_wino_supported": (C.c_int, [C.POINTER(Conv3dDesc)]),
    "tmdiff_conv3d_wgrad_wino_workspace_bytes": (C.c_size_t, [C.POINTER(Conv3dDesc)]),
    "tmdiff_conv3d_wgrad_wino": (C.c_int, [C.POINTER(Conv3dDesc), vp, vp, vp, vp]),
    "tmdiff_conv3d_wgrad_wino_bias": (C.c_int, [C.POINTER(Conv3dDesc), vp, vp, vp, vp, vp]),
    "tmdiff_conv3d_pack_weights_bf16_dgrad": (C.c_int, [vp, vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp]),
    "tmdiff_conv3d_wgrad_bf16_supported": (C.c_int, [C.POINTER(Conv3dDesc)]),
    "tmdiff_conv3d_wgrad_bf16_workspace_bytes": (C.c_size_t, [C.POINTER(Conv3dDesc)]),
    "tmdiff_conv3d_wgrad_bf16_slots": (C.c_int32, [C.POINTER(Conv3dDesc)]),
    "tmdiff_conv3d_wgrad_bf16": (C.c_int, [C.POINTER(Conv3dDesc), vp, vp, vp, vp, vp]),
    "tmdiff_channel_sum": (C.c_int, [vp, vp, C.c_int32, C.c_int32, C.c_int64, C.c_float, vp]),
    "tmdiff_conv3d_prologue_bwd": (C.c_int, [C.POINTER(Conv3dDesc), vp, vp * 3, C.c_int32 * 3, vp, vp, vp]),
    "tmdiff_conv3d_prologue_bwd_workspace_bytes": (C.c_size_t, [C.POINTER(Conv3dDesc)]),
    "tmdiff_conv3d_prologue_bwd_ws": (C.c_int, [C.POINTER(Conv3dDesc), vp, vp * 3, C.c_int32 * 3, vp, vp, vp, vp]),
    "tmdiff_conv3d_prologue_bwd_add": (C.c_int, [C.POINTER(Conv3dDesc), vp, vp * 3, vp * 3, vp, vp, vp, vp]),
    "tmdiff_stem_bwd": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp]),
    "tmdiff_stem_bwd_input": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                        vp]),
    "tmdiff_head_bwd": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_int32, C.c_int32, C.c_int64, vp]),
    "tmdiff_linear_bwd": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp]),
    "tmdiff_stem_fwd": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                  C.c_int32, vp]),
    "tmdiff_head_fwd": (C.c_int, [vp, vp, vp, C.c_int32, vp, C.c_int32, C.c_int32, C.c_int64, vp]),
    "tmdiff_haar_dwt2d": (C.c_int, [vp, vp, vp, vp, vp, C.c_int64, C.c_int32, C.c_int32, C.c_float, C.c_float, vp]),
    "tmdiff_haar_idwt2d": (C.c_int, [vp * 2, C.c_int32, vp, vp, vp, C.c_int64, C.c_int64, vp * 2, C.c_int64,
                                     C.c_int32, C.c_int32, C.c_float, vp]),
    "tmdiff_linear_fwd": (C.c_int, [vp, vp, vp, vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp]),
    "tmdiff_gamma_embedding": (C.c_int, [vp, vp, vp, C.c_int32, C.c_int32, vp]),
    "tmdiff_ddpm_step": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_float,
                                   C.c_float, C.c_int32, vp]),
    "tmdiff_ddpm_step_dev": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_int64, vp, vp, C.c_int32, C.c_int32, C.c_int32, vp]),
    "tmdiff_sampler_tick": (C.c_int, [vp, vp, C.c_int32, C.c_int32, vp]),
    "tmdiff_ddpm_frame_slot": (C.c_int, [C.c_int32, C.c_int32, C.c_int32]),
    "tmdiff_axpby": (C.c_int, [vp * 4, C.c_float * 4, C.c_int32, vp, C.c_int64, vp]),
    "tmdiff_multi_axpby_chunk": (C.c_int32, []),
    "tmdiff_multi_axpby": (C.c_int, [vp, vp, vp, C.c_int32, C.c_float, C.c_float, vp]),
    "tmdiff_multi_adamw": (C.c_int, [vp, vp, vp, C.c_int32, vp, vp, C.c_float, C.c_float, C.c_float, C.c_float, vp]),
    "tmdiff_multi_sqnorm_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "tmdiff_multi_sqnorm_partial": (C.c_int, [vp, vp, vp, C.c_int32, vp, vp]),
    "tmdiff_multi_sqnorm_finish": (C.c_int, [vp, C.c_int32, C.c_float, vp, vp, vp, vp]),
    "tmdiff_multi_adamw_scaled": (C.c_int, [vp, vp, vp, C.c_int32, vp, vp, C.c_float, C.c_float, C.c_float, C.c_float, vp, vp,
                                            vp]),
    "tmdiff_x0_from_model": (C.c_int, [vp, vp, vp, C.c_int64, C.c_float, C.c_float, C.c_int32, vp]),
    "tmdiff_abs_quantile_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int64]),
    "tmdiff_abs_quantile_clamp": (C.c_int, [vp, C.c_int32, C.c_int64, C.c_float, C.c_float, vp, vp]),
    "tmdiff_add": (C.c_int, [vp, vp, vp, C.c_int64, C.c_float, vp]),
    "tmdiff_attn_fwd": (C.c_int, [vp, vp, vp, vp, vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                  C.c_int64 * 3, C.c_int64 * 3, C.c_int64 * 3, C.c_int64 * 3, C.c_float, vp]),
    "tmdiff_attn_ctx_queries_per_workgroup": (C.c_int32, [C.c_int32] * 5),
    "tmdiff_attn_fwd_lse": (C.c_int, [vp, vp, vp, vp, vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                      C.c_int64 * 3, C.c_int64 * 3, C.c_int64 * 3, C.c_int64 * 3, C.c_float, vp, vp]),
    "tmdiff_attn_bwd_supported": (C.c_int, [C.c_int32] * 5),
    "tmdiff_attn_bwd_workspace_bytes": (C.c_size_t, [C.c_int32] * 5),
    "tmdiff_attn_bwd": (C.c_int, [vp] * 11 + [C.c_int32] * 5 + [C.c_int64 * 3] * 4 + [C.c_float, vp]),
    "tmdiff_gemm_nt": (C.c_int, [vp, vp, vp, vp, vp, C.c_int64, C.c_int32, C.c_int32, vp]),
    "tmdiff_group_norm": (C.c_int, [vp, vp, vp, vp, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_float, vp]),
    "tmdiff_layer_norm": (C.c_int, [vp, vp, vp, vp, C.c_int64, C.c_int32, C.c_float, vp]),
    "tmdiff_geglu": (C.c_int, [vp, vp, C.c_int64, C.c_int32, C.c_int32, vp]),
    "tmdiff_layer_norm_stats": (C.c_int, [vp] * 6 + [C.c_int64, C.c_int32, C.c_float, vp]),
    "tmdiff_group_norm_stats": (C.c_int, [vp] * 6 + [C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_float, vp]),
    "tmdiff_layer_norm_bwd_supported": (C.c_int, [C.c_int64, C.c_int32]),
    "tmdiff_layer_norm_bwd_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32]),
    "tmdiff_layer_norm_bwd": (C.c_int, [vp] * 9 + [C.c_int64, C.c_int32, vp]),
    "tmdiff_group_norm_bwd_supported": (C.c_int, [C.c_int32, C.c_int32, C.c_int64, C.c_int32]),
    "tmdiff_group_norm_bwd_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int64, C.c_int32]),
    "tmdiff_group_norm_bwd": (C.c_int, [vp] * 9 + [C.c_int32, C.c_int32, C.c_int64, C.c_int32, vp]),
    "tmdiff_geglu_bwd": (C.c_int, [vp, vp, vp, C.c_int64, C.c_int32, C.c_int32, vp]),
    "tmdiff_q_sample": (C.c_int, [vp, vp, vp, vp, C.c_int32, C.c_int64, vp]),
    # per-operator names (thin fronts of the entry points above)
    "tmdiff_conv3d_k3_fwd": (C.c_int, [C.POINTER(Conv3dDesc), vp]),
    "tmdiff_conv3d_k3_dgrad": (C.c_int, [C.POINTER(Conv3dDesc), vp]),
    "tmdiff_conv3d_k3_wgrad": (C.c_int, [C.POINTER(Conv3dDesc), vp, vp, vp, vp]),
    "tmdiff_conv3d_k1_fwd": (C.c_int, [C.POINTER(Conv3dDesc), vp]),
    "tmdiff_conv3d_k1_dgrad": (C.c_int, [C.POINTER(Conv3dDesc), vp]),
    "tmdiff_conv3d_k1_wgrad": (C.c_int, [C.POINTER(Conv3dDesc), vp, vp, vp, vp]),
    "tmdiff_haar_dwt2d_fwd": (C.c_int, [vp, vp, vp, vp, vp, C.c_int64, C.c_int32, C.c_int32, C.c_float, C.c_float, vp]),
    "tmdiff_haar_dwt2d_bwd": (C.c_int, [vp, vp, vp, vp, vp, C.c_int64, C.c_int32, C.c_int32, C.c_float, C.c_float, vp]),
    "tmdiff_haar_idwt2d_fwd": (C.c_int, [vp, vp, vp, vp, vp, C.c_int64, C.c_int32, C.c_int32, C.c_float, vp]),
    "tmdiff_haar_idwt2d_bwd": (C.c_int, [vp, vp, vp, vp, vp, C.c_int64, C.c_int32, C.c_int32, C.c_float, vp]),
    "tmdiff_dpm_axpby2": (C.c_int, [vp, C.c_float, vp, C.c_float, vp, C.c_int64, vp]),
    "tmdiff_dpm_axpby3": (C.c_int, [vp, C.c_float, vp, C.c_float, vp, C.c_float, vp, C.c_int64, vp]),
    "tmdiff_dpm_axpby4": (C.c_int, [vp, C.c_float, vp, C.c_float, vp, C.c_float, vp, C.c_float, vp, C.c_int64, vp]),
}


class PlanePrologue(C.Structure):
    """struct tmdiff_plane_prologue"""
    _fields_ = [("shift", vp), ("scale", vp), ("shift_stride", C.c_int32), ("scale_stride", C.c_int32),
                ("C", C.c_int32), ("n_per_channel", C.c_int32), ("act", C.c_int32)]


SIGNATURES.update({
    "tmdiff_haar_dwt2d_pro": (C.c_int, [vp, vp, vp, vp, vp, C.c_int64, C.c_int32, C.c_int32, C.c_float, C.c_float,
                                        C.POINTER(PlanePrologue), vp]),
    "tmdiff_haar_idwt2d_pro": (C.c_int, [vp * 2, C.c_int32, vp, vp, vp, C.c_int64, C.c_int64, vp * 2, C.c_int64,
                                         C.c_int32, C.c_int32, C.c_float, C.POINTER(PlanePrologue), vp]),
    "tmdiff_haar_dwt2d_pack_bf16": (C.c_int, [vp, vp, vp, vp, vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                              C.c_float, C.c_float, C.POINTER(PlanePrologue), vp]),
    "tmdiff_haar_idwt2d_pack_bf16": (C.c_int, [vp, vp, vp, vp, vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                               C.c_float, C.POINTER(PlanePrologue), vp]),
    "tmdiff_stem_fwd_pack_bf16": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_int32, vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                            C.c_int32, C.c_int32, vp]),
    "tmdiff_stem_fwd_scaled": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_int32, vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                         C.c_int32, C.c_int32, vp]),
    # overlapped scene tiles (csrc/tiles.hip): (B, C, H, W, tile, overlap) after the two tensors
    "tmdiff_tile_plan": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_int32]),
    "tmdiff_tile_supported": (C.c_int, [C.c_int32] * 6),
    "tmdiff_tile_gather": (C.c_int, [vp, vp] + [C.c_int32] * 6 + [vp]),
    "tmdiff_tile_blend": (C.c_int, [vp, vp] + [C.c_int32] * 6 + [vp]),
    # quality metrics (csrc/metrics.hip): tensors come with their batch / channel strides in elements
    "tmdiff_metrics_supported": (C.c_int, [C.c_int32] * 4),
    "tmdiff_metrics_workspace_bytes": (C.c_size_t, [C.c_int32] * 4),
    "tmdiff_metrics_pair": (C.c_int, [vp, C.c_int64, C.c_int64, vp, C.c_int64, C.c_int64] + [C.c_int32] * 4 +
                            [C.c_double, C.c_double, vp, vp, C.c_size_t, vp]),
    "tmdiff_metrics_noref": (C.c_int, [vp, C.c_int64, C.c_int64, vp, C.c_int64, vp, C.c_int64, vp, C.c_int64, C.c_int64] +
                             [C.c_int32] * 6 + [vp, vp, C.c_size_t, vp]),
    "tmdiff_metrics_q2n_supported": (C.c_int, [C.c_int32] * 6),
    "tmdiff_metrics_q2n_workspace_bytes": (C.c_size_t, [C.c_int32] * 6),
    "tmdiff_metrics_q2n": (C.c_int, [vp, C.c_int64, C.c_int64, vp, C.c_int64, C.c_int64] + [C.c_int32] * 6 +
                           [vp, vp, vp, C.c_size_t, vp]),                    # ... block, shift, out, map_out, workspace
    "tmdiff_metrics_dsblock_supported": (C.c_int, [C.c_int32] * 5),
    "tmdiff_metrics_dsblock_workspace_bytes": (C.c_size_t, [C.c_int32] * 5),
    # ps, strides, ms_exp, strides, pan, stride, pan_lp, stride | B, C, H, W, block | q, d_lambda, alpha, beta | out, maps, workspace
    "tmdiff_metrics_dsblock": (C.c_int, [vp, C.c_int64, C.c_int64, vp, C.c_int64, C.c_int64, vp, C.c_int64, vp, C.c_int64] +
                               [C.c_int32] * 5 + [C.c_double, vp, C.c_double, C.c_double, vp, vp, vp, C.c_size_t, vp]),
    # composite finetune loss (csrc/loss.hip): x0, xhat, ms, g | base_kind, w_sam, w_lap | out64, out32, workspace, bytes | B, C, H, W
    "tmdiff_loss_supported": (C.c_int, [C.c_int32] * 5),
    "tmdiff_loss_workspace_bytes": (C.c_size_t, [C.c_int32] * 5),
    "tmdiff_spectral_spatial_loss": (C.c_int, [vp] * 4 + [C.c_int32, C.c_double, C.c_double, vp, vp, vp, C.c_size_t] +
                                     [C.c_int32] * 4 + [vp]),
    # SSIM loss term (csrc/ssim_loss.hip): x_true, x_pred, ms, g | win, data_range, weight, accumulate | terms_in, out64, out32,
    # workspace, bytes | B, C, H, W
    "tmdiff_ssim_loss_supported": (C.c_int, [C.c_int32] * 5),
    "tmdiff_ssim_loss_workspace_bytes": (C.c_size_t, [C.c_int32] * 5),
    "tmdiff_ssim_loss": (C.c_int, [vp] * 4 + [C.c_int32, C.c_double, C.c_double, C.c_int32, vp, vp, vp, vp, C.c_size_t] +
                         [C.c_int32] * 4 + [vp]),
    # local PAN-correlation loss (csrc/local_corr.hip): x, pan, g, rho_max | win, weight, accumulate | out64, per_image, out32,
    # workspace, bytes | B, C, H, W
    "tmdiff_local_corr_loss_supported": (C.c_int, [C.c_int32] * 5),
    "tmdiff_local_corr_loss_workspace_bytes": (C.c_size_t, [C.c_int32] * 5),
    "tmdiff_local_corr_loss": (C.c_int, [vp] * 4 + [C.c_int32, C.c_double, C.c_int32, vp, vp, vp, vp, C.c_size_t] +
                               [C.c_int32] * 4 + [vp]),
    # resampling (csrc/resample.hip): (planes, H, W, levels | ratio) after the two tensors
    "tmdiff_pyr_down": (C.c_int, [vp, vp] + [C.c_int32] * 4 + [vp]),
    "tmdiff_upsample_bilinear": (C.c_int, [vp, vp] + [C.c_int32] * 4 + [vp]),
    "tmdiff_upsample_poly23": (C.c_int, [vp, vp] + [C.c_int32] * 5 + [vp]),      # ... ratio, phase
    # FIR filtering with decimation (csrc/mtf.hip): x, taps, y | planes, taps_period, H, W, K, ratio, off_y, off_x
    "tmdiff_fir_decimate": (C.c_int, [vp, vp, vp] + [C.c_int32] * 8 + [vp]),
    # its adjoint: g, taps, base, dx | alpha, beta | planes, taps_period, H, W, K, ratio, off_y, off_x
    "tmdiff_fir_decimate_adjoint": (C.c_int, [vp, vp, vp, vp, C.c_float, C.c_float] + [C.c_int32] * 8 + [vp]),
    # MTF-GLP: the filter bank: x, taps, y | images, tables, H, W, K, ratio, off_y, off_x
    "tmdiff_fir_decimate_bank": (C.c_int, [vp, vp, vp] + [C.c_int32] * 8 + [vp]),
    # ms_exp, pan, pan_lp | B, C, H, W | out, workspace, bytes;  ms_exp, pan, pan_lp, moments, out | B, C, H, W, mode
    "tmdiff_glp_moments_workspace_bytes": (C.c_size_t, [C.c_int32] * 4),
    "tmdiff_glp_moments": (C.c_int, [vp, vp, vp] + [C.c_int32] * 4 + [vp, vp, C.c_size_t, vp]),
    "tmdiff_glp_inject": (C.c_int, [vp] * 5 + [C.c_int32] * 5 + [vp]),
    # component substitution: ms, pan | B, C, H, W | out, workspace, bytes;  full, low, out | B, C, mode;
    # ms_exp, pan, coef, out | B, C, H, W, mode
    "tmdiff_plane_gram_workspace_bytes": (C.c_size_t, [C.c_int32] * 4),
    "tmdiff_plane_gram": (C.c_int, [vp, vp] + [C.c_int32] * 4 + [vp, vp, C.c_size_t, vp]),
    "tmdiff_cs_coeffs": (C.c_int, [vp, vp, vp] + [C.c_int32] * 3 + [vp]),
    "tmdiff_cs_inject": (C.c_int, [vp] * 4 + [C.c_int32] * 5 + [vp]),
    # BDSD: low_lp, low_pan, low_ms | B, C, H, W, bs | out, workspace, bytes;  moments, out | systems, C;
    # ms_exp, pan, gamma, out | B, C, H, W, block
    "tmdiff_bdsd_gram_workspace_bytes": (C.c_size_t, [C.c_int32] * 5),
    "tmdiff_bdsd_gram": (C.c_int, [vp, vp, vp] + [C.c_int32] * 5 + [vp, vp, C.c_size_t, vp]),
    "tmdiff_bdsd_solve": (C.c_int, [vp, vp] + [C.c_int32] * 2 + [vp]),
    "tmdiff_bdsd_inject": (C.c_int, [vp] * 4 + [C.c_int32] * 5 + [vp]),
    # conjugate gradients for Wald's consistency (csrc/cg.hip): a0, b0, n0, partials0, a1, b1, n1, partials1 | planes;
    # partials, out | planes, count, items, item_stride;  p, q, d, r, gamma, qq, pp | damp | rr | planes, n_full, n_low, first;
    # s, p, gamma_new, gamma_old, pp | planes, n_full
    "tmdiff_plane_dots_partials": (C.c_int32, [C.c_int32]),
    "tmdiff_plane_dots": (C.c_int, [vp, vp, C.c_int32, vp, vp, vp, C.c_int32, vp, C.c_int32, vp]),
    "tmdiff_plane_totals": (C.c_int, [vp, vp, C.c_int32, C.c_int32, C.c_int32, C.c_int64, vp]),
    "tmdiff_cg_step": (C.c_int, [vp] * 7 + [C.c_double, vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp]),
    "tmdiff_cg_direction": (C.c_int, [vp] * 5 + [C.c_int32, C.c_int32, vp]),
    # TV pansharpening (csrc/tv.hip): u, x, pan, ph, pv, weights | tau, sigma, lam, gamma | x', ph', pv' | B, C, H, W;
    # x | B, C, H, W | out, workspace, bytes
    "tmdiff_tv_supported": (C.c_int, [C.c_int32] * 4),
    "tmdiff_tv_pd_step": (C.c_int, [vp] * 6 + [C.c_double] * 4 + [vp] * 3 + [C.c_int32] * 4 + [vp]),
    "tmdiff_tv_norm_workspace_bytes": (C.c_size_t, [C.c_int32] * 4),
    "tmdiff_tv_norm": (C.c_int, [vp] + [C.c_int32] * 4 + [vp, vp, C.c_size_t, vp]),
    # a-trous wavelet pansharpening (csrc/atrous.hip): B, C, H, W, levels, first; x, out | B, C, H, W, levels, first;
    # ms_exp, pan, pan_lp, moments, out | B, C, H, W, mode
    "tmdiff_atrous_supported": (C.c_int, [C.c_int32] * 6),
    "tmdiff_atrous_lowpass": (C.c_int, [vp, vp] + [C.c_int32] * 6 + [vp]),
    "tmdiff_awlp_inject": (C.c_int, [vp] * 5 + [C.c_int32] * 5 + [vp]),
})


class TmdiffError(RuntimeError):
    """Non-zero status from the C ABI (the reference surfaces errors as ordinary exceptions)."""


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `make` (or `python -c 'import __graft_entry__ as g; g.build()'`). "
            "tmdiff_amd has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError here == header/library mismatch
        fn.restype, fn.argtypes = res, args
    return lib


lib = _load()
ABI_VERSION = lib.tmdiff_version()


def check(status, what=""):
    if status != 0:
        msg = lib.tmdiff_last_error_string().decode("utf-8", "replace")
        raise TmdiffError(f"{what or 'tmdiff'} failed with status {status}: {msg}")
