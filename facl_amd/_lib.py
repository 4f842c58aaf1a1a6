"""ctypes binding of libfacl_hip.so (the C ABI declared in include/facl_hip.h).

PyTorch is only plumbing here: tensors provide device memory (``data_ptr()``) and the current
HIP stream.  ``import torch`` MUST precede the dlopen so that the library binds to the HIP
runtime PyTorch already loaded (same SONAME libamdhip64.so.7) -- stream handles are only
meaningful inside one runtime.
"""
import ctypes
import os

import torch  # noqa: F401  (must be loaded before libfacl_hip.so, see module docstring)

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

c_p = ctypes.c_void_p
c_i = ctypes.c_int
c_f = ctypes.c_float
c_d = ctypes.c_double
c_l = ctypes.c_longlong


class c_s(ctypes.c_void_p):
    """The `void* stream` slot that closes an entry's signature: `call` fills it with the current stream."""


# name -> argtypes; every function returns int.  Kept in one table so tests can check that the
# library exports every symbol the header declares.
SIGNATURES = {
    "facl_version": [],
    "facl_fps_f32": [c_p, c_i, c_i, c_i, c_i, c_p, c_p, c_s],
    "facl_fps_f64": [c_p, c_i, c_i, c_i, c_i, c_p, c_p, c_s],
    "facl_fps_reorder": [c_p, c_i, c_i, c_i, c_p, c_i, c_p, c_s],
    "facl_group": [c_p, c_i, c_i, c_i, c_i, c_i, c_f, c_p, c_p, c_p, c_s],
    "facl_group_clips": [c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_f, c_p, c_p, c_p, c_s],
    "facl_gather_rows": [c_p, c_i, c_i, c_i, c_i, c_p, c_i, c_p, c_p, c_i, c_i, c_s],
    "facl_scatter_rows": [c_p, c_i, c_i, c_i, c_i, c_i, c_p, c_i, c_p, c_s],
    "facl_sinkhorn": [c_p, c_i, c_i, c_i, c_p, c_p, c_s],
    "facl_kmeans": [c_p, c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_s],
    "facl_adam_prep": [c_p, c_p, c_f, c_f, c_p, c_s],
    "facl_adam_apply": [c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_f, c_f, c_f, c_s],
    "facl_ws_bytes": [],
    "facl_bn_finalize": [c_p, c_i, c_d, c_p, c_p, c_f, c_f, c_p, c_p, c_p, c_p, c_p, c_s],
    "facl_bn_finalize_after": [c_p, c_i, c_d, c_p, c_p, c_f, c_f, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_s],
    "facl_bn_eval_consts_after": [c_i, c_p, c_p, c_p, c_p, c_f, c_p, c_p, c_i, c_s],
    "facl_absmax": [c_p, c_l, c_p, c_s],
    "facl_rows_act_amax": [c_p, c_l, c_i, c_p, c_p, c_p, c_s],
    "facl_bn_eval_consts": [c_i, c_p, c_p, c_p, c_p, c_f, c_p, c_s],
    "facl_sa_x_moments": [c_p, c_l, c_i, c_p, c_p, c_s],
    "facl_bn1_sums_from_moments": [c_p, c_d, c_i, c_p, c_p, c_p, c_s],
    "facl_sa_bn1_chain": [c_p, c_d, c_i, c_p, c_p, c_p, c_p, c_f, c_f, c_p, c_p, c_p, c_p, c_p, c_p, c_s],
    "facl_sa_l1tab": [c_p, c_p, c_i, c_p, c_p, c_p, c_p, c_p, c_s],
    "facl_sa_fwd2": [c_p, c_l, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_s],
    "facl_sa_fwd3": [c_p, c_l, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_s],
    "facl_sa_fwd3_h3": [c_p, c_l, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_s],
    "facl_sa_fwd3_f16": [c_p, c_l, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_s],
    "facl_sa_pool": [c_p, c_l, c_i, c_p, c_p, c_p, c_p, c_s],
    "facl_sa_eval": [c_p, c_l, c_i] + [c_p] * 11 + [c_s],
    "facl_rows_stats": [c_p, c_l, c_i, c_p, c_p, c_s],
    "facl_rows_bn_relu": [c_p, c_l, c_i, c_p, c_p, c_p, c_s],
    "facl_rows_segmax": [c_p, c_l, c_i, c_i, c_p, c_p, c_p, c_s],
    "facl_rows_bwd_stats": [c_p, c_p, c_l, c_i, c_p, c_p, c_p, c_s],
    "facl_rows_bwd_apply": [c_p, c_p, c_l, c_i, c_p, c_p, c_p, c_s],
    "facl_rows_bwd_apply_amax": [c_p, c_p, c_l, c_i, c_p, c_p, c_p, c_p, c_s],
    "facl_segmax_bwd_stats": [c_p, c_p, c_p, c_p, c_l, c_i, c_i, c_p, c_p, c_p, c_s],
    "facl_segmax_bwd_stats_ymax": [c_p, c_p, c_p, c_l, c_i, c_p, c_p, c_p, c_p, c_i, c_s],
    "facl_segmax_bwd_apply": [c_p, c_p, c_p, c_p, c_l, c_i, c_i, c_p, c_p, c_p, c_s],
    "facl_segmax_bwd_apply_amax": [c_p, c_p, c_p, c_p, c_l, c_i, c_i, c_p, c_p, c_p, c_p, c_s],
    "facl_gemm_fwd": [c_p, c_l, c_i, c_p, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_i, c_p, c_p, c_p, c_s],
    "facl_gemm_fwd_segmax": [c_p, c_l, c_i, c_p, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_s],
    "facl_gemm_dgrad": [c_p, c_l, c_i, c_p, c_i, c_i, c_p, c_s],
    "facl_gemm_wgrad": [c_p, c_p, c_l, c_i, c_i, c_i, c_p, c_p, c_i, c_s],
    "facl_gemm_fwd_f16": [c_p, c_l, c_i, c_p, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_i, c_p, c_p, c_p, c_s],
    "facl_gemm_fwd_segmax_f16": [c_p, c_l, c_i, c_p, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_s],
    "facl_gemm_dgrad_f16": [c_p, c_l, c_i, c_p, c_i, c_i, c_p, c_s],
    "facl_gemm_wgrad_f16": [c_p, c_p, c_l, c_i, c_i, c_i, c_p, c_p, c_i, c_s],
    "facl_gemm_wgrad_pro": [c_p, c_p, c_l, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_i, c_s],
    "facl_gemm_wgrad_pro_x3": [c_p, c_p, c_l, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_i, c_s],
    "facl_gemm_wgrad_h3": [c_p, c_p, c_l, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_s],
    "facl_gemm_rs_wgrad_slices": [c_l, c_i, c_i],
    "facl_gemm_rs_wgrad": [c_p, c_p, c_l, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_s],
    "facl_gemm_rs_planes_bytes": [c_i, c_i, c_i],
    "facl_gemm_rs_planes": [c_p, c_i, c_i, c_i, c_i, c_p, c_i, c_i, c_p, c_s],
    "facl_gemm_rs_planes_multi": [c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_l, c_p, c_s],
    "facl_gemm_rs_supported": [c_l, c_i, c_i],
    "facl_gemm_rs_fwd": [c_p, c_l, c_i, c_p, c_i, c_p, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_s],
    "facl_gemm_rs_dgrad": [c_p, c_l, c_i, c_p, c_i, c_p, c_i, c_p, c_s],
    "facl_gemm_rs_dgrad_bnstats": [c_p, c_l, c_i, c_p, c_i, c_p, c_i, c_p, c_p, c_p, c_p, c_p, c_s],
    "facl_gemm_fwd_x3": [c_p, c_l, c_i, c_p, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_i, c_p, c_p, c_p, c_s],
    "facl_gemm_fwd_segmax_x3": [c_p, c_l, c_i, c_p, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_s],
    "facl_gemm_dgrad_x3": [c_p, c_l, c_i, c_p, c_i, c_i, c_p, c_s],
    "facl_gemm_wgrad_x3": [c_p, c_p, c_l, c_i, c_i, c_i, c_p, c_p, c_i, c_s],
    "facl_sa_fwd3_x3": [c_p, c_l, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_s],
    "facl_contrast_pair": [c_p, c_i, c_i, c_i, c_i, c_p, c_i, c_p, c_p, c_p, c_s],
    "facl_normalize_map": [c_p, c_l, c_i, c_p, c_i, c_p, c_p, c_s],
    "facl_scale_rows2": [c_p, c_p, c_l, c_l, c_i, c_p, c_p, c_s],
    "facl_build_views_f32": [c_p, c_l, c_i, c_p, c_p, c_p, c_i, c_p, c_s],
    "facl_build_views_f64": [c_p, c_l, c_i, c_p, c_p, c_p, c_i, c_p, c_s],
    "facl_views_temporal_rows_f32": [c_p, c_l, c_i, c_p, c_i, c_p, c_p, c_p, c_s],
    "facl_views_temporal_rows_f64": [c_p, c_l, c_i, c_p, c_i, c_p, c_p, c_p, c_s],
    "facl_build_views_philox_f32": [c_p, c_l, c_i, c_p, c_p, c_p, c_l, c_i, c_i, c_p, c_p, c_s],
    "facl_build_views_philox_f64": [c_p, c_l, c_i, c_p, c_p, c_p, c_l, c_i, c_i, c_p, c_p, c_s],
    "facl_build_views_philox_gp_f32": [c_p, c_l, c_i, c_p, c_p, c_p, c_l, c_i, c_i, c_i, c_i, c_p, c_p, c_s],
    "facl_build_views_philox_gp_f64": [c_p, c_l, c_i, c_p, c_p, c_p, c_l, c_i, c_i, c_i, c_i, c_p, c_p, c_s],
    "facl_resident_temporal_rows_f32": [c_p, c_p, c_p, c_i, c_i, c_p, c_s],
    "facl_resident_temporal_rows_f64": [c_p, c_p, c_p, c_i, c_i, c_p, c_s],
    "facl_build_views_resident_f32": [c_p, c_p, c_p, c_i, c_p, c_i, c_l, c_i, c_p, c_p, c_p, c_s],
    "facl_build_views_resident_f64": [c_p, c_p, c_p, c_i, c_p, c_i, c_l, c_i, c_p, c_p, c_p, c_s],
    "facl_build_views_resident_gp_f32": [c_p, c_p, c_p, c_i, c_p, c_i, c_i, c_i, c_l, c_i, c_p, c_p, c_p, c_s],
    "facl_build_views_resident_gp_f64": [c_p, c_p, c_p, c_i, c_p, c_i, c_i, c_i, c_l, c_i, c_p, c_p, c_p, c_s],
    "facl_build_views_philox_recipe_f32": [c_p, c_l, c_i, c_p, c_p, c_p, c_l, c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_i, c_p, c_s],
    "facl_build_views_philox_recipe_f64": [c_p, c_l, c_i, c_p, c_p, c_p, c_l, c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_i, c_p, c_s],
    "facl_build_views_resident_recipe_f32": [c_p, c_p, c_p, c_i, c_p, c_i, c_i, c_i, c_l, c_i, c_p, c_p, c_p, c_p, c_i, c_p, c_s],
    "facl_build_views_resident_recipe_f64": [c_p, c_p, c_p, c_i, c_p, c_i, c_i, c_i, c_l, c_i, c_p, c_p, c_p, c_p, c_i, c_p, c_s],
    "facl_view_recipe_table": [c_p, c_i, c_p, c_p],
    "facl_sa_bwd0": [c_p, c_p, c_l, c_p, c_p, c_p, c_p, c_s],
    "facl_sa_bwd1": [c_p, c_l, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_s],
    "facl_sa_bwd_w3": [c_p, c_l, c_p, c_p, c_p, c_p, c_p, c_p, c_s],
    "facl_sa_bwd2": [c_p, c_p, c_p, c_l, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_s],
    "facl_sa_bwd_consts3": [c_p, c_p, c_p, c_p, c_d, c_p, c_p, c_s],
    "facl_sa_bwd_consts2": [c_p, c_p, c_d, c_p, c_s],
    "facl_bn_bwd_consts": [c_p, c_p, c_i, c_d, c_p, c_p, c_p, c_s],
    "facl_rows_center_wgrad": [c_p, c_p, c_l, c_i, c_p, c_p, c_s],
    "facl_viewmax_fwd": [c_p, c_i, c_i, c_i, c_p, c_p, c_s],
    "facl_viewmax_bwd": [c_p, c_p, c_i, c_i, c_i, c_p, c_s],
    "facl_viewmax_bwd_add": [c_p, c_p, c_i, c_i, c_i, c_p, c_s],
    "facl_sa_bwd_final": [c_p] * 13 + [c_i, c_d] + [c_p] * 9 + [c_s],
    "facl_bn_bwd_consts_frozen": [c_p, c_p, c_i, c_p, c_p, c_p, c_p, c_s],
    "facl_sa_bwd_consts3_frozen": [c_p, c_p, c_s],
    "facl_sa_bwd_consts2_frozen": [c_p, c_p, c_s],
    "facl_sa_bwd_final_frozen": [c_p] * 9 + [c_i] + [c_p] * 12 + [c_s],
    "facl_viewmax_stack": [c_p, c_i, c_i, c_i, c_p, c_p, c_s],
    "facl_fc_bn_stats": [c_p, c_l, c_l, c_i, c_p, c_p, c_s],
    "facl_fc_bn_apply": [c_p, c_l, c_l, c_i, c_p, c_p, c_i, c_i, c_d, c_d, c_p, c_p, c_f, c_f, c_p, c_p, c_p, c_p, c_s],
    "facl_fc_bn_bwd_stats": [c_p, c_p, c_l, c_l, c_i, c_p, c_p, c_p, c_s],
    "facl_fc_bn_bwd_apply": [c_p, c_p, c_l, c_l, c_i, c_p, c_p, c_p, c_d, c_d, c_p, c_p, c_p, c_p, c_s],
    "facl_col_sums": [c_p, c_l, c_i, c_p, c_s],
    "facl_contrast_pair_sum": [c_p, c_i, c_i, c_i, c_i, c_p, c_i, c_p, c_p, c_p, c_p, c_s],
    "facl_gemm_wgrad_acc": [c_p, c_p, c_l, c_i, c_i, c_i, c_p, c_i, c_s],
    "facl_contrast_pair_sum_mask": [c_p, c_i, c_i, c_i, c_i, c_p, c_i, c_i, c_p, c_p, c_p, c_p, c_s],
    "facl_loss_rows_fwd": [c_p, c_l, c_i, c_i, c_f, c_p, c_p, c_s],
    "facl_loss_rows_bwd": [c_p, c_p, c_p, c_l, c_i, c_i, c_f, c_p, c_s],
    "facl_contrast_pair_queue": [c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_p, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_s],
    "facl_queue_push": [c_p, c_i, c_i, c_p, c_i, c_p, c_s],
    "facl_contrast_pair_sum_cls": [c_p, c_i, c_i, c_i, c_i, c_p, c_i, c_p, c_p, c_p, c_p, c_p, c_s],
    "facl_contrast_pair_queue_cls": [c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_p, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_s],
    "facl_queue_push_ids": [c_p, c_i, c_p, c_i, c_p, c_s],
    "facl_contrast_pair_sum_sup": [c_p, c_i, c_i, c_i, c_i, c_p, c_i, c_p, c_f, c_p, c_p, c_p, c_p, c_s],
    "facl_contrast_pair_queue_sup": [c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_p, c_i, c_p, c_p, c_p, c_f, c_p, c_p, c_p, c_p, c_p, c_s],
    "facl_ema_apply": [c_i, c_p, c_p, c_p, c_f, c_s],
    "facl_grad_sqnorm": [c_i, c_p, c_p, c_p, c_s],
    "facl_adam_prep_ex": [c_p, c_p, c_f, c_f, c_p, c_i, c_d, c_i, c_i, c_i, c_d, c_p, c_s],
    "facl_adamw_apply": [c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_f, c_f, c_f, c_f, c_s],
    "facl_tensor_sqnorms": [c_i, c_p, c_p, c_p, c_p, c_p, c_s],
    "facl_sgd_prep": [c_p, c_p, c_p, c_p, c_i, c_i, c_p, c_p, c_d, c_i, c_i, c_i, c_i, c_d, c_d, c_d, c_p, c_p, c_s],
    "facl_sgd_apply": [c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_f, c_f, c_i, c_s],
    "facl_mailbox_bytes": [c_i, c_i],
    "facl_mailbox_alloc": [c_l, c_p, c_p],
    "facl_mailbox_open": [c_p, c_p],
    "facl_mailbox_close": [c_p],
    "facl_mailbox_free": [c_p],
    "facl_mailbox_allreduce": [c_p, c_p, c_i, c_i, c_p, c_i, c_i, c_p, c_p, c_s],
    "facl_gen3dv_frames": [c_p, c_i, c_i, c_i, c_p, c_p, c_p, c_s],
    "facl_gen3dv_voxelise": [c_p, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_l, c_l, c_d, c_p, c_p, c_p, c_p, c_s],
    "facl_gen3dv_volumes": [c_p, c_p, c_p, c_p, c_i, c_i, c_l, c_p, c_p, c_s],
    "facl_gen3dv_filter": [c_p, c_p, c_p, c_i, c_i, c_l, c_i, c_i, c_p, c_p, c_s],
    "facl_gen3dv_compact": [c_p, c_p, c_p, c_p, c_i, c_i, c_l, c_p, c_p, c_s],
    "facl_gen3dv_sample": [c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_l, c_p, c_l, c_i, c_p, c_p, c_p, c_p, c_p, c_s],
    "facl_gen3dv_app": [c_p, c_i, c_i, c_i, c_p, c_p, c_p, c_l, c_p, c_i, c_p, c_l, c_i, c_p, c_p, c_p, c_i, c_i, c_l, c_d,
                        c_p, c_p, c_p, c_p, c_s],
    "facl_knn_ws_bytes": [c_i, c_i, c_i],
    "facl_knn_topk": [c_p, c_i, c_i, c_p, c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_s],
    "facl_knn_vote": [c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_f, c_p, c_p, c_s],
    "facl_cls_gather_norm_fwd": [c_p, c_i, c_i, c_i, c_p, c_p, c_s],
    "facl_cls_gather_norm_bwd": [c_p, c_p, c_p, c_i, c_i, c_i, c_p, c_s],
    "facl_softmax_ce": [c_p, c_i, c_p, c_i, c_i, c_p, c_p, c_p, c_p, c_s],
    "facl_cls_probs_acc": [c_p, c_i, c_i, c_i, c_p, c_i, c_s],
    "facl_cls_topk": [c_p, c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_s],
    "facl_cluster_ws_bytes": [c_i, c_i, c_i],
    "facl_cluster_row_inv": [c_p, c_i, c_i, c_i, c_p, c_s],
    "facl_cluster_sums": [c_p, c_i, c_i, c_i, c_p, c_p, c_p, c_i, c_p, c_p, c_p, c_s],
    "facl_proto_nce_ws_bytes": [c_i],
    "facl_proto_nce": [c_p, c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_i, c_p, c_p, c_p, c_p, c_s],
}
RESTYPE_I64 = {"facl_ws_bytes", "facl_gemm_rs_planes_bytes", "facl_mailbox_bytes", "facl_knn_ws_bytes", "facl_cluster_ws_bytes",
               "facl_proto_nce_ws_bytes"}


def lib_path():
    # FACL_LIB: load another build of the same ABI (kernel experiments: A/B timing, parity of a candidate build)
    return os.environ.get("FACL_LIB") or os.path.join(_HERE, "libfacl_hip.so")


def load_library():
    """dlopen the HIP library; raises RuntimeError (never falls back) when it is missing."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} not found: facl_amd has no CPU/eager fallback. Build it with "
            "`python -m facl_amd.build` (hipcc --offload-arch=gfx950).")
    lib = ctypes.CDLL(path)
    for name, argtypes in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError here = header/library mismatch
        fn.argtypes = argtypes
        fn.restype = ctypes.c_longlong if name in RESTYPE_I64 else ctypes.c_int
    _LIB = lib
    return lib


E_SHAPE, E_NULL, E_ALIGN, E_CONFIG = -1, -2, -3, -4          # include/facl_hip.h: FACL_E_<NAME>
_ERR = {E_SHAPE: "unsupported shape", E_NULL: "NULL pointer", E_ALIGN: "misaligned pointer", E_CONFIG: "unsupported configuration"}


def check(rc, what):
    if rc != 0:
        msg = _ERR.get(rc, f"hipError {rc}")
        raise RuntimeError(f"{what} failed: {msg} (code {rc})")


def _invoke(name, args, stream_):
    """The C entry `name` on `args`: tensors as their device pointers, the stream slot filled, the count checked against
    SIGNATURES[name] (not fn.argtypes: a stand-in for the library need not carry them).  The function is looked up at call
    time, so whatever `load_library` returns now serves the call."""
    sig = SIGNATURES[name]
    if stream_ is not None:
        args += (stream_,)
    elif len(args) == len(sig) - 1 and sig[-1] is c_s:
        args += (stream(),)
    if len(args) != len(sig):
        raise TypeError("%s takes %d arguments%s, %d given"
                        % (name, len(sig), " (the stream may be left out)" if sig and sig[-1] is c_s else "", len(args)))
    return getattr(load_library(), name)(*[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args])


def call(name, *args, stream=None, detail=None, accept=()):
    """Launch the C entry `name`.  A tensor stands for its `data_ptr()`, None for NULL, everything else (numbers, the host arrays
    of `ptr_array` / `int_array`, raw addresses) goes through as it is.  An entry whose last slot is the stream (c_s) gets the
    current stream when that argument is left out; `stream=` names another one.  A non-zero return code raises through `check`
    under the entry's name (`detail`: shapes to add to the message) unless it is listed in `accept`: then it is returned, 0 on
    success -- `accept=(E_CONFIG,)` is how a caller learns that a fused kernel does not serve the shape and falls back."""
    rc = _invoke(name, args, stream)
    if rc != 0 and rc not in accept:
        check(rc, name if detail is None else "%s(%s)" % (name, detail))
    return rc


def call_size(name, *args, detail=None):
    """The value of an entry that returns a size or a count instead of a status (RESTYPE_I64, facl_gemm_rs_wgrad_slices,
    facl_gemm_rs_supported); a negative one is its refusal and raises like `call`."""
    n = _invoke(name, args, None)
    if n < 0:
        check(n, name if detail is None else "%s(%s)" % (name, detail))
    return n


def env_on(name, default="1"):
    """A/B switch from the environment: on unless set to 0."""
    return os.environ.get(name, default) != "0"


AMAX_WORDS = 2048          # include/facl_hip.h: FACL_AMAX_WORDS

# include/facl_hip.h: FACL_VIEW_<NAME>, the kind codes of a view recipe in code order, and the recipe's sizes
VIEW_KINDS = ("raw", "mirror", "key", "key_mirror", "rot", "t4", "t7", "res30", "res10", "jitter", "scale", "tilt_neg", "tilt_pos")
VIEW_POS_MAX = 12          # FACL_VIEW_POS_MAX: positions of a round at most
VIEW_NSTRENGTH = 6         # FACL_VIEW_NSTRENGTH: jitter_sigma, jitter_clip, rot_range, scale_lo, scale_hi, tilt_angle
VIEW_TABLE_COLS = 8        # FACL_VIEW_TABLE_COLS: int32 words per position of facl_view_recipe_table

# include/facl_hip.h: the chunk table of the optimizer entries (facl_adam_apply, facl_ema_apply, facl_grad_sqnorm, facl_adamw_apply,
# facl_tensor_sqnorms, facl_sgd_apply)
ADAM_MAX_TENSORS = 64      # FACL_ADAM_MAX_TENSORS: tensors per launch at most
ADAM_CHUNK = 2048          # FACL_ADAM_CHUNK: elements per workgroup; facl_grad_sqnorm writes one partial per chunk

# include/facl_hip.h: the input widths of grouping and the SA point-MLP, and the D-dependent layer-1 layouts
SA_D_MIN, SA_D_MAX = 3, 8  # FACL_SA_D_MIN, FACL_SA_D_MAX


def sa_l1_cols(D):
    """FACL_SA_L1_COLS(D): floats per row of the folded layer-1 table (weights, zero padding, the bias in column cols - 4, zeros)
    and rows of R1 in facl_sa_bwd2's output (x_0..x_{D-1}, then sum dz1, then zeros)."""
    return 8 if D <= 4 else 12


def sa_bwd2_out(D):
    """FACL_SA_BWD2_OUT(D): doubles of facl_sa_bwd2's output, [dW2 (64,64) | R1 (sa_l1_cols(D), 64)]."""
    return 64 * 64 + 64 * sa_l1_cols(D)


def amax_buffers(n, device, zero=True):
    """(n, AMAX_WORDS) int32: n operand-maximum buffers of the fp16x3 GEMMs (csrc/common.h).  Producers either STORE a bound
    into every slot (facl_bn_finalize) or RAISE slots with atomics (facl_sa_pool, facl_absmax, the BatchNorm-backward row
    kernels): the latter need zeros to start from -- `zero=False` when every row is stored or zeroed by a kernel of the step
    itself (facl_bn_finalize's `zamax`), which spares the fill launch."""
    if zero:
        return torch.zeros((n, AMAX_WORDS), dtype=torch.int32, device=device)
    return empty((n, AMAX_WORDS), dtype=torch.int32, device=device)


def ptr(t):
    """device pointer of a tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()


def ptr_array(tensors):
    """HOST array of the tensors' device pointers (a column of the optimizer entries' chunk table)."""
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def int_array(values):
    """HOST array of C ints (the table's element counts and flags)."""
    return (ctypes.c_int * len(values))(*[int(v) for v in values])


def stream():
    return torch.cuda.current_stream().cuda_stream


# ---- debug switch: poisoned scratch ------------------------------------------------------------------------------------
# Every output / scratch tensor the host layer hands to a kernel is `torch.empty` (the kernels write every element
# they later read).  With POISON on (FACL_POISON=1, or `with poisoned():`) those tensors and the partial-sum workspace are
# filled with NaN / 0xFF bytes first, so a partial row or an output element that a launch leaves unwritten for some
# ragged shape shows up as NaN in the results instead of silently reading whatever the allocator recycled.
POISON = os.environ.get("FACL_POISON", "0") not in ("", "0")


class poisoned:
    def __enter__(self):
        global POISON
        self.prev, POISON = POISON, True
        return self

    def __exit__(self, *exc):
        global POISON
        POISON = self.prev
        return False


def _poison(t):
    if POISON and t.numel():
        if t.is_floating_point():
            t.fill_(float("nan"))
        else:
            t.view(torch.uint8).fill_(0xFF)
    return t


def empty(*size, **kw):
    return _poison(torch.empty(*size, **kw))


def empty_like(t, **kw):
    return _poison(torch.empty_like(t, **kw))


def require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("facl_amd ops run on the GPU only (tensor is on %s); there is no CPU path" % t.device)


# ---- debug taps: integer side outputs of a forward that no caller of the reference's interface ever sees ----------------------
# When TAPS is a dict (tests: tests/helpers.routing_taps), forward passes drop the argmax tensors of their max-pools here
# ("sa_arg": max over the K neighbours, "seg_arg": my_max_pool over the S centroids, "view_arg": the view maximum), so a
# reference evaluation can route its gradients through the same positions (tie-proof gradient parity).
TAPS = None


def tap(name, t):
    if TAPS is not None:
        TAPS[name] = t.detach().clone()


def tap_relu(name, y=None, scale=None, shift=None, a=None):
    """ReLU decisions of a layer as a bool tensor: `a > 0` where the activation exists, else the sign of the kernels' own
    fma(scale, y, shift) (BatchNorm folded into two constants per channel) evaluated exactly: the product of two fp32
    numbers and the sum are exact enough in fp64 that the sign equals the sign of the fp32 FMA."""
    if TAPS is not None:
        TAPS[name] = (a > 0) if a is not None else ((y.double() * scale.double() + shift.double()) > 0)


# ---- optional in-step kernel timing (bench.py's roofline section) ----------------------------------------------------
# When TIMING is a dict, `timed(label)` brackets the launches issued inside the `with` block with HIP events on the
# launch stream (eager execution only: events cannot be recorded inside a graph replay) and appends the event pair to
# TIMING[label] (created on first use, so bench.py sees every heavy entry point of the step without a fixed list).
TIMING = None


class timed:
    def __init__(self, label):
        self.on = TIMING is not None
        self.label = label

    def __enter__(self):
        if self.on:
            import torch
            self.e0, self.e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            self.e0.record(torch.cuda.current_stream())
        return self

    def __exit__(self, *exc):
        if self.on:
            import torch
            self.e1.record(torch.cuda.current_stream())
            TIMING.setdefault(self.label, []).append((self.e0, self.e1))
        return False


def timing_ms(label):
    """Average milliseconds of the recorded brackets of `label` (synchronises)."""
    evs = TIMING.get(label)
    if not evs:
        return None
    evs[-1][1].synchronize()
    return sum(a.elapsed_time(b) for a, b in evs) / len(evs)


def timing_table():
    """{label: (average ms per bracket, number of brackets)} for everything recorded so far (synchronises)."""
    import torch
    torch.cuda.synchronize()
    return {k: (sum(a.elapsed_time(b) for a, b in v) / len(v), len(v)) for k, v in TIMING.items() if v}
