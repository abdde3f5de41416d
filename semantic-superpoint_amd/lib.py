"""ctypes binding of include/ssp_hip.h plus `Engine`, the owner of the torch-allocated device buffers.

PyTorch is plumbing here: it allocates HBM, provides the stream and (in the trainer) RCCL; every
arithmetic step runs in csrc/libssp_hip.so.  There is NO CPU / eager fallback: if the library cannot be
loaded or the tensors are not on a HIP device, calls raise.
"""
import ctypes as C
import math
import os
from collections import OrderedDict

import numpy as np
import torch

from . import hipbuild as _build

ARCHS = {"SuperPointNet_gauss2": 0, "SuperPointNet_gauss2_ssmall": 1}
SCALAR_NAMES = ["loss", "loss_det", "loss_det_warp", "loss_desc", "loss_sem", "loss_sem_warp", "positive_dist",
                "negative_dist", "eta_det", "eta_desc", "eta_sem"]
N_SCALARS = 16
NREP = 32  # SSP_NREP
SAMPLER_MAX_MATCHES = 8192  # SAMPLER_MAX_CELLS of csrc/sem_kernels.hip.h (bitonic sort capacity of the device sampler)
PROF = {"none": 0, "conv3x3_fwd": 1, "conv3x3_dgrad": 2, "conv3x3_wgrad": 3, "conv_big_fwd": 4, "conv3x3_all": 5,
        "conv3x3_every": 6}
PROF_KERNELS = ["conv_wino4_kernel", "conv_wino_pipe_kernel", "conv_wino_p2_kernel", "wgrad_wino_kernel", "wgrad_wino4_kernel",
                "other", "conv_bf16_kernel", "wgrad_bf16_kernel"]  # SSP_PROF_K_*


class SspConfig(C.Structure):
    _fields_ = [("arch", C.c_int), ("n_classes", C.c_int), ("max_batch", C.c_int), ("height", C.c_int),
                ("width", C.c_int), ("n_match", C.c_int), ("n_non", C.c_int), ("dense_loss", C.c_int)]


class SspBuffers(C.Structure):
    _fields_ = [("params_dev", C.c_void_p), ("grads_dev", C.c_void_p), ("adam_m_dev", C.c_void_p),
                ("adam_v_dev", C.c_void_p), ("bn_running_dev", C.c_void_p), ("num_batches_tracked_dev", C.c_void_p),
                ("workspace_dev", C.c_void_p), ("workspace_bytes", C.c_size_t)]


class SspPairInputs(C.Structure):
    _fields_ = [("batch", C.c_int), ("image_dev", C.c_void_p), ("warped_image_dev", C.c_void_p),
                ("labels_dev", C.c_void_p), ("warped_labels_dev", C.c_void_p), ("valid_mask_dev", C.c_void_p),
                ("warped_valid_mask_dev", C.c_void_p), ("homographies_dev", C.c_void_p), ("semantic_dev", C.c_void_p),
                ("warped_semantic_dev", C.c_void_p), ("match_a_dev", C.c_void_p), ("match_b_dev", C.c_void_p),
                ("nonmatch_b_dev", C.c_void_p), ("seed", C.c_uint64), ("lambda_loss", C.c_float),
                ("lamda_d", C.c_float), ("multi_task", C.c_int), ("train", C.c_int), ("dense_loss", C.c_int),
                ("dense_lamda_d", C.c_float), ("descriptor_dist", C.c_float), ("cell_homographies_dev", C.c_void_p),
                ("sparse_method", C.c_int), ("sparse_dist", C.c_int)]


class SspHomographyParams(C.Structure):
    _fields_ = [("perspective", C.c_int32), ("scaling", C.c_int32), ("rotation", C.c_int32), ("translation", C.c_int32),
                ("allow_artifacts", C.c_int32), ("n_scales", C.c_int32), ("n_angles", C.c_int32),
                ("scaling_amplitude", C.c_float), ("perspective_amplitude_x", C.c_float),
                ("perspective_amplitude_y", C.c_float), ("patch_ratio", C.c_float), ("max_angle", C.c_float),
                ("translation_overflow", C.c_float)]


class SspPhotometricParams(C.Structure):
    """ssp_photometric_params (include/ssp_hip.h): `struct_size` first; the enable fields are counts (see photometric_params_from_config)."""
    _fields_ = [("struct_size", C.c_uint32), ("random_brightness", C.c_int32), ("random_contrast", C.c_int32),
                ("additive_gaussian_noise", C.c_int32), ("additive_speckle_noise", C.c_int32), ("motion_blur", C.c_int32),
                ("additive_shade", C.c_int32), ("brightness_max_abs_change", C.c_int32),
                ("contrast_lo", C.c_float), ("contrast_hi", C.c_float), ("noise_std_lo", C.c_float), ("noise_std_hi", C.c_float),
                ("impulse_prob_lo", C.c_float), ("impulse_prob_hi", C.c_float), ("shade_nb_ellipses", C.c_int32),
                ("shade_transparency_lo", C.c_float), ("shade_transparency_hi", C.c_float),
                ("shade_kernel_lo", C.c_int32), ("shade_kernel_hi", C.c_int32)]


# the row of draws (SSP_PHOTO_* of include/ssp_hip.h)
PHOTO_MAX_ELLIPSES, PHOTO_MAX_KSIZE = 32, 351
(PHOTO_BRIGHTNESS, PHOTO_CONTRAST, PHOTO_SIGMA, PHOTO_IMPULSE_P, PHOTO_BLUR_FLAG, PHOTO_BLUR_W, PHOTO_ELLIPSES, PHOTO_TRANSPARENCY,
 PHOTO_KSIZE, PHOTO_KEY, PHOTO_DRAW_STRIDE) = 0, 1, 2, 3, 4, 5, 14, 174, 175, 176, 180


class SspShapesParams(C.Structure):
    """ssp_shapes_params (include/ssp_hip.h): `struct_size` first (see shapes_params_from_config)."""
    _fields_ = [("struct_size", C.c_uint32), ("gen_h", C.c_int32), ("gen_w", C.c_int32), ("out_h", C.c_int32), ("out_w", C.c_int32),
                ("blur_size", C.c_int32), ("weights", C.c_float * 9),
                ("bg_nb_blobs", C.c_int32), ("bg_min_kernel", C.c_int32), ("bg_max_kernel", C.c_int32),
                ("bg_min_rad_ratio", C.c_float), ("bg_max_rad_ratio", C.c_float),
                ("lines_nb_lines", C.c_int32), ("polygon_max_sides", C.c_int32), ("multi_max_sides", C.c_int32),
                ("multi_nb_polygons", C.c_int32), ("multi_nb_blobs", C.c_int32), ("multi_kernel_lo", C.c_int32),
                ("multi_kernel_hi", C.c_int32), ("ellipses_nb", C.c_int32), ("star_nb_branches", C.c_int32),
                ("checker_max_rows", C.c_int32), ("checker_max_cols", C.c_int32), ("stripes_max_nb_cols", C.c_int32),
                ("checker_transform", C.c_float * 2), ("stripes_transform", C.c_float * 2), ("stripes_min_width_ratio", C.c_float),
                ("cube_min_size_ratio", C.c_float), ("cube_scale", C.c_float * 2), ("cube_trans", C.c_float * 2),
                ("resize_scale_y", C.c_float), ("resize_scale_x", C.c_float), ("gauss_w", C.c_float * 63)]


# the scene table row (SSP_SHAPES_* of include/ssp_hip.h)
SHAPES_PRIMITIVES = ["draw_lines", "draw_polygon", "draw_multiple_polygons", "draw_ellipses", "draw_star", "draw_checkerboard",
                     "draw_stripes", "draw_cube", "gaussian_noise"]  # SyntheticDataset_gaussian.drawing_primitives
SHAPES_MAX_BLOBS, SHAPES_MAX_CMDS, SHAPES_MAX_VERTS, SHAPES_MAX_TEX, SHAPES_MAX_POINTS, SHAPES_MAX_BLUR = 128, 64, 256, 32, 256, 63
(SHAPES_PRIM, SHAPES_THR, SHAPES_KEY, SHAPES_KSIZE, SHAPES_NBLOBS, SHAPES_MEAN0, SHAPES_MEAN, SHAPES_NCMDS, SHAPES_NPOINTS, SHAPES_NVERTS,
 SHAPES_NTEX, SHAPES_BLOBS, SHAPES_CMDS, SHAPES_VERTS, SHAPES_TEX, SHAPES_POINTS, SHAPES_ROW) = (0, 1, 2, 4, 5, 6, 7, 8, 9, 10, 11, 16, 528, 1296,
                                                                                              1808, 2192, 2704)


class SspDetEvalParams(C.Structure):
    _fields_ = [("height", C.c_int32), ("width", C.c_int32), ("remove_zero", C.c_float), ("r2", C.c_int32),
                ("prob_thresh", C.c_float), ("simplified", C.c_int32)]


class SspWorldUpkeepParams(C.Structure):
    _fields_ = [("merge", C.c_int32), ("merge_thresh", C.c_double), ("cull_age", C.c_int32), ("cull_min_views", C.c_int32),
                ("high_water", C.c_int32), ("low_water", C.c_int32)]


class SspExportParams(C.Structure):
    _fields_ = [("n_views", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("conf_thresh", C.c_float),
                ("nms_dist", C.c_int32), ("border_remove", C.c_int32), ("top_k", C.c_int32), ("subpixel", C.c_int32)]


_lib = None


def _signatures():
    """{name: (argtypes, restype)} of every function declared in include/ssp_hip.h, in the header's order.  load_library applies
    it; tests/test_boundary_cpu.py holds every argtypes list against the number of parameters of the declaration."""
    vp, i, f, d, sz, u32, u64, i64, P = (C.c_void_p, C.c_int, C.c_float, C.c_double, C.c_size_t, C.c_uint32, C.c_uint64, C.c_int64,
                                         C.POINTER)
    return {
        "ssp_last_error": ([], C.c_char_p),
        "ssp_build_id": ([], C.c_char_p),
        "ssp_set_deterministic": ([i], i),
        "ssp_get_deterministic": ([], i),
        "ssp_clock_probe": ([f, P(d), vp], i),
        "ssp_create": ([P(SspConfig), P(vp)], i),
        "ssp_destroy": ([vp], None),
        "ssp_param_count": ([vp], sz),
        "ssp_bn_channel_count": ([vp], sz),
        "ssp_bn_layer_count": ([vp], i),
        "ssp_workspace_bytes": ([vp], sz),
        "ssp_bind": ([vp, P(SspBuffers), vp], i),
        "ssp_forward": ([vp, i, vp, i, i, i, i, vp, vp, vp, vp], i),
        "ssp_backward": ([vp, i, vp, vp, vp, vp], i),
        "ssp_zero_grad": ([vp, vp], i),
        "ssp_pair_step": ([vp, P(SspPairInputs), vp, vp], i),
        "ssp_adam_step": ([vp, f, i, vp], i),
        "ssp_adam_step_scaled": ([vp, f, i, f, vp], i),
        "ssp_pair_step_phase": ([vp, P(SspPairInputs), vp, i, vp], i),
        "ssp_grad_early_offset": ([vp], sz),
        "ssp_pair_step_graph": ([vp, P(SspPairInputs), vp, i, i, vp], i),
        "ssp_sample_indices": ([vp, vp, i, u64, vp, vp, vp, vp], i),
        "ssp_sample_indices_cell": ([vp, vp, i, u64, vp, vp, vp, vp], i),
        "ssp_profile_enable": ([vp, i], i),
        "ssp_profile_read": ([vp, P(d), P(i64), P(d), P(d)], i),
        "ssp_profile_pause": ([vp, i], i),
        "ssp_profile_read_kernel": ([vp, i, P(d), P(i64), P(d), P(d), P(d)], i),
        "ssp_profile_read_executed": ([vp, P(d)], i),
        "ssp_op_conv": ([vp, vp, vp, vp] + [i] * 7 + [vp, vp, vp, i, vp, sz, vp], i),
        "ssp_op_conv_wgrad": ([vp, vp, vp] + [i] * 7 + [vp, vp, vp, sz, vp], i),
        "ssp_op_conv_bf16": ([vp, vp, vp, vp] + [i] * 7 + [vp, vp, vp, i, i, i, vp, vp, vp, sz, vp], i),
        "ssp_op_conv_wgrad_bf16": ([vp, vp, vp] + [i] * 7 + [vp, vp, i, vp, sz, vp], i),
        "ssp_op_bn_bwd_bf16": ([vp] * 9 + [i] * 7 + [vp], i),
        "ssp_op_labels": ([vp, vp, vp, vp, i, i, i, vp], i),
        "ssp_op_detector_loss": ([vp, i, vp, vp, i, i, i, vp, sz, vp, vp, vp], i),
        "ssp_op_sem_loss": ([vp, i, vp] + [i] * 5 + [vp, sz, vp, vp, vp], i),
        "ssp_op_sem_predict": ([vp, i, vp, i, i, i, i, vp, vp, vp], i),
        "ssp_sem_predict": ([vp, i, vp, vp, vp, vp], i),
        "ssp_op_warp_image": ([vp, vp, vp, i, i, i, i, vp], i),
        "ssp_op_erode": ([vp, vp, i, i, i, i, vp], i),
        "ssp_op_warp_labels": ([vp, vp, vp, i, i, i, vp], i),
        "ssp_op_warp_labels_px": ([vp, vp, vp, i, i, i, vp], i),
        "ssp_op_sample_homographies": ([u64, P(SspHomographyParams), i, vp, vp, vp], i),
        "ssp_op_warp_labels_full": ([vp] * 5 + [i, i, i, vp], i),
        "ssp_op_warp_labels_full_px": ([vp] * 5 + [i, i, i, vp], i),
        "ssp_op_label_quantize": ([vp, vp, sz, vp], i),
        "ssp_op_sem_finalize": ([vp, vp, vp, sz, i, vp], i),
        "ssp_op_photometric_draw": ([u64, P(SspPhotometricParams), i, i, i, vp, vp], i),
        "ssp_op_photometric_apply": ([vp, vp, vp, i, i, i, vp], i),
        "ssp_shapes_workspace_bytes": ([P(SspShapesParams), i], sz),
        "ssp_op_shapes_draw": ([u64, P(SspShapesParams), i, vp, vp], i),
        "ssp_op_shapes_render": ([vp, P(SspShapesParams), i] + [vp] * 5, i),
        "ssp_op_warp_points_scatter": ([vp, vp, vp, vp, i, i, i, i, vp], i),
        "ssp_export_workspace_bytes": ([P(SspExportParams)], sz),
        "ssp_export_max_points": ([P(SspExportParams)], i),
        "ssp_export_points": ([vp, P(SspExportParams), i] + [P(vp)] * 7 + [vp], i),
        "ssp_op_homoadapt_views": ([vp, vp, vp, vp, i, i, i, vp], i),
        "ssp_op_flatten_detection": ([vp, vp, vp, i, i, i, vp], i),
        "ssp_op_combine_heatmap": ([vp, vp, vp, vp, i, i, i, vp], i),
        "ssp_op_heatmap_points": ([vp, P(SspExportParams), vp, vp, vp, vp], i),
        "ssp_op_soft_argmax_points": ([vp, vp, vp, i, i, i, vp], i),
        "ssp_detector_heatmap": ([vp, i, vp, vp], i),
        "ssp_op_heatmap_nms": ([vp, P(SspExportParams), i] + [vp] * 5, i),
        "ssp_describe_workspace_bytes": ([P(SspExportParams), i], sz),
        "ssp_describe_points": ([vp, i, P(SspExportParams), i] + [vp] * 5, i),
        "ssp_op_sample_descriptors": ([vp, i, i, i, vp, vp, i, vp, vp], i),
        "ssp_match_workspace_bytes": ([i, i], sz),
        "ssp_match_two_way": ([vp, vp, vp, vp, i, i, i, f, vp, vp, vp, vp], i),
        "ssp_op_point_classes": ([vp] + [i] * 5 + [vp, i, vp, i, vp, vp], i),
        "ssp_point_classes": ([vp, i, i, vp, i, vp, i, vp, vp], i),
        "ssp_filter_workspace_bytes": ([i, i], sz),
        "ssp_op_filter_points": ([vp, vp, vp, vp, P(u32), i, i] + [vp] * 6, i),
        "ssp_match_two_way_classes": ([vp] * 6 + [i, i, i, f, vp, vp, vp, vp], i),
        "ssp_eval_repeatability": ([vp, vp, vp, vp, i, i, i, vp, vp, i, i, i, d, vp, vp], i),
        "ssp_eval_ransac_workspace_bytes": ([i, i], sz),
        "ssp_eval_ransac": ([vp, vp, i, i, i] + [vp] * 10, i),
        "ssp_epi_ransac_workspace_bytes": ([i, i], sz),
        "ssp_epi_ransac": ([vp, vp, i, i, i, i, vp, vp, vp, d, i] + [vp] * 8, i),
        "ssp_op_filter_matches": ([vp] * 5 + [i, i, i, vp, vp, vp], i),
        "ssp_pose_from_fundamental": ([vp] * 6 + [i, i, i, i, vp, vp, vp, i] + [vp] * 11, i),
        "ssp_pose_chain": ([vp] * 5 + [i] + [vp] * 7 + [i, i, vp, vp, i, vp], i),
        "ssp_pose_from_homography": ([vp] * 6 + [i] * 4 + [vp, vp, vp, i, vp, vp, d, d] + [vp] * 13, i),
        "ssp_model_select": ([vp] * 10 + [i] * 4 + [vp, vp, d] + [vp] * 6, i),
        "ssp_landmark_workspace_bytes": ([i, i], sz),
        "ssp_map_window": ([vp, vp, i, vp, i, i, i, vp, vp], i),
        "ssp_op_triangulate_tracks": ([vp, vp, vp, i, vp, i, i, i, i, d, d] + [vp] * 6, i),
        "ssp_op_landmarks_select": ([vp] * 8 + [i, i, i, vp, vp, vp, vp], i),
        "ssp_pnp_workspace_bytes": ([i], sz),
        "ssp_op_landmark_matches": ([vp, vp, i, vp, vp, i, vp, i, i, vp, vp, vp], i),
        "ssp_pnp_ransac": ([vp, vp, i, i, vp, i, vp, d, i, i] + [vp] * 9, i),
        "ssp_pose_repair": ([vp, vp, vp, i, vp, vp, i, vp], i),
        "ssp_ba_workspace_bytes": ([i, i], sz),
        "ssp_bundle_adjust": ([vp, vp, vp, i, vp, i, i, i, vp, vp, i] + [vp] * 6, i),
        "ssp_ba_apply": ([vp, vp, i, i, i, vp, vp, i, vp], i),
        "ssp_world_insert_workspace_bytes": ([i], sz),
        "ssp_match_world_workspace_bytes": ([i, i], sz),
        "ssp_op_world_insert": ([vp, vp, i, vp, vp, i, vp] + [i] * 5 + [vp] * 11, i),
        "ssp_match_world": ([vp, vp, i, vp, vp, i, f, vp, vp, vp, vp], i),
        "ssp_op_world_correspondences": ([vp, vp, i, vp, vp, i, vp, i, vp, i, vp, vp, vp], i),
        "ssp_world_repair": ([vp] * 5 + [i, i, vp, vp], i),
        "ssp_world_upkeep_workspace_bytes": ([i], sz),
        "ssp_op_world_upkeep": ([vp, vp, i, vp, vp, i, vp, i, vp, i, vp, i, i, vp, vp, i, i] + [vp] * 13, i),
        "ssp_op_track_class_votes": ([vp, vp, i, vp, vp, i, vp, i, vp], i),
        "ssp_op_world_classes": ([vp, vp, i, vp, i, vp, vp], i),
        "ssp_match_world_classes": ([vp, vp, vp, i, vp, i, vp, vp, vp, i, P(u32), f, vp, vp, vp, vp], i),
        "ssp_op_traj_align": ([vp, i, vp, i, vp, i, i, vp, i, i, i, vp, vp], i),
        "ssp_op_traj_ape": ([vp, i, vp, i, vp, i, i, vp, i, i, vp, vp, vp, vp, vp], i),
        "ssp_op_traj_rpe_delta": ([vp, i, vp, i, vp, i, i, vp, i, i, vp, i, i, vp, vp, vp, vp], i),
        "ssp_op_traj_rpe_segments": ([vp, i, vp, i, vp, i, i, vp, i, i, vp, i, vp, i, i, vp, vp, vp, vp, vp], i),
        "ssp_op_traj_stats": ([vp, vp, i, i, vp, vp], i),
        "ssp_pose_graph_workspace_bytes": ([i], sz),
        "ssp_op_loop_correspondences": ([vp, vp, vp, i, vp, vp, i, vp, i, vp, i, vp, vp, i, i, i, vp, vp, vp, vp], i),
        "ssp_loop_edge": ([vp] * 7 + [i, vp, i, vp, i, i, i, i, d, vp, vp, vp, vp], i),
        "ssp_pose_graph": ([vp, i, vp, vp, i, i] + [vp] * 6, i),
        "ssp_loop_apply": ([vp] * 5 + [i, vp, vp, i, vp, vp, vp, i, vp], i),
        "ssp_eval_pixel_homographies": ([vp, i, i, i, vp, vp, vp], i),
        "ssp_eval_accumulate": ([vp] * 6 + [i, vp, i, i, i, P(d), i64, vp, i64, vp, vp], i),
        "ssp_det_eval_workspace_bytes": ([P(SspDetEvalParams), i, i], sz),
        "ssp_op_det_tp_fp": ([vp, vp, i, P(SspDetEvalParams), i, vp, vp, i64, vp, vp], i),
        "ssp_op_det_tp_fp_points": ([vp, vp, i, vp, i, P(SspDetEvalParams), i, vp, vp, i64, vp, vp], i),
        "ssp_det_pr_curve_workspace_bytes": ([i64], sz),
        "ssp_op_det_pr_curve": ([vp, i64] + [vp] * 8, i),
        "ssp_track_workspace_bytes": ([i, i, i], sz),
        "ssp_op_track_update": ([vp] * 8 + [i, i, i] + [vp] * 6, i),
        "ssp_op_track_select": ([vp, vp, vp, vp, i, i, i, vp, vp, vp, vp], i),
        "ssp_op_track_points": ([vp, vp, vp, vp, i, i, i, i, vp, vp], i),
        "ssp_op_bn_bwd": ([vp] * 9 + [i] * 6 + [vp], i),
        "ssp_op_bn_bwd_strided": ([vp] * 9 + [i] * 7 + [vp], i),
        "ssp_set_conv_algo": ([i], i),
        "ssp_handle_set_conv_algo": ([vp, i], i),
        "ssp_debug_conv_knobs": ([i, i], i),
        "ssp_debug_occupancy": ([i], i),
        "ssp_debug_buffer": ([vp, i, C.c_char_p, P(vp), P(sz)], i),
        "ssp_debug_backward_taps": ([vp, vp, sz, u32], i),
        "ssp_debug_backward_tap_floats": ([vp, u32], sz),
        "ssp_debug_backward_tap": ([vp, i, i, i, P(sz), P(sz), P(u32)], i),
        "ssp_op_sparse_loss": ([vp] * 5 + [i] * 7 + [f, f, vp, vp, vp, vp], i),
        "ssp_op_sparse_loss_path": ([vp] * 5 + [i] * 7 + [f, f, vp, vp, vp, i, vp, vp, vp, vp], i),
        "ssp_op_dense_loss": ([vp, vp, vp, vp, i, i, i, f, f, i, f, vp, sz, vp, vp, vp, vp], i),
    }


SIGNATURES = _signatures()
EXPORTS = list(SIGNATURES)

MATCH_MAX_POINTS = 4096  # SSP_MATCH_MAX_POINTS (include/ssp_hip.h)
TRACK_MAX_LENGTH = 16  # SSP_TRACK_MAX_LENGTH (include/ssp_hip.h)
TRACK_NO_SCORE = 9999.0  # score of a track that has no match yet (PointTracker.max_score)
CLASS_NONE = 255  # SSP_CLASS_NONE (include/ssp_hip.h): the class of a row past its image's point count
DET_EVAL_MAX_R2 = 64  # SSP_DET_EVAL_MAX_R2 (include/ssp_hip.h): largest squared match radius of the detector evaluation
DET_EVAL_STATE_WORDS = 80  # SSP_DET_EVAL_STATE_WORDS: int64 words of an evaluation state block
DET_EVAL_OUTSIDE = 3  # state word: point-list rows skipped because they lie outside the image (DET_STATE_OUTSIDE)
DET_EVAL_HIST = 8  # first word of the d2 histogram in a state block (DET_STATE_HIST, csrc/detector_eval_kernels.hip.h)
DET_CURVE_TILE = 1024  # DET_CURVE_TILE (csrc/detector_eval_kernels.hip.h): records per workgroup of the curve kernels
EVAL_ACC_MAX_PAIRS = 128  # SSP_EVAL_ACC_MAX_PAIRS (include/ssp_hip.h): pairs per ssp_eval_accumulate call
EVAL_ROW_WORDS = 16  # SSP_EVAL_ROW_WORDS: fp64 words of a pair's row of the streamed descriptor metrics
EVAL_STATE_WORDS = 16  # SSP_EVAL_STATE_WORDS: fp64 words of their state block
POSE_ROW_WORDS = 16  # SSP_POSE_ROW_WORDS: fp64 words of a trajectory row (Rw [9], C [3], s, n_shared, flags, ratio)
POSE_STATE_WORDS = 16  # SSP_POSE_STATE_WORDS: fp64 words of a pose chain state (n_frames, s, Rw [9], tw [3], 2 spare)
POSE_FLAG_NO_POSE, POSE_FLAG_SCALE_CARRIED = 1, 2  # flag bits of a trajectory row
CAM_WORDS = 20  # SSP_CAM_WORDS: fp64 words of a camera record (Rw [9], C [3], fx, fy, cx, cy, valid, 3 spare)
LANDMARK_WORDS = 8  # SSP_LANDMARK_WORDS: track id, X, Y, Z, n_views, rms, cos_parallax, index of the point in the newest frame
LANDMARK_OK, LANDMARK_FEW_VIEWS, LANDMARK_DEGENERATE, LANDMARK_BEHIND, LANDMARK_REPROJ = 0, 1, 2, 3, 4  # SSP_LANDMARK_*
CORR_WORDS = 8  # SSP_CORR_WORDS: fp64 words of a 3-D to 2-D correspondence (X, Y, Z, px, py, landmark row, valid, 0)
POSE_FLAG_ABSOLUTE = 4  # SSP_POSE_FLAG_ABSOLUTE: flag bit of a trajectory row rewritten from an absolute pose
POSE_FLAG_ADJUSTED = 8  # SSP_POSE_FLAG_ADJUSTED: flag bit of a trajectory row rewritten by the bundle adjustment
BA_INFO_WORDS = 8  # SSP_BA_INFO_WORDS: status, cost before, cost after, n_obs, rows used, accepted steps, refused V solves, lambda
BA_MAX_ITERATIONS = 16  # SSP_BA_MAX_ITERATIONS
BA_ADJUSTED, BA_NOTHING, BA_NO_STEP = 0, 1, 2  # info[0] of op_bundle_adjust


def load_library(path=None):
    """dlopen csrc/libssp_hip.so.  Without an explicit path (argument or SSP_HIP_LIB) the in-tree library is rebuilt
    first when it is missing or older than its sources (hipbuild.build_locked(): serialised across ranks by a file
    lock).  Raises if the library cannot be produced: there is no fallback."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    path = path or os.environ.get("SSP_HIP_LIB")  # SSP_HIP_LIB: A/B builds of the kernels (tools/)
    if path is None:
        path = _build.build_locked()
    if not os.path.exists(path):
        raise RuntimeError("libssp_hip.so not found at %s" % path)
    if os.environ.get("SSP_SKIP_ISA_VERIFY") != "1" and not _build.verified(path):  # the binary about to be loaded (e.g. shipped to the GPU box) keeps the register contract
        try:
            _build.verify_and_stamp(path)
        except _build.MissingTool as e:
            raise RuntimeError("%s - cannot check the accumulation-register contract of %s; set SSP_SKIP_ISA_VERIFY=1 to load it "
                               "unchecked" % (e, path)) from e
        except OSError:  # read-only tree: verified, not stamped
            _build.verify_binary(path)
    lib = C.CDLL(path)
    for name, (argtypes, restype) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:  # (an A/B library of an older revision, SSP_HIP_LIB, may lack the newer entry points)
            if os.environ.get("SSP_HIP_LIB") is None:
                raise
            continue
        fn.argtypes, fn.restype = argtypes, restype
    _lib = lib
    return lib


def set_deterministic(on=True):
    """Bit-reproducible accumulation for Engines created AFTER the call (also SSP_DETERMINISTIC=1): the fp64 accumulators take
    addends rounded to a fixed quantum, the fp32 scatter targets (descriptor / segmentation gradients, bias and first-layer weight
    gradients) go through 64-bit fixed-point shadows.  Two runs from the same state then agree bit for bit; the default mode keeps
    the plain floating-point atomics (run-to-run differences ~1e-6)."""
    _check(load_library().ssp_set_deterministic(1 if on else 0))


def get_deterministic():
    return bool(load_library().ssp_get_deterministic())


def clock_probe(ms=5.0):
    """Shader clock (MHz) the current device sustains under fp32 matrix-core load for ~`ms` milliseconds (ssp_clock_probe; blocking).
    None for an A/B library of an older revision that lacks the entry point."""
    import torch
    lib = load_library()
    if not hasattr(lib, "ssp_clock_probe"):
        return None
    out = C.c_double(0.0)
    _check(lib.ssp_clock_probe(float(ms), C.byref(out), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return float(out.value)


def build_id():
    """Build id of the LOADED library (sha256 of its sources at build time); equals hipbuild.source_id() for the in-tree library."""
    return load_library().ssp_build_id().decode()


def set_conv_algo(algo):
    """Process-wide default (new Engines, handle-less operators): 0 = direct implicit GEMM, 1 = Winograd F(2x2,3x3)
    for the eligible 3x3 convolutions (default).  `Engine.set_conv_algo` changes one engine."""
    _check(load_library().ssp_set_conv_algo(int(algo)))


def _check(rc):
    if rc != 0:
        raise RuntimeError("libssp_hip: %s (code %d)" % (load_library().ssp_last_error().decode(), rc))


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _need_gpu(t, name):
    if not t.is_cuda:
        raise RuntimeError("%s must live on a HIP device: the MI355X path has no CPU fallback" % name)
    if not t.is_contiguous():
        raise RuntimeError("%s must be contiguous" % name)


# ---- argument checks of the operator wrappers (one copy of each) ----
def _shape_text(shape):
    return "[%s]" % ", ".join("." if w is None else str(w) if not isinstance(w, tuple) else
                              (">= %d" % w[0] if w[1] is None else "%d..%d" % w) for w in shape)


def _tensor(t, name, dtype, shape, hint=None):
    """One device tensor argument.  _need_gpu first: a CPU or strided tensor is its RuntimeError.  Anything else that is wrong is
    a ValueError naming the argument, the dtype and the shape.  shape: one entry per dimension, an int, None (any) or a (lo, hi)
    range (hi None: open); dtype None: any.  hint: where the sizes come from, for the message.  Returns t."""
    _need_gpu(t, name)
    if t.shape == shape and t.dtype == dtype:  # an exact spec: one compare
        return t
    ok = (dtype is None or t.dtype == dtype) and t.dim() == len(shape)
    if ok:
        for n, w in zip(t.shape, shape):
            if w is None or n == w:
                continue
            if w.__class__ is not tuple or n < w[0] or (w[1] is not None and n > w[1]):
                ok = False
                break
    if not ok:
        raise ValueError("%s must be %s %s%s (got %s %s)" % (name, "a tensor" if dtype is None else str(dtype)[6:], _shape_text(shape),
                                                            " (%s)" % hint if hint else "", str(t.dtype)[6:], list(t.shape)))
    return t


def _count(t, name, n, dtype=torch.int32, like=None, hint=None):
    """A tensor held by its length, not its shape: a per-pair vector may be [P] or [P, 1], a matrix per pair [P, 3, 3] or [P, 9]
    (`like`: the shape the message shows).  Device and contiguity as in _tensor.  Returns t."""
    _need_gpu(t, name)
    if t.dtype != dtype or t.numel() != n:
        raise ValueError("%s must be %s %s%s (got %s %s)" % (name, str(dtype)[6:], list(like or (n,)), " (%s)" % hint if hint else "",
                                                            str(t.dtype)[6:], list(t.shape)))
    return t


def _pair_inputs(pts1, pts2, match, n_match, pair_stride=1, pt_stride=(2, None), what="", S=None, single=False, points=True):
    """The matches of P pairs, as every pair operator takes them; returns (P, cap, match as [P, cap, 3]).  match float32 [P, cap, 3]
    with 1 <= cap <= MATCH_MAX_POINTS, n_match int32 of P entries and, with `points`, pts1 / pts2 float64 [>= (P-1)*pair_stride+1,
    cap, pt_stride] with one pt_stride (an int or a range).  what: the suffix of both names ("_cur"); S: the P the caller already
    holds, as (P, where it comes from); single: a [cap, 3] match is one pair."""
    name, m = "match" + what, match
    if single:
        _need_gpu(match, name)
        m = match[None] if match.dim() == 2 else match
    S, hint = S or (None, "[cap, 3] for one pair" if single else None)
    _tensor(m, name, torch.float32, (S, None, 3), hint)
    P, cap = m.shape[0], m.shape[1]
    if not 1 <= cap <= MATCH_MAX_POINTS:
        raise ValueError("1 <= cap <= %d matches per pair (got %d)" % (MATCH_MAX_POINTS, cap))
    if points:
        rows = ((P - 1) * pair_stride + 1, None)
        _tensor(pts1, "pts1", torch.float64, (rows, cap, pt_stride), "(P-1)*pair_stride+1 rows or more, P and cap from match")
        _tensor(pts2, "pts2", torch.float64, (rows, cap, pts1.shape[2]), "as pts1; P and cap from match, at pair_stride")
    _count(n_match, "n_match" + what, P, hint="one per pair of " + name)
    return P, cap, m


def _model_inputs(geometry, key, what, P, cap):
    """(matrix, mask, n_inliers, status) of a RANSAC dict, checked: all four are held by their lengths."""
    for k in (key, "mask", "n_inliers", "status"):
        if k not in geometry:
            raise ValueError("%s must be the dict of a RANSAC operator (no %r)" % (what, k))
    return (_count(geometry[key], "%s[%r]" % (what, key), P * 9, torch.float64, (P, 3, 3)),
            _count(geometry["mask"], "%s['mask']" % what, P * cap, torch.uint8, (P, cap)),
            _count(geometry["n_inliers"], "%s['n_inliers']" % what, P), _count(geometry["status"], "%s['status']" % what, P))


def _intrinsics(t, name, rows, n):
    """Camera intrinsics float64 [1, *rows] (shared) or [n, *rows], rows = (2, 4) or (4,) of (fx, fy, cx, cy); returns the count."""
    _tensor(t, name, torch.float64, (None,) + rows, "rows (fx, fy, cx, cy)")
    if t.shape[0] not in (1, n):
        raise ValueError("%s must be float64 %s or %s rows (fx, fy, cx, cy)" % (name, [1] + list(rows), [n] + list(rows)))
    return int(t.shape[0])


def _chain_arrays(state, table, S):
    """The pose chain of S sequences: state float64 [S, POSE_STATE_WORDS] held by its length (one sequence may be flat), table
    float64 [S, capacity, POSE_ROW_WORDS] or [capacity, .] for one sequence; returns capacity."""
    _count(state, "state", S * POSE_STATE_WORDS, torch.float64, (S, POSE_STATE_WORDS))
    _need_gpu(table, "table")
    if (table.dtype != torch.float64 or table.dim() not in (2, 3) or table.shape[-1] != POSE_ROW_WORDS
            or table.numel() != S * table.shape[-2] * POSE_ROW_WORDS):
        raise ValueError("table must be float64 [%d, capacity, %d] (pose_table)" % (S, POSE_ROW_WORDS))
    return int(table.shape[-2])


_SHAPES = {}


def _shapes(spec, dims):
    """{key: shape} of a buffer family at sizes `dims`.  spec: (symbols, {key: (dtype, shape in those symbols or constants)}), the one
    statement of the family's layout; dims: a size per symbol, in their order.  A process meets a handful of sizes: each is built once."""
    shapes = _SHAPES.get((id(spec), dims))
    if shapes is None:
        if len(_SHAPES) >= 256:
            _SHAPES.clear()
        size = dict(zip(spec[0], dims))
        shapes = _SHAPES[id(spec), dims] = {k: tuple(size.get(n, n) for n in shape) for k, (_, shape) in spec[1].items()}
    return shapes


def _alloc(spec, dims, device, keys=None, zero=True):
    """The tensors `keys` (default: all) of a buffer family at sizes `dims`, zeroed unless told otherwise."""
    new, shapes = torch.zeros if zero else torch.empty, _shapes(spec, dims)
    return {k: new(*shapes[k], dtype=spec[1][k][0], device=device) for k in (keys or spec[1])}


def _check_family(d, what, spec, dims, keys, source):
    """The members `keys` of the dict argument `what` against the family that its allocator `source` allocates from."""
    shapes = _shapes(spec, dims)
    for k in keys:
        if k not in d:
            raise ValueError("%s must be the dict of %s (no %r)" % (what, source, k))
        _tensor(d[k], "%s[%r]" % (what, k), spec[1][k][0], shapes[k], source)
    return d


def scaled_homographies(hn, height, width):
    """T^-1 @ H @ T with T = [[2/width, 0, -1], [0, 2/height, -1], [0, 0, 1]] for a batch of normalised homographies,
    computed on the HOST with the reference's own fp32 op sequence (`torch.inverse(trans) @ H @ trans`, per matrix:
    utils/utils.py:297-300 homography_scaling_torch, utils/homographies.py:270-276 scale_homography_torch), so that the
    matrix - and with it every integer index the device derives from it - is bit-identical to the reference's.
    (height, width) = (H, W) for pixel coordinates (warpLabels), (H/8, W/8) for cell coordinates (sparse-loss matches).
    hn: [B,3,3] on any device (a device tensor costs one small D2H copy); returns a CPU float32 tensor [B,3,3]."""
    h = hn.detach().to("cpu", torch.float32).reshape(-1, 3, 3)
    trans = torch.tensor([[2.0 / width, 0.0, -1.0], [0.0, 2.0 / height, -1.0], [0.0, 0.0, 1.0]])
    inv = torch.inverse(trans)
    return torch.stack([inv @ m @ trans for m in h]).contiguous()


# ------------------------------------------------------------------------------------------------
# parameter layout == reference state_dict layout
# ------------------------------------------------------------------------------------------------
_ENC = [("inc.conv.conv.0", "inc.conv.conv.1", 1, 64, 3), ("inc.conv.conv.3", "inc.conv.conv.4", 64, 64, 3),
        ("down1.mpconv.1.conv.0", "down1.mpconv.1.conv.1", 64, 64, 3),
        ("down1.mpconv.1.conv.3", "down1.mpconv.1.conv.4", 64, 64, 3),
        ("down2.mpconv.1.conv.0", "down2.mpconv.1.conv.1", 64, 128, 3),
        ("down2.mpconv.1.conv.3", "down2.mpconv.1.conv.4", 128, 128, 3),
        ("down3.mpconv.1.conv.0", "down3.mpconv.1.conv.1", 128, 128, 3),
        ("down3.mpconv.1.conv.3", "down3.mpconv.1.conv.4", 128, 128, 3)]
_HEADS = [("convPa", "bnPa", 128, 256, 3), ("convPb", "bnPb", 256, 65, 1), ("convDa", "bnDa", 128, 256, 3),
          ("convDb", "bnDb", 256, 256, 1)]


def layer_table(arch, n_classes=133):
    t = _ENC + _HEADS
    if arch == "SuperPointNet_gauss2_ssmall":
        t = t + [("convDS", "bnS1", 128, 256, 3), ("convSout", None, 256, n_classes, 1)]
    elif arch != "SuperPointNet_gauss2":
        raise KeyError(arch)
    return t


def param_layout(arch, n_classes=133):
    """[(state_dict key, shape, offset)] of the flat parameter vector, net.parameters() order."""
    out, off = [], 0
    for conv, bn, cin, cout, k in layer_table(arch, n_classes):
        for key, shape in ((conv + ".weight", (cout, cin, k, k)), (conv + ".bias", (cout,))):
            out.append((key, shape, off))
            off += int(np.prod(shape))
        if bn is not None:
            for key in (bn + ".weight", bn + ".bias"):
                out.append((key, (cout,), off))
                off += cout
    return out, off


def bn_layout(arch, n_classes=133):
    """[(bn key prefix, C, channel offset)] in layer order."""
    out, off = [], 0
    for conv, bn, cin, cout, k in layer_table(arch, n_classes):
        if bn is not None:
            out.append((bn, cout, off))
            off += cout
    return out, off


class Engine:
    """One libssp handle plus its torch-owned device buffers (one per GPU / stream)."""

    def __init__(self, arch, max_batch, height, width, device, n_classes=133, n_match=1000, n_non=100,
                 with_grad=True, dense_loss=False):
        self.lib = load_library()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("Engine needs a HIP device (got %s): no CPU fallback exists" % self.device)
        self.arch, self.n_classes = arch, n_classes
        self.max_batch, self.height, self.width = max_batch, height, width
        self.n_match, self.n_non = n_match, n_non
        self.dense_loss = bool(dense_loss)
        cfg = SspConfig(ARCHS[arch], n_classes, max_batch, height, width, n_match, n_non, int(self.dense_loss))
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            _check(self.lib.ssp_create(C.byref(cfg), C.byref(h)))
        self.h = h
        self.layout, self.n_params = param_layout(arch, n_classes)
        self.bns, self.n_bn_ch = bn_layout(arch, n_classes)
        assert self.n_params == self.lib.ssp_param_count(h), "parameter layout mismatch with the library"
        assert self.n_bn_ch == self.lib.ssp_bn_channel_count(h)
        f32 = dict(dtype=torch.float32, device=self.device)
        self.params = torch.zeros(self.n_params + 3, **f32)
        self.params[self.n_params:] = torch.tensor([1.0, 2.0, 1.0])  # MultiTaskLoss.eta init
        self.grads = torch.zeros(self.n_params + 3, **f32) if with_grad else None
        self.adam_m = torch.zeros(self.n_params + 3, **f32) if with_grad else None
        self.adam_v = torch.zeros(self.n_params + 3, **f32) if with_grad else None
        self.bn_running = torch.cat([torch.zeros(self.n_bn_ch, **f32), torch.ones(self.n_bn_ch, **f32)])
        self.nbt = torch.zeros(len(self.bns), dtype=torch.int64, device=self.device)
        self.ws_bytes = self.lib.ssp_workspace_bytes(h)
        self._tap_arena = None   # debug_backward_taps
        self.workspace = torch.empty(self.ws_bytes, dtype=torch.uint8, device=self.device)
        self.scalars = torch.zeros(N_SCALARS, **f32)
        self.adam_t = 0
        self.bind()

    def bind(self):
        b = SspBuffers(_ptr(self.params), _ptr(self.grads), _ptr(self.adam_m), _ptr(self.adam_v),
                       _ptr(self.bn_running), _ptr(self.nbt), _ptr(self.workspace), self.ws_bytes)
        with torch.cuda.device(self.device):
            _check(self.lib.ssp_bind(self.h, C.byref(b), _stream()))

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.lib.ssp_destroy(self.h)
                self.h = None
        except Exception:
            pass

    # ---- state ----
    def load_state_dict(self, sd):
        for key, shape, off in self.layout:
            v = torch.as_tensor(np.asarray(sd[key]) if not torch.is_tensor(sd[key]) else sd[key])
            self.params[off:off + v.numel()] = v.reshape(-1).to(self.device, torch.float32)
        for i, (bn, c, off) in enumerate(self.bns):
            for j, name in enumerate(("running_mean", "running_var")):
                k = bn + "." + name
                if k in sd:
                    v = torch.as_tensor(np.asarray(sd[k]) if not torch.is_tensor(sd[k]) else sd[k])
                    self.bn_running[j * self.n_bn_ch + off:j * self.n_bn_ch + off + c] = v.to(self.device, torch.float32)
            k = bn + ".num_batches_tracked"
            if k in sd:
                self.nbt[i] = int(sd[k])

    def state_dict(self):
        out = OrderedDict()
        bn_iter = {bn: (i, c, off) for i, (bn, c, off) in enumerate(self.bns)}
        for key, shape, off in self.layout:
            n = int(np.prod(shape))
            out[key] = self.params[off:off + n].view(shape).clone()
            prefix = key.rsplit(".", 1)[0]
            if key.endswith(".bias") and prefix in bn_iter:
                i, c, boff = bn_iter[prefix]
                out[prefix + ".running_mean"] = self.bn_running[boff:boff + c].clone()
                out[prefix + ".running_var"] = self.bn_running[self.n_bn_ch + boff:self.n_bn_ch + boff + c].clone()
                out[prefix + ".num_batches_tracked"] = self.nbt[i].clone()
        return out

    def grad_dict(self):
        out = OrderedDict()
        for key, shape, off in self.layout:
            out[key] = self.grads[off:off + int(np.prod(shape))].view(shape)
        out["eta"] = self.grads[self.n_params:]
        return out

    @property
    def eta(self):
        return self.params[self.n_params:]

    # ---- compute ----
    def forward(self, x, slot=0, train=True, want=("semi", "desc")):
        _need_gpu(x, "x")
        n, c, hh, ww = x.shape
        assert c == 1 and x.dtype == torch.float32
        f32 = dict(dtype=torch.float32, device=self.device)
        out = {}
        semi = torch.empty(n, 65, hh // 8, ww // 8, **f32) if "semi" in want else None
        desc = torch.empty(n, 256, hh // 8, ww // 8, **f32) if "desc" in want else None
        sem = torch.empty(n, self.n_classes, hh, ww, **f32) if "sem" in want else None
        if not hasattr(self, "_x"):
            self._x = [None, None]
        self._x[slot] = x  # the first-layer weight gradient re-reads the image in backward: keep it alive
        with torch.cuda.device(self.device):
            _check(self.lib.ssp_forward(self.h, slot, _ptr(x), n, hh, ww, int(bool(train)), _ptr(semi), _ptr(desc),
                                        _ptr(sem), _stream()))
        if semi is not None:
            out["semi"] = semi
        if desc is not None:
            out["desc"] = desc
        if sem is not None:
            out["sem"] = sem
        return out

    def backward(self, slot, dsemi=None, ddesc=None, dsem=None):
        for t, nm in ((dsemi, "dsemi"), (ddesc, "ddesc"), (dsem, "dsem")):
            if t is not None:
                _need_gpu(t, nm)
        with torch.cuda.device(self.device):
            _check(self.lib.ssp_backward(self.h, slot, _ptr(dsemi), _ptr(ddesc), _ptr(dsem), _stream()))

    def zero_grad(self):
        with torch.cuda.device(self.device):
            _check(self.lib.ssp_zero_grad(self.h, _stream()))

    def adam_step(self, lr, grad_scale=None):
        """Fused Adam over the flat vector; grad_scale (e.g. 1 / world_size after an all-reduce SUM) scales the
        gradient inside the kernel without touching `grads`."""
        self.adam_t += 1
        with torch.cuda.device(self.device):
            if grad_scale is None:
                _check(self.lib.ssp_adam_step(self.h, float(lr), self.adam_t, _stream()))
            else:
                _check(self.lib.ssp_adam_step_scaled(self.h, float(lr), self.adam_t, float(grad_scale), _stream()))

    def set_conv_algo(self, algo):
        _check(self.lib.ssp_handle_set_conv_algo(self.h, int(algo)))

    @property
    def early_offset(self):
        """First element of the gradient bucket that is final after phase 1 of a split pair step."""
        return int(self.lib.ssp_grad_early_offset(self.h))

    def sample_indices(self, homographies, seed, cell_homographies=None):
        """Device sampler of the sparse-loss indices.  cell_homographies ([B,3,3], host or device): the reference's
        scale_homography_torch matrices (`scaled_homographies(H, Hc, Wc)`): the sampled matches are then exact
        correspondences of the reference (bit-identical rounding); without them T^-1 H T is derived on the device."""
        _need_gpu(homographies, "homographies")
        B = homographies.shape[0]
        i32 = dict(dtype=torch.int32, device=self.device)
        ma = torch.empty(B, self.n_match, **i32)
        mb = torch.empty(B, self.n_match, **i32)
        nm = torch.empty(B, self.n_match * self.n_non, **i32)
        with torch.cuda.device(self.device):
            if cell_homographies is not None:
                hc = cell_homographies.to(self.device, torch.float32).contiguous()
                assert tuple(hc.shape) == (B, 3, 3)
                self._keep_hc = hc
                _check(self.lib.ssp_sample_indices_cell(self.h, _ptr(hc), B, int(seed), _ptr(ma), _ptr(mb), _ptr(nm), _stream()))
            else:
                _check(self.lib.ssp_sample_indices(self.h, _ptr(homographies), B, int(seed), _ptr(ma), _ptr(mb), _ptr(nm),
                                                   _stream()))
        return ma, mb, nm

    def pair_step(self, sample, indices=None, seed=0, train=True, lambda_loss=1.0, lamda_d=1.0, multi_task=True,
                  gaussian=True, dense=None, phase=0, graph=False, sparse_method="2d", sparse_dist="cos"):
        """`sample`: dict of device tensors with the reference's keys (Train_model_heatmap_all.py:212-251).
        indices: (match_a, match_b, nonmatch_b) int32 device tensors or None (device sampler with `seed`).
        sparse_method / sparse_dist: model.sparse_loss.params.method / dist (sparse_loss.py:76-77): "2d" = bilinear grid_sample of the
        matches (every shipped config), anything else = index_select at the cell; "cos" = hinges on the dot product, anything else =
        the euclidean forms (pixelwise_contrastive_loss.py:140,185-210,247-258).
        dense: None (sparse descriptor loss) or the model.dense_loss.params dict (dense descriptor loss,
        utils/utils.py:779-893; keys lamda_d (default 250: the shipped `lambda_d` spelling is ignored by the reference
        too) and descriptor_dist (4)); needs an Engine created with dense_loss=True.
        phase: 0 whole step; 1 / 2 = the two halves of ssp_pair_step_phase (data-parallel overlap; call 2 with the
        same arguments).  graph=True replays the step as a hipGraph (ssp_pair_step_graph; needs a non-default
        current stream; the device sampler then fills persistent index buffers inside the graph).
        A sample WITHOUT "warped_img" is the single-view step of `data.warped_pair.enable: false`
        (Train_model_heatmap_all.py:207,237-262,330-332; configs/magicpoint_shapes_pair.yaml): one forward, detector
        (+ segmentation) loss of the image only; lambda_loss must be 0 (the reference asserts "need a pair of images").
        Returns the device tensor of SSP_N_SCALARS floats (no host sync)."""
        img = sample["image"]
        B, c1, H, W = img.shape
        single = sample.get("warped_img") is None
        if single and lambda_loss > 0:
            raise AssertionError("need a pair of images")  # Train_model_heatmap_all.py:343
        lab = sample["labels_2D_gaussian"] if gaussian else sample["labels_2D"]
        if single:
            imgw = labw = maskw = None
            req = [img, lab, sample["valid_mask"]]
        else:
            imgw, maskw = sample["warped_img"], sample["warped_valid_mask"]
            labw = sample["warped_labels_gaussian"] if gaussian else sample["warped_labels"]
            req = [img, imgw, lab, labw, sample["valid_mask"], maskw]
        for t in req:
            _need_gpu(t, "sample tensor")
            if t.dtype != torch.float32 or tuple(t.shape) != (B, 1, H, W):
                raise ValueError("pair-step image / label / mask tensors must be float32 [B,1,H,W] = %s, got %s %s"
                                 % ((B, 1, H, W), t.dtype, tuple(t.shape)))
        if (H, W) != (self.height, self.width) or B > self.max_batch:
            raise ValueError("pair step [%d,1,%d,%d] does not match the engine (%d x %dx%d)"
                             % (B, H, W, self.max_batch, self.height, self.width))
        Hm = None
        if not single:
            Hm = sample["homographies"].to(torch.float32)
            if not Hm.is_contiguous():
                Hm = Hm.contiguous()
            _need_gpu(Hm, "homographies")
            if tuple(Hm.shape) != (B, 3, 3):
                raise ValueError("homographies must be [B,3,3]")
        if dense is not None and not self.dense_loss:
            raise RuntimeError("create the Engine with dense_loss=True to use the dense descriptor loss")
        sample_in_graph = False
        if lambda_loss > 0 and indices is None and dense is None:
            if graph:  # persistent buffers: the captured sampler writes them
                if getattr(self, "_graph_idx", None) is None or self._graph_idx[0].shape[0] != B:
                    i32 = dict(dtype=torch.int32, device=self.device)
                    self._graph_idx = (torch.zeros(B, self.n_match, **i32), torch.zeros(B, self.n_match, **i32),
                                       torch.zeros(B, self.n_match * self.n_non, **i32))
                indices = self._graph_idx
                sample_in_graph = True
            elif phase != 2:
                indices = self._last_idx = self.sample_indices(Hm, seed, sample.get("cell_homographies"))
            else:
                indices = self._last_idx
        if indices is not None:
            ma, mb, nm = indices
            for t, shp in ((ma, (B, self.n_match)), (mb, (B, self.n_match)), (nm, (B, self.n_match * self.n_non))):
                _need_gpu(t, "sparse-loss indices")
                if t.dtype != torch.int32 or tuple(t.shape) != shp:
                    raise ValueError("sparse-loss indices must be int32 %s, got %s %s" % (shp, t.dtype, tuple(t.shape)))
        else:
            ma = mb = nm = None
        sem = semw = None
        if self.arch.endswith("ssmall"):
            sem, semw = sample.get("semantic"), (None if single else sample.get("warped_sem"))
            for t in ((sem,) if single else (sem, semw)):
                if t is None:
                    raise KeyError("the ssmall model needs sample['semantic'] and sample['warped_sem']")
                _need_gpu(t, "semantic labels")
                if t.dtype != torch.int64 or tuple(t.shape) != (B, H, W):
                    raise ValueError("semantic labels must be int64 [B,H,W] = %s, got %s %s"
                                     % ((B, H, W), t.dtype, tuple(t.shape)))
            if getattr(self, "check_label_range", False):  # one host sync: off by default (torch raises here too)
                for t in ((sem,) if single else (sem, semw)):
                    if int(t.min()) < 0 or int(t.max()) > self.n_classes:
                        raise ValueError("semantic label outside [0, %d]" % self.n_classes)
        inp = SspPairInputs(B, _ptr(img), _ptr(imgw), _ptr(lab), _ptr(labw), _ptr(sample["valid_mask"]),
                            _ptr(maskw), _ptr(Hm), _ptr(sem), _ptr(semw), _ptr(ma), _ptr(mb),
                            _ptr(nm), int(seed) & 0xFFFFFFFFFFFFFFFF, float(lambda_loss), float(lamda_d),
                            int(bool(multi_task)), int(bool(train)), int(dense is not None),
                            float((dense or {}).get("lamda_d", 250.0)), float((dense or {}).get("descriptor_dist", 4.0)),
                            None, int(sparse_method != "2d"), int(sparse_dist != "cos"))
        hcell = sample.get("cell_homographies")
        if hcell is not None:  # the reference's own cell-space matrices (scaled_homographies): exact match indices
            _need_gpu(hcell, "cell_homographies")
            if hcell.dtype != torch.float32 or tuple(hcell.shape) != (B, 3, 3):
                raise ValueError("cell_homographies must be float32 [B,3,3]")
            inp.cell_homographies_dev = hcell.data_ptr()
        self._keep = (req, Hm, indices, sem, semw, hcell)  # keep alive until the stream has consumed them
        with torch.cuda.device(self.device):
            if graph:
                _check(self.lib.ssp_pair_step_graph(self.h, C.byref(inp), _ptr(self.scalars), int(phase),
                                                    int(sample_in_graph), _stream()))
            elif phase == 0:
                _check(self.lib.ssp_pair_step(self.h, C.byref(inp), _ptr(self.scalars), _stream()))
            else:
                _check(self.lib.ssp_pair_step_phase(self.h, C.byref(inp), _ptr(self.scalars), int(phase), _stream()))
        return self.scalars

    def export_points(self, views, masks, unwarp_h, conf_thresh=0.015, nms_dist=4, top_k=600, subpixel=True,
                      border_remove=4, want_heatmap=False):
        """Homography-adaptation export of 1 or 2 images (export.py:296-309).  views/masks: lists of [n,1,H,W] (or
        [n,H,W]) device tensors -- one BatchNorm batch each; unwarp_h: list of [n,3,3] (sample["homographies"]).
        Returns a list of dicts {"pts": device [count,5] rows (x, y, conf, sx, sy), "count": device int32,
        "heatmap": [H,W] or None}; no host synchronisation happens here."""
        k = len(views)
        n, hh, ww = views[0].shape[0], views[0].shape[-2], views[0].shape[-1]
        p = SspExportParams(n, hh, ww, float(np.float32(conf_thresh)), int(nms_dist), int(border_remove),
                            int(top_k or 0), int(bool(subpixel)))
        for t in list(views) + list(masks) + list(unwarp_h):
            _need_gpu(t, "export tensor")
            assert t.dtype == torch.float32 and t.shape[0] == n
        wsb = self.lib.ssp_export_workspace_bytes(C.byref(p))
        cap = self.lib.ssp_export_max_points(C.byref(p))
        if wsb == 0 or cap < 0:
            _check(-1)
        key = (n, hh, ww, int(nms_dist), int(top_k or 0))
        if getattr(self, "_export_ws_key", None) != key:
            self._export_ws = [torch.empty(wsb, dtype=torch.uint8, device=self.device) for _ in range(2)]
            self._export_ws_key = key
        f32 = dict(dtype=torch.float32, device=self.device)
        pts = [torch.empty(max(cap, 1), 5, **f32) for _ in range(k)]
        cnt = [torch.zeros(1, dtype=torch.int32, device=self.device) for _ in range(k)]
        hm = [torch.empty(hh, ww, **f32) if want_heatmap else None for _ in range(k)]
        arr = lambda ts: (C.c_void_p * 2)(*[t.data_ptr() if t is not None else None for t in ts])  # noqa: E731
        self._keep_export = (views, masks, unwarp_h)
        with torch.cuda.device(self.device):
            _check(self.lib.ssp_export_points(self.h, C.byref(p), k, arr(views), arr(masks), arr(unwarp_h),
                                              arr(self._export_ws[:k]), arr(hm), arr(pts), arr(cnt), _stream()))
        return [{"pts": pts[j], "count": cnt[j], "heatmap": hm[j]} for j in range(k)]

    def describe_points(self, slot, n, conf_thresh=0.015, nms_dist=4, subpixel=True, top_k=0, border_remove=4, classes=False):
        """Keypoints + sparse descriptors of the first n images of the last EVAL forward in `slot` (Val_model_heatmap's
        run / heatmap_to_pts / soft_argmax_points / desc_to_sparseDesc, export.py:126-142).  Returns device tensors
        {"pts": [n,cap,5] rows (x, y, conf, sx, sy), "count": [n] int32, "desc": [n,cap,256]}; no host synchronisation.
        classes=True adds "cls": uint8 [n,cap], the segmentation head's class at each keypoint (point_classes)."""
        hh, ww = self.height, self.width
        x = getattr(self, "_x", [None, None])[slot]
        if x is not None:
            hh, ww = x.shape[-2], x.shape[-1]
        p = SspExportParams(1, hh, ww, float(np.float32(conf_thresh)), int(nms_dist), int(border_remove), int(top_k or 0),
                            int(bool(subpixel)))
        wsb = self.lib.ssp_describe_workspace_bytes(C.byref(p), int(n))
        cap = self.lib.ssp_export_max_points(C.byref(p))
        if wsb == 0 or cap < 0:
            _check(-1)
        if getattr(self, "_describe_ws", None) is None or self._describe_ws.numel() < wsb:
            self._describe_ws = torch.empty(wsb, dtype=torch.uint8, device=self.device)
        f32 = dict(dtype=torch.float32, device=self.device)
        pts = torch.empty(n, cap, 5, **f32)
        cnt = torch.zeros(n, dtype=torch.int32, device=self.device)
        desc = torch.empty(n, cap, 256, **f32)
        with torch.cuda.device(self.device):
            _check(self.lib.ssp_describe_points(self.h, int(slot), C.byref(p), int(n), _ptr(self._describe_ws), _ptr(pts),
                                                _ptr(cnt), _ptr(desc), _stream()))
        if classes:
            return {"pts": pts, "count": cnt, "desc": desc, "cls": self.point_classes(slot, pts, cnt)}
        return {"pts": pts, "count": cnt, "desc": desc}

    def point_classes(self, slot, pts, count):
        """The class the segmentation head gives each keypoint, from the logits the last forward / pair step left in `slot`
        (ssp_point_classes; see op_point_classes): pts float32 [n,cap,>=2] rows starting with the integer pixel (x, y), count
        int32 [n] -> uint8 [n,cap], CLASS_NONE in the rows past each count.  No host synchronisation."""
        pts, count = _point_class_args(pts, count)
        n, cap, stride = pts.shape
        cls = torch.empty(n, cap, dtype=torch.uint8, device=self.device)
        if cap == 0:
            return cls
        with torch.cuda.device(self.device):
            _check(self.lib.ssp_point_classes(self.h, int(slot), n, _ptr(pts), stride, _ptr(count), cap, _ptr(cls), _stream()))
        return cls

    def detector_heatmap(self, slot, n, hh, ww):
        """flattenDetection of the detector logits left in `slot` by the last forward / pair step -> [n,1,hh,ww]."""
        out = torch.empty(n, 1, hh, ww, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _check(self.lib.ssp_detector_heatmap(self.h, slot, _ptr(out), _stream()))
        return out

    def sem_predict(self, slot, n, hh, ww, labels=None, want_pred=True, confusion=None):
        """Class map and / or confusion matrix of the segmentation logits left in `slot` by the last forward / pair step (fused
        upsample + argmax + counting, ssp_sem_predict; see op_sem_predict) -> (pred uint8 [n,hh,ww] | None, confusion | None)."""
        labels, pred, confusion = _sem_predict_buffers(n, hh, ww, self.n_classes, self.device, labels, want_pred, confusion)
        with torch.cuda.device(self.device):
            _check(self.lib.ssp_sem_predict(self.h, int(slot), _ptr(labels), _ptr(pred), _ptr(confusion), _stream()))
        return pred, confusion

    def debug_buffer(self, slot, name, shape, dtype=torch.float32):
        """Test hook: copy of an internal NHWC buffer as a torch tensor of `shape` (dtype bfloat16 for the activation /
        gradient tensors of the bf16 path)."""
        p, n = C.c_void_p(), C.c_size_t()
        _check(self.lib.ssp_debug_buffer(self.h, slot, name.encode(), C.byref(p), C.byref(n)))
        numel = int(np.prod(shape))
        es = 2 if dtype == torch.bfloat16 else 4
        base = self.workspace.data_ptr()
        off = p.value - base
        assert 0 <= off and off + numel * es <= self.ws_bytes
        return self.workspace[off:off + numel * es].view(dtype).view(*shape).clone()

    def debug_backward_taps(self, layers):
        """Test hook: switch the backward taps on for the layers in `layers` (iterable of layer indices; 8 = the three 3x3 heads)
        with a fresh device arena owned by this engine, or off (`layers` empty / None)."""
        mask = 0
        for l in layers or ():
            mask |= 1 << int(l)
        self._tap_arena = None
        if mask == 0:
            _check(self.lib.ssp_debug_backward_taps(self.h, None, 0, 0))
            return
        n = int(self.lib.ssp_debug_backward_tap_floats(self.h, mask))
        self._tap_arena = torch.zeros(n, dtype=torch.float32, device=self.device)
        _check(self.lib.ssp_debug_backward_taps(self.h, _ptr(self._tap_arena), n, mask))

    def backward_route(self, layer):
        """Route record of `layer` in the last backward pass (include/ssp_hip.h, ssp_debug_backward_tap)."""
        r = C.c_uint()
        _check(self.lib.ssp_debug_backward_tap(self.h, 0, layer, 0, None, None, C.byref(r)))
        return r.value

    def backward_tap(self, slot, layer, which, shape, dtype=torch.float32):
        """Test hook: host copy of one backward tap (which: 0 = dOut, 1 = dY) of the last step as a tensor of `shape` (NHWC, the
        step's batch: a prefix of the tap's max_batch slice).  dtype bfloat16 for the bf16 taps of the bf16 path (the slice's
        bytes viewed as bf16, as debug_buffer does)."""
        off, n = C.c_size_t(), C.c_size_t()
        _check(self.lib.ssp_debug_backward_tap(self.h, slot, layer, which, C.byref(off), C.byref(n), None))
        numel = int(np.prod(shape))
        es = 2 if dtype == torch.bfloat16 else 4
        assert self._tap_arena is not None and 0 < numel * es <= n.value * 4, (layer, which, numel, n.value)
        return self._tap_arena[off.value:off.value + n.value].view(dtype)[:numel].view(*shape).cpu()

    def profile_enable(self, family):
        _check(self.lib.ssp_profile_enable(self.h, PROF[family] if isinstance(family, str) else int(family)))

    def profile_pause(self, paused):
        if hasattr(self.lib, "ssp_profile_pause"):
            _check(self.lib.ssp_profile_pause(self.h, int(bool(paused))))

    def profile_read(self):
        ms, n, fl, by = C.c_double(), C.c_int64(), C.c_double(), C.c_double()
        _check(self.lib.ssp_profile_read(self.h, C.byref(ms), C.byref(n), C.byref(fl), C.byref(by)))
        ex = C.c_double()
        _check(self.lib.ssp_profile_read_executed(self.h, C.byref(ex)))
        return {"ms": ms.value, "launches": n.value, "flops": fl.value, "bytes": by.value, "exec_flops": ex.value}

    def profile_read_kernels(self):
        """Per-kernel split of profile_read(): {kernel name: {ms, launches, flops, exec_flops, bytes}} (launched kernels only)."""
        out = {}
        if not hasattr(self.lib, "ssp_profile_read_kernel"):  # (an A/B library of an older revision, SSP_HIP_LIB)
            return out
        for k, name in enumerate(PROF_KERNELS):
            ms, n, fl, ex, by = C.c_double(), C.c_int64(), C.c_double(), C.c_double(), C.c_double()
            _check(self.lib.ssp_profile_read_kernel(self.h, k, C.byref(ms), C.byref(n), C.byref(fl), C.byref(ex), C.byref(by)))
            if n.value > 0:
                out[name] = {"ms": ms.value, "launches": n.value, "flops": fl.value, "exec_flops": ex.value, "bytes": by.value}
        return out


# ---- optimizer state in torch.optim.Adam's wire format ----
def optimizer_state_dict(eng, lr):
    """state_dict() of the reference's optimizer, torch.optim.Adam(list(net.parameters()) + [eta], lr, betas=(0.9, 0.999))
    (Train_model_frontend_all.py:183-198), filled from the engine's flat m / v vectors."""
    state, idx = {}, 0
    step = torch.tensor(float(eng.adam_t))
    entries = [(shape, off) for _, shape, off in eng.layout] + [((3,), eng.n_params)]
    for shape, off in entries:
        n = int(np.prod(shape))
        if eng.adam_t > 0:
            state[idx] = {"step": step.clone(), "exp_avg": eng.adam_m[off:off + n].view(shape).detach().cpu().clone(),
                          "exp_avg_sq": eng.adam_v[off:off + n].view(shape).detach().cpu().clone()}
        idx += 1
    group = {"lr": float(lr), "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 0, "amsgrad": False, "maximize": False,
             "foreach": None, "capturable": False, "differentiable": False, "fused": None, "decoupled_weight_decay": False,
             "params": list(range(idx))}
    return {"state": state, "param_groups": [group]}


def load_optimizer_state(eng, osd, eta=None):
    """Inverse of optimizer_state_dict (also accepts round 1's {"adam_m", "adam_v", "step"} form); eta: 3 floats."""
    if osd is not None and "state" in osd:
        entries = [(shape, off) for _, shape, off in eng.layout] + [((3,), eng.n_params)]
        steps = []
        for idx, (shape, off) in enumerate(entries):
            st = osd["state"].get(idx)
            if st is None:
                continue
            n = int(np.prod(shape))
            eng.adam_m[off:off + n] = torch.as_tensor(st["exp_avg"]).reshape(-1).to(eng.device, torch.float32)
            eng.adam_v[off:off + n] = torch.as_tensor(st["exp_avg_sq"]).reshape(-1).to(eng.device, torch.float32)
            steps.append(int(float(st["step"])))
        if steps:
            if len(set(steps)) != 1:
                raise ValueError("per-parameter Adam steps differ: the fused kernel keeps one step count")
            eng.adam_t = steps[0]
    elif osd is not None and "adam_m" in osd:
        eng.adam_m.copy_(torch.as_tensor(osd["adam_m"]).to(eng.device))
        eng.adam_v.copy_(torch.as_tensor(osd["adam_v"]).to(eng.device))
        eng.adam_t = int(osd.get("step", 0))
    if eta is not None:
        eng.params[eng.n_params:] = torch.as_tensor(eta).reshape(3).to(eng.device, torch.float32)


# ---- operator-level wrappers (tests) ----
def op_conv(x_nhwc, w_oihw, bias, ksize, in_mode=0, in_scale=None, in_shift=None, stats=None, transpose_flip=False,
            out_hw=None):
    lib = load_library()
    _need_gpu(x_nhwc, "x")
    N, Hin, Win, cin = x_nhwc.shape
    H, W = (Hin // 2, Win // 2) if in_mode == 2 else (Hin, Win)
    cout = w_oihw.shape[1] if transpose_flip else w_oihw.shape[0]
    out = torch.empty(N, H, W, cout, dtype=torch.float32, device=x_nhwc.device)
    # packed weight image of the kernel family (3x3: Winograd components; 1x1: 32 x 32 operand tiles + the work-queue counters)
    ws = torch.empty(max(((cin + 15) // 16) * ((cout + 63) // 64) * (36 if ksize == 3 else 1) * 16 * 64 * 4,
                         ((cin + 31) // 32) * ((cout + 31) // 32) * 4096 + 512) + 1024, dtype=torch.uint8, device=x_nhwc.device)
    with torch.cuda.device(x_nhwc.device):
        _check(lib.ssp_op_conv(_ptr(x_nhwc), _ptr(w_oihw), _ptr(bias), _ptr(out), N, H, W, cin, cout, ksize, in_mode,
                               _ptr(in_scale), _ptr(in_shift), _ptr(stats), int(transpose_flip), _ptr(ws), ws.numel(),
                               _stream()))
    return out


def op_conv_bf16(x_nhwc, w_oihw, bias, ksize, in_mode=0, in_scale=None, in_shift=None, stats=None, transpose_flip=False,
                 out_f32=False, pool_gamma=None):
    """conv_bf16_kernel as an operator: x bf16 (or fp32) NHWC, fp32 OIHW weights -> bf16 (or fp32) NHWC output
    (+ the raw pooled copy when pool_gamma is given)."""
    lib = load_library()
    _need_gpu(x_nhwc, "x")
    N, H, W, cin = x_nhwc.shape
    cout = w_oihw.shape[1] if transpose_flip else w_oihw.shape[0]
    in_f32 = x_nhwc.dtype == torch.float32
    if not in_f32 and x_nhwc.dtype != torch.bfloat16:
        raise RuntimeError("x must be bfloat16 or float32")
    out = torch.empty(N, H, W, cout, dtype=torch.float32 if out_f32 else torch.bfloat16, device=x_nhwc.device)
    pool = torch.empty(N, H // 2, W // 2, cout, dtype=torch.bfloat16, device=x_nhwc.device) if pool_gamma is not None else None
    ws = torch.empty(((cout + 63) // 64) * ((cin + 31) // 32) * ksize * ksize * 4096, dtype=torch.uint8, device=x_nhwc.device)
    with torch.cuda.device(x_nhwc.device):
        _check(lib.ssp_op_conv_bf16(_ptr(x_nhwc), _ptr(w_oihw), _ptr(bias), _ptr(out), N, H, W, cin, cout, ksize, in_mode,
                                    _ptr(in_scale), _ptr(in_shift), _ptr(stats), int(transpose_flip), int(in_f32), int(out_f32),
                                    _ptr(pool), _ptr(pool_gamma), _ptr(ws), ws.numel(), _stream()))
    return (out, pool) if pool_gamma is not None else out


def op_conv_wgrad_bf16(x_nhwc, dy_nhwc, ksize, in_mode=0, in_scale=None, in_shift=None, dw=None):
    """wgrad_bf16_kernel as an operator: x bf16 NHWC, dY bf16 (or fp32) NHWC -> fp32 OIHW gradient (accumulated into dw)."""
    lib = load_library()
    _need_gpu(x_nhwc, "x")
    N, H, W, cin = x_nhwc.shape
    cout = dy_nhwc.shape[3]
    if x_nhwc.dtype != torch.bfloat16:
        raise RuntimeError("x must be bfloat16")
    dy_f32 = dy_nhwc.dtype == torch.float32
    if dw is None:
        dw = torch.zeros(cout, cin, ksize, ksize, dtype=torch.float32, device=x_nhwc.device)
    ws = torch.empty(512 * ksize * ksize * 4096 * 4, dtype=torch.uint8, device=x_nhwc.device)
    with torch.cuda.device(x_nhwc.device):
        _check(lib.ssp_op_conv_wgrad_bf16(_ptr(x_nhwc), _ptr(dy_nhwc), _ptr(dw), N, H, W, cin, cout, ksize, in_mode,
                                          _ptr(in_scale), _ptr(in_shift), int(dy_f32), _ptr(ws), ws.numel(), _stream()))
    return dw


def op_conv_wgrad(x_nhwc, dout_nhwc, ksize, in_mode=0, in_scale=None, in_shift=None):
    lib = load_library()
    N, Hin, Win, cin = x_nhwc.shape
    _, H, W, cout = dout_nhwc.shape
    dw = torch.zeros(cout, cin, ksize, ksize, dtype=torch.float32, device=x_nhwc.device)
    # partial slabs: 512 x taps x [64][64] (3x3 / generic 1x1) or 512 x [256][128] (grouped pointwise kernel, 256 input channels)
    ws = torch.empty(512 * max(ksize * ksize * 4096, 32768 if ksize == 1 else 0) * 4, dtype=torch.uint8, device=x_nhwc.device)
    with torch.cuda.device(x_nhwc.device):
        _check(lib.ssp_op_conv_wgrad(_ptr(x_nhwc), _ptr(dout_nhwc), _ptr(dw), N, H, W, cin, cout, ksize, in_mode,
                                     _ptr(in_scale), _ptr(in_shift), _ptr(ws), ws.numel(), _stream()))
    return dw


def op_labels(labels2d=None, mask2d=None):
    """labels2Dto3D(add_dustbin=True) and getMasks on the device; returns (target [B,65,Hc,Wc], cellmask [B,Hc,Wc])."""
    lib = load_library()
    ref = labels2d if labels2d is not None else mask2d
    _need_gpu(ref, "labels/mask")
    B, _, H, W = ref.shape
    f32 = dict(dtype=torch.float32, device=ref.device)
    tgt = torch.empty(B, 65, H // 8, W // 8, **f32) if labels2d is not None else None
    cm = torch.empty(B, H // 8, W // 8, **f32) if mask2d is not None else None
    with torch.cuda.device(ref.device):
        _check(lib.ssp_op_labels(_ptr(labels2d), _ptr(mask2d), _ptr(tgt), _ptr(cm), B, H, W, _stream()))
    return tgt, cm


def op_sem_loss(sout_nchw, labels, grad=True, algo=0, cs=None):
    """sem_loss of public NCHW logits [B,C,Hc,Wc] at 1/8 resolution against int64 labels [B,8Hc,8Wc] (C = ignore index): the fused
    bilinear upsample + cross entropy of the training step; returns (loss, d loss / d logits NCHW or None).  algo: see ssp_op_sem_loss."""
    lib = load_library()
    _need_gpu(sout_nchw, "sout")
    B, c, Hc, Wc = sout_nchw.shape
    cs = cs or (c + 7) // 8 * 8
    dev = sout_nchw.device
    x = torch.zeros(B, Hc, Wc, cs, dtype=torch.float32, device=dev)
    x[..., :c] = sout_nchw.permute(0, 2, 3, 1)
    d = torch.full_like(x, float("nan")) if grad else None   # (the operator overwrites it)
    out = torch.zeros(1, dtype=torch.float32, device=dev)
    scratch = torch.empty(65536, dtype=torch.uint8, device=dev)
    lab = labels.to(device=dev, dtype=torch.int64).contiguous()
    assert tuple(lab.shape) == (B, Hc * 8, Wc * 8)
    with torch.cuda.device(dev):
        _check(lib.ssp_op_sem_loss(_ptr(x), cs, _ptr(lab), B, Hc * 8, Wc * 8, c, algo, _ptr(scratch), scratch.numel(), _ptr(out), _ptr(d),
                                   _stream()))
    return float(out.item()), (d[..., :c].permute(0, 3, 1, 2).contiguous() if grad else None)


def _sem_predict_buffers(n, hh, ww, n_classes, dev, labels, want_pred, confusion):
    """Checked arguments of the two sem_predict entry points: (labels | None, pred | None, confusion | None)."""
    if confusion is True:
        confusion = torch.zeros(n_classes, n_classes, dtype=torch.int64, device=dev)
    if confusion is not None:
        _need_gpu(confusion, "confusion")
        if confusion.dtype != torch.int64 or tuple(confusion.shape) != (n_classes, n_classes):
            raise ValueError("confusion must be int64 [%d,%d], got %s %s" % (n_classes, n_classes, confusion.dtype, tuple(confusion.shape)))
        if labels is None:
            raise ValueError("a confusion matrix needs labels")
    if not want_pred and confusion is None:
        raise ValueError("sem_predict: neither a class map nor a confusion matrix requested")
    if hh % 8 or ww % 8:
        raise ValueError("sem_predict: H and W must be multiples of 8, got %dx%d" % (hh, ww))
    if labels is not None:
        _need_gpu(labels, "semantic labels")
        if labels.dtype != torch.int64 or tuple(labels.shape) != (n, hh, ww):
            raise ValueError("semantic labels must be int64 [B,H,W] = %s, got %s %s" % ((n, hh, ww), labels.dtype, tuple(labels.shape)))
    pred = torch.empty(n, hh, ww, dtype=torch.uint8, device=dev) if want_pred else None
    return labels, pred, confusion


def op_sem_predict(sout_nchw, labels=None, want_pred=True, confusion=None, cs=None, n_classes=None):
    """Class map and confusion matrix of public NCHW logits [B,C,Hc,Wc] at 1/8 resolution, as the segmentation head is read during
    training: bilinear upsample x8 (align_corners=False) + argmax over the classes in one kernel, without the [B,C,8Hc,8Wc] logits.
    Ties go to the lowest class index.  labels: int64 [B,8Hc,8Wc] on the device; values outside [0, C) are ignored (op_sem_loss).
    confusion: an int64 [C,C] device matrix to ACCUMULATE into (row = label, column = prediction), True for a fresh one, None for
    none.  cs: channel stride of the NHWC copy the kernel reads (default: C rounded up to 8; the padding is zero).  n_classes <
    C: only the first n_classes channels are classes, the others play the padding of a stride-C map AS GIVEN (test hook).
    Returns (pred uint8 [B,8Hc,8Wc] | None, confusion | None)."""
    lib = load_library()
    _need_gpu(sout_nchw, "sout")
    B, c, Hc, Wc = sout_nchw.shape
    dev = sout_nchw.device
    if n_classes is None:
        n_classes = c
        cs = cs or (c + 7) // 8 * 8
        x = torch.zeros(B, Hc, Wc, cs, dtype=torch.float32, device=dev)
        x[..., :c] = sout_nchw.permute(0, 2, 3, 1)
    else:
        cs = c
        x = sout_nchw.permute(0, 2, 3, 1).contiguous().float()
    labels, pred, confusion = _sem_predict_buffers(B, Hc * 8, Wc * 8, n_classes, dev, labels, want_pred, confusion)
    with torch.cuda.device(dev):
        _check(lib.ssp_op_sem_predict(_ptr(x), cs, _ptr(labels), B, Hc * 8, Wc * 8, n_classes, _ptr(pred), _ptr(confusion), _stream()))
    return pred, confusion


def _point_class_args(pts, count):
    _need_gpu(pts, "pts")
    _need_gpu(count, "count")
    if pts.dtype != torch.float32 or pts.dim() != 3 or pts.shape[2] < 2:
        raise ValueError("pts must be float32 [n, cap, >= 2] rows starting (x, y), got %s %s" % (pts.dtype, tuple(pts.shape)))
    if count.dtype != torch.int32 or count.numel() != pts.shape[0]:
        raise ValueError("count must be int32 [%d]" % pts.shape[0])
    return pts, count


def op_point_classes(sout_nchw, pts, count, n_classes=None):
    """The class of each keypoint on public NCHW logits [B,C,Hc,Wc] at 1/8 resolution, without the class map: row r < count[b]
    of pts [B,cap,>=2] (float32 rows starting with the integer pixel (x, y), e.g. Engine.describe_points' "pts") gets exactly
    op_sem_predict(sout_nchw)[0][b, y, x]; rows past the count get CLASS_NONE.  n_classes < C: only the first n_classes channels
    are classes, the others play the padding of a stride-C map AS GIVEN (test hook, as in op_sem_predict).  At most 255 classes.
    Returns uint8 [B,cap] on the device; no host synchronisation."""
    lib = load_library()
    _need_gpu(sout_nchw, "sout")
    pts, count = _point_class_args(pts, count)
    B, c, Hc, Wc = sout_nchw.shape
    if pts.shape[0] != B:
        raise ValueError("pts holds %d images, the logits %d" % (pts.shape[0], B))
    dev = sout_nchw.device
    if n_classes is None:
        n_classes, cs = c, (c + 7) // 8 * 8
        x = torch.zeros(B, Hc, Wc, cs, dtype=torch.float32, device=dev)
        x[..., :c] = sout_nchw.permute(0, 2, 3, 1)
    else:
        cs = c
        x = sout_nchw.permute(0, 2, 3, 1).contiguous().float()
    cap, stride = pts.shape[1], pts.shape[2]
    cls = torch.empty(B, cap, dtype=torch.uint8, device=dev)
    if cap == 0:
        return cls
    with torch.cuda.device(dev):
        _check(lib.ssp_op_point_classes(_ptr(x), cs, B, Hc * 8, Wc * 8, int(n_classes), _ptr(pts), stride, _ptr(count), cap,
                                        _ptr(cls), _stream()))
    return cls


def class_mask(keep=None, drop=None, n_classes=133):
    """The 256-bit keep mask of op_filter_points as eight 32-bit words (bit c of word c // 32 = class c is kept): exactly one of
    `keep` (the classes to keep) and `drop` (the classes to remove among 0 .. n_classes-1) is given.  Ids outside [0, n_classes)
    raise ValueError."""
    if (keep is None) == (drop is None):
        raise ValueError("class_mask: exactly one of keep and drop must be given")
    n_classes = int(n_classes)
    if not 1 <= n_classes <= CLASS_NONE:
        raise ValueError("class_mask: 1 <= n_classes <= %d required (got %d)" % (CLASS_NONE, n_classes))
    ids = [int(c) for c in (keep if keep is not None else drop)]
    for c in ids:
        if not 0 <= c < n_classes:
            raise ValueError("class_mask: class id %d outside [0, %d)" % (c, n_classes))
    kept = set(ids) if keep is not None else set(range(n_classes)) - set(ids)
    words = [0] * 8
    for c in kept:
        words[c >> 5] |= 1 << (c & 31)
    return tuple(words)


def op_filter_points(pts, count, desc, cls, mask):
    """Stable per-image compaction of a point set by class (ssp_op_filter_points): pts float32 [n,cap,5], count int32 [n], desc
    float32 [n,cap,256], cls uint8 [n,cap] as Engine.describe_points(classes=True) returns them, mask = class_mask(...).  The rows
    below the count whose class bit is set keep their order.  Returns new device tensors {"pts", "count", "desc", "cls"}: rows
    past the new count are CLASS_NONE in "cls" and unspecified elsewhere.  No host synchronisation."""
    lib = load_library()
    for t, nm in ((pts, "pts"), (count, "count"), (desc, "desc"), (cls, "cls")):
        _need_gpu(t, nm)
    mask = [int(w) for w in mask]
    if len(mask) != 8 or any(not 0 <= w < 1 << 32 for w in mask):
        raise ValueError("mask must be eight 32-bit words (class_mask)")
    if pts.dtype != torch.float32 or pts.dim() != 3 or pts.shape[2] != 5:
        raise ValueError("pts must be float32 [n, cap, 5], got %s %s" % (pts.dtype, tuple(pts.shape)))
    n, cap = pts.shape[0], pts.shape[1]
    if desc.dtype != torch.float32 or tuple(desc.shape) != (n, cap, 256):
        raise ValueError("desc must be float32 [%d, %d, 256]" % (n, cap))
    if cls.dtype != torch.uint8 or tuple(cls.shape) != (n, cap) or count.dtype != torch.int32 or count.numel() != n:
        raise ValueError("cls must be uint8 [%d, %d] and count int32 [%d]" % (n, cap, n))
    dev = pts.device
    out = {"pts": torch.empty_like(pts), "count": torch.zeros(n, dtype=torch.int32, device=dev),
           "desc": torch.empty_like(desc), "cls": torch.empty_like(cls)}
    if n == 0 or cap == 0:
        return out
    wsb = lib.ssp_filter_workspace_bytes(n, cap)
    if wsb == 0:
        _check(-1)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _check(lib.ssp_op_filter_points(_ptr(pts), _ptr(count), _ptr(desc), _ptr(cls), (C.c_uint32 * 8)(*mask), n, cap,
                                        _ptr(out["pts"]), _ptr(out["count"]), _ptr(out["desc"]), _ptr(out["cls"]), _ptr(ws),
                                        _stream()))
    return out


def sem_metrics(confusion):
    """Pixel accuracy and mean intersection over union of a confusion matrix [C,C] (row = label, column = prediction; torch tensor on
    any device or numpy array; one device-to-host copy).  With tp = diag, row = sums over the predictions, col = sums over the labels:
      n_pixels = confusion.sum();  pixel_acc = tp.sum() / n_pixels (nan without pixels);
      iou[c] = tp[c] / (row[c] + col[c] - tp[c]) (nan where that union is 0: the class occurs in neither labels nor predictions);
      miou = mean of the non-nan iou (nan when there is none);  classes_present = their number.
    This is the standard definition.  The reference's only mIoU is the smoothed soft-IoU of the non-functional `_ang` trainer
    (Train_model_heatmap_all_ang.py:181-190, under "TODO: mIoU with ignore index"): one (intersection + 0.01) / (union + 0.01) over
    all classes and pixels of soft predictions at once, without an ignore label; it is deliberately not reproduced."""
    m = confusion.detach().cpu().numpy() if torch.is_tensor(confusion) else np.asarray(confusion)
    if m.ndim != 2 or m.shape[0] != m.shape[1]:
        raise ValueError("confusion must be a square matrix, got shape %s" % (tuple(m.shape),))
    m = m.astype(np.float64)
    tp, row, col = np.diag(m), m.sum(1), m.sum(0)
    n_pixels = m.sum()
    union = row + col - tp
    present = union > 0
    iou = np.full(m.shape[0], np.nan)
    iou[present] = tp[present] / union[present]
    return {"n_pixels": int(n_pixels), "pixel_acc": float(tp.sum() / n_pixels) if n_pixels > 0 else float("nan"),
            "iou": iou, "miou": float(iou[present].mean()) if present.any() else float("nan"),
            "classes_present": int(present.sum())}


def op_detector_loss(semi_nchw, labels2d, mask2d, grad=True):
    """detector_loss (softmax + BCE) of public NCHW logits [B,65,Hc,Wc]; returns (loss, d loss / d semi NCHW or None)."""
    lib = load_library()
    _need_gpu(semi_nchw, "semi")
    B, c, Hc, Wc = semi_nchw.shape
    assert c == 65
    dev = semi_nchw.device
    x = torch.zeros(B, Hc, Wc, 80, dtype=torch.float32, device=dev)
    x[..., :65] = semi_nchw.permute(0, 2, 3, 1)
    d = torch.empty_like(x) if grad else None
    out = torch.zeros(1, dtype=torch.float32, device=dev)
    scratch = torch.empty(65536 + 4 * (B * Hc * Wc + 256), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _check(lib.ssp_op_detector_loss(_ptr(x), 80, _ptr(labels2d.contiguous()), _ptr(mask2d.contiguous()), B, Hc * 8, Wc * 8,
                                        _ptr(scratch), scratch.numel(), _ptr(out), _ptr(d), _stream()))
    return float(out.item()), (d[..., :65].permute(0, 3, 1, 2).contiguous() if grad else None)


def op_sparse_loss(desc_a_nchw, desc_b_nchw, match_a, match_b, nonmatch_b, method="2d", dist="cos", grad=None, gather=None, csr=False):
    """(positive_dist, negative_dist) of the sparse descriptor loss for NCHW descriptor maps and explicit indices; with
    grad = (coef_pos, coef_neg) also the gradients of coef_pos * positive_dist + coef_neg * negative_dist wrt both maps (NCHW).
    method / dist: sparse_loss.params ("2d" / "cos" in every shipped config; see Engine.pair_step).
    gather: path of the match term's gradient - True = per-cell gather over corner lists, False = atomic scatter, None = the process
    default (SSP_DESC_GATHER).  csr (gather path with grad): also return the corner lists (offsets [B, 2, Hc*Wc + 1] int32,
    match [B, 2, 4 n_match] int32, weight [B, 2, 4 n_match] float32; only the first offsets[..., -1] entries of a list are defined)."""
    lib = load_library()
    _need_gpu(desc_a_nchw, "desc")
    B, D, Hc, Wc = desc_a_nchw.shape
    a = desc_a_nchw.permute(0, 2, 3, 1).contiguous()
    b = desc_b_nchw.permute(0, 2, 3, 1).contiguous()
    out = torch.zeros(2, dtype=torch.float32, device=a.device)
    da = torch.full_like(a, float("nan")) if grad is not None else None   # (the operator overwrites them)
    db = torch.full_like(b, float("nan")) if grad is not None else None
    cp, cn = grad if grad is not None else (0.0, 0.0)
    n_match = match_a.shape[1]
    lists = None
    if csr:
        lists = (torch.zeros(B, 2, Hc * Wc + 1, dtype=torch.int32, device=a.device),
                 torch.full((B, 2, 4 * n_match), -1, dtype=torch.int32, device=a.device),
                 torch.full((B, 2, 4 * n_match), float("nan"), dtype=torch.float32, device=a.device))
    with torch.cuda.device(a.device):
        if gather is None and not csr:
            _check(lib.ssp_op_sparse_loss(_ptr(a), _ptr(b), _ptr(match_a), _ptr(match_b), _ptr(nonmatch_b), B, Hc, Wc,
                                          n_match, nonmatch_b.shape[1] // n_match, int(method != "2d"), int(dist != "cos"),
                                          float(cp), float(cn), _ptr(da), _ptr(db), _ptr(out), _stream()))
        else:
            _check(lib.ssp_op_sparse_loss_path(_ptr(a), _ptr(b), _ptr(match_a), _ptr(match_b), _ptr(nonmatch_b), B, Hc, Wc,
                                               n_match, nonmatch_b.shape[1] // n_match, int(method != "2d"), int(dist != "cos"),
                                               float(cp), float(cn), _ptr(da), _ptr(db), _ptr(out),
                                               -1 if gather is None else int(bool(gather)), _ptr(lists[0]) if csr else None,
                                               _ptr(lists[1]) if csr else None, _ptr(lists[2]) if csr else None, _stream()))
    torch.cuda.synchronize()
    if grad is None:
        return float(out[0]), float(out[1])
    res = (float(out[0]), float(out[1]), da.permute(0, 3, 1, 2).contiguous(), db.permute(0, 3, 1, 2).contiguous())
    return res + (lists,) if csr else res


def op_dense_loss(desc_a_nchw, desc_b_nchw, homographies, mask_valid, lamda_d=250.0, descriptor_dist=4.0, grad=None):
    """Dense descriptor loss (utils/utils.py:779-893) of NCHW descriptor maps.  Returns (loss, pos_sum, neg_sum) and,
    with grad = ("loss", scale) or ("multi_task", scale), the gradients of scale * loss_desc resp.
    scale * (pos_sum + neg_sum) wrt both maps (NCHW)."""
    lib = load_library()
    _need_gpu(desc_a_nchw, "desc")
    B, D, Hc, Wc = desc_a_nchw.shape
    dev = desc_a_nchw.device
    a = desc_a_nchw.permute(0, 2, 3, 1).contiguous()
    b = desc_b_nchw.permute(0, 2, 3, 1).contiguous()
    hm = homographies.to(dev, torch.float32).contiguous()
    mv = mask_valid.to(dev, torch.float32).reshape(B, Hc * Wc).contiguous()
    out = torch.zeros(3, dtype=torch.float32, device=dev)
    da = torch.empty_like(a) if grad else None
    db = torch.empty_like(b) if grad else None
    scratch = torch.empty(65536 + (B * (Hc * Wc) ** 2 * 4 if grad else 0), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _check(lib.ssp_op_dense_loss(_ptr(a), _ptr(b), _ptr(hm), _ptr(mv), B, Hc, Wc, float(lamda_d), float(descriptor_dist),
                                     int(bool(grad and grad[0] == "multi_task")), float(grad[1]) if grad else 0.0,
                                     _ptr(scratch), scratch.numel(), _ptr(out), _ptr(da), _ptr(db), _stream()))
    o = out.cpu().tolist()
    if not grad:
        return o[0], o[1], o[2]
    return (o[0], o[1], o[2]), da.permute(0, 3, 1, 2).contiguous(), db.permute(0, 3, 1, 2).contiguous()


def op_bn_bwd(y_nhwc, dout_nhwc, gamma, scale, shift, mean, invstd, relu=True, pool=False):
    """Backward of BatchNorm2d(train)+ReLU(+MaxPool2d(2)); returns (dy, dgamma, dbeta, dbias).  The channel count is
    len(gamma); the NHWC tensors may be channel-padded (pixel stride = their last dimension, a multiple of 4)."""
    lib = load_library()
    _need_gpu(y_nhwc, "y")
    N, H, W, cs = y_nhwc.shape
    Cc = gamma.numel()
    dev = y_nhwc.device
    stats4 = torch.cat([scale, shift, mean, invstd]).contiguous()
    dy = torch.zeros_like(y_nhwc) if cs != Cc else torch.empty_like(y_nhwc)
    dg, db, dbias = (torch.zeros(Cc, dtype=torch.float32, device=dev) for _ in range(3))
    sums = torch.zeros(NREP * 2 * Cc, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _check(lib.ssp_op_bn_bwd_strided(_ptr(y_nhwc), _ptr(dout_nhwc), _ptr(gamma), _ptr(stats4), _ptr(dy), _ptr(dg),
                                         _ptr(db), _ptr(dbias), _ptr(sums), N, H, W, Cc, cs, int(relu), int(pool), _stream()))
    return dy, dg, db, dbias


def op_bn_bwd_bf16(y_nhwc, dout_nhwc, gamma, scale, shift, mean, invstd, pool=False):
    """op_bn_bwd on bf16 tensors (BatchNorm + ReLU (+ MaxPool2d(2)) backward of the bf16 path); dy is bf16."""
    lib = load_library()
    _need_gpu(y_nhwc, "y")
    if y_nhwc.dtype != torch.bfloat16 or dout_nhwc.dtype != torch.bfloat16:
        raise RuntimeError("y and dout must be bfloat16")
    N, H, W, cs = y_nhwc.shape
    Cc = gamma.numel()
    dev = y_nhwc.device
    stats4 = torch.cat([scale, shift, mean, invstd]).contiguous()
    dy = torch.zeros_like(y_nhwc)
    dg, db, dbias = (torch.zeros(Cc, dtype=torch.float32, device=dev) for _ in range(3))
    sums = torch.zeros(NREP * 2 * Cc, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _check(lib.ssp_op_bn_bwd_bf16(_ptr(y_nhwc), _ptr(dout_nhwc), _ptr(gamma), _ptr(stats4), _ptr(dy), _ptr(dg), _ptr(db),
                                      _ptr(dbias), _ptr(sums), N, H, W, Cc, cs, 1, int(pool), _stream()))
    return dy, dg, db, dbias


def op_warp_image(img, inv_h, nearest=False):
    """inv_warp_image_batch on the device: img [B,1,H,W], inv_h [B,3,3] -> warped [B,1,H,W]."""
    lib = load_library()
    _need_gpu(img, "img")
    inv_h = inv_h.to(img.device, torch.float32).contiguous()
    B, _, H, W = img.shape
    out = torch.empty_like(img)
    with torch.cuda.device(img.device):
        _check(lib.ssp_op_warp_image(_ptr(img), _ptr(inv_h), _ptr(out), B, H, W, int(bool(nearest)), _stream()))
    return out


def op_erode(mask, radius):
    lib = load_library()
    _need_gpu(mask, "mask")
    B, _, H, W = mask.shape
    out = torch.empty_like(mask)
    with torch.cuda.device(mask.device):
        _check(lib.ssp_op_erode(_ptr(mask), _ptr(out), B, H, W, int(radius), _stream()))
    return out


def op_warp_labels(labels, hn, exact=True):
    """warpLabels on a keypoint map.  exact=True (default): the pixel-space homography is computed on the host like the
    reference (`scaled_homographies`) -> bit-identical indices; exact=False: analytic T^-1 H T on the device (no D2H copy)."""
    lib = load_library()
    _need_gpu(labels, "labels")
    B, _, H, W = labels.shape
    out = torch.empty_like(labels)
    with torch.cuda.device(labels.device):
        if exact:
            hpx = scaled_homographies(hn, H, W).to(labels.device)
            _check(lib.ssp_op_warp_labels_px(_ptr(labels), _ptr(hpx), _ptr(out), B, H, W, _stream()))
        else:
            hn = hn.to(labels.device, torch.float32).contiguous()
            _check(lib.ssp_op_warp_labels(_ptr(labels), _ptr(hn), _ptr(out), B, H, W, _stream()))
    return out


# ---- homography-adaptation export operators ----
def op_homoadapt_views(img, inv_h):
    """datasets/Coco.py:279-288 on the device: img [H,W], inv_h [n,3,3] -> (views [n,1,H,W], masks [n,1,H,W])."""
    lib = load_library()
    _need_gpu(img, "img")
    inv_h = inv_h.to(img.device, torch.float32).contiguous()
    n, (H, W) = inv_h.shape[0], img.shape[-2:]
    views = torch.empty(n, 1, H, W, dtype=torch.float32, device=img.device)
    masks = torch.empty_like(views)
    with torch.cuda.device(img.device):
        _check(lib.ssp_op_homoadapt_views(_ptr(img), _ptr(inv_h), _ptr(views), _ptr(masks), n, H, W, _stream()))
    return views, masks


def op_flatten_detection(semi, mask=None):
    """flattenDetection (utils/utils.py:515-560) of semi [n,65,Hc,Wc] -> [n,1,8Hc,8Wc], times mask if given."""
    lib = load_library()
    _need_gpu(semi, "semi")
    n, c, Hc, Wc = semi.shape
    assert c == 65
    out = torch.empty(n, 1, Hc * 8, Wc * 8, dtype=torch.float32, device=semi.device)
    if mask is not None:
        _need_gpu(mask, "mask")
    with torch.cuda.device(semi.device):
        _check(lib.ssp_op_flatten_detection(_ptr(semi), _ptr(mask), _ptr(out), n, Hc, Wc, _stream()))
    return out


def op_combine_heatmap(heat, mask, unwarp_h):
    """combine_heatmap (export.py:49-60); heat must already be heatmap*mask.  -> [H,W]"""
    lib = load_library()
    _need_gpu(heat, "heat")
    _need_gpu(mask, "mask")
    unwarp_h = unwarp_h.to(heat.device, torch.float32).contiguous()
    n, (H, W) = heat.shape[0], heat.shape[-2:]
    out = torch.empty(H, W, dtype=torch.float32, device=heat.device)
    with torch.cuda.device(heat.device):
        _check(lib.ssp_op_combine_heatmap(_ptr(heat), _ptr(mask), _ptr(unwarp_h), _ptr(out), n, H, W, _stream()))
    return out


def op_heatmap_points(heatmap, conf_thresh, nms_dist=4, border_remove=4, top_k=0, subpixel=False):
    """getPtsFromHeatmap (+ soft_argmax_points, top-k) on the device.  Returns a float64 numpy [N,3] array of
    (x, y, conf), assembled exactly like models/model_wrap.py:245 (x + sx - 2 in float64)."""
    lib = load_library()
    _need_gpu(heatmap, "heatmap")
    H, W = heatmap.shape
    p = SspExportParams(1, H, W, float(np.float32(conf_thresh)), int(nms_dist), int(border_remove), int(top_k or 0),
                        int(bool(subpixel)))
    wsb, cap = lib.ssp_export_workspace_bytes(C.byref(p)), lib.ssp_export_max_points(C.byref(p))
    if wsb == 0 or cap < 0:
        _check(-1)
    ws = torch.empty(wsb, dtype=torch.uint8, device=heatmap.device)
    pts = torch.empty(max(cap, 1), 5, dtype=torch.float32, device=heatmap.device)
    cnt = torch.zeros(1, dtype=torch.int32, device=heatmap.device)
    with torch.cuda.device(heatmap.device):
        _check(lib.ssp_op_heatmap_points(_ptr(heatmap), C.byref(p), _ptr(ws), _ptr(pts), _ptr(cnt), _stream()))
    return points_to_numpy(pts, cnt, subpixel)


def op_heatmap_nms(heat, labels=None, conf_thresh=0.015, nms_dist=4, border_remove=4, want_map=True):
    """heatmap_to_nms + the per-image terms of batch_precision_recall on the device.  heat, labels: [B,1,H,W] (or
    [B,H,W]).  Returns (nms_map [B,H,W] or None, pr [B,2] = (precision, recall) or None) as device tensors."""
    lib = load_library()
    _need_gpu(heat, "heat")
    B, (H, W) = heat.shape[0], heat.shape[-2:]
    p = SspExportParams(1, H, W, float(np.float32(conf_thresh)), int(nms_dist), int(border_remove), 0, 0)
    wsb = lib.ssp_export_workspace_bytes(C.byref(p))
    if wsb == 0:
        _check(-1)
    ws = torch.empty(wsb, dtype=torch.uint8, device=heat.device)
    if labels is not None:
        _need_gpu(labels, "labels")
        assert labels.numel() == heat.numel() and labels.dtype == torch.float32
    nms = torch.empty(B, H, W, dtype=torch.float32, device=heat.device) if want_map else None
    pr = torch.empty(B, 2, dtype=torch.float32, device=heat.device) if labels is not None else None
    with torch.cuda.device(heat.device):
        _check(lib.ssp_op_heatmap_nms(_ptr(heat), C.byref(p), B, _ptr(ws), _ptr(labels), _ptr(nms), _ptr(pr), _stream()))
    return nms, pr


def op_soft_argmax_points(heatmap, xy):
    """(sx, sy) in [0,4] of the 5x5 soft-argmax around each (x, y) of xy [n,2] (device float32) -> device [n,2]."""
    lib = load_library()
    _need_gpu(heatmap, "heatmap")
    _need_gpu(xy, "xy")
    H, W = heatmap.shape
    out = torch.empty(xy.shape[0], 2, dtype=torch.float32, device=heatmap.device)
    with torch.cuda.device(heatmap.device):
        _check(lib.ssp_op_soft_argmax_points(_ptr(heatmap), _ptr(xy), _ptr(out), xy.shape[0], H, W, _stream()))
    return out


def op_sample_descriptors(desc, xy, counts=None):
    """sample_desc_from_points (models/model_wrap.py:295-313) on the device: desc [B,256,Hc,Wc] (the L2-normalised coarse
    descriptor), xy [B,cap,2] float32 points (x, y) in pixels, counts [B] int32 (default: all cap).  Image b samples its own
    map.  Returns [B,cap,256] unit rows (rows >= counts[b] are undefined)."""
    lib = load_library()
    _need_gpu(desc, "desc")
    _need_gpu(xy, "xy")
    B, D, hc, wc = desc.shape
    assert D == 256 and desc.dtype == torch.float32 and xy.dtype == torch.float32 and xy.shape[0] == B and xy.shape[2] == 2
    cap = xy.shape[1]
    if counts is None:
        counts = torch.full((B,), cap, dtype=torch.int32, device=desc.device)
    _need_gpu(counts, "counts")
    assert counts.dtype == torch.int32 and counts.numel() == B
    out = torch.empty(B, cap, 256, dtype=torch.float32, device=desc.device)
    with torch.cuda.device(desc.device):
        _check(lib.ssp_op_sample_descriptors(_ptr(desc), B, hc, wc, _ptr(xy), _ptr(counts), cap, _ptr(out), _stream()))
    return out


def op_match_two_way(desc1, count1, desc2, count2, nn_thresh, pair_stride=1, n_pairs=None, cls1=None, cls2=None):
    """PointTracker.nn_match_two_way (models/model_wrap.py:451-497) for P pairs on the device.  desc1, desc2:
    [P*pair_stride, cap, 256] unit rows, count1, count2: [P*pair_stride] int32 (pair p uses entry p*pair_stride).
    cls1, cls2 (both or neither): uint8 [P*pair_stride, cap] classes beside the descriptors; rows of different classes are
    never matched (ssp_match_two_way_classes).
    Returns (match [P,cap,3] rows (i, j, score) in ascending i, n_match [P] int32) as device tensors."""
    lib = load_library()
    if nn_thresh < 0.0:
        raise ValueError("'nn_thresh' should be non-negative")
    if (cls1 is None) != (cls2 is None):
        raise ValueError("cls1 and cls2: both or neither")
    for t, nm in ((desc1, "desc1"), (desc2, "desc2"), (count1, "count1"), (count2, "count2")):
        _need_gpu(t, nm)
    cap = desc1.shape[1]
    assert desc1.shape[1:] == (cap, 256) and desc2.shape[1:] == (cap, 256), "both sides need the same [cap,256] rows"
    assert count1.dtype == torch.int32 and count2.dtype == torch.int32
    P = n_pairs if n_pairs is not None else desc1.shape[0] // pair_stride
    assert (P - 1) * pair_stride < min(desc1.shape[0], desc2.shape[0], count1.numel(), count2.numel())
    wsb = lib.ssp_match_workspace_bytes(cap, P)
    if wsb == 0:
        _check(-1)
    ws = torch.empty(wsb, dtype=torch.uint8, device=desc1.device)
    match = torch.empty(P, cap, 3, dtype=torch.float32, device=desc1.device)
    n_match = torch.empty(P, dtype=torch.int32, device=desc1.device)
    if cls1 is not None:
        _tensor(cls1, "cls1", torch.uint8, (desc1.shape[0], cap), "a class beside each row of desc1")
        _tensor(cls2, "cls2", torch.uint8, (desc2.shape[0], cap), "a class beside each row of desc2")
    with torch.cuda.device(desc1.device):
        if cls1 is not None:
            _check(lib.ssp_match_two_way_classes(_ptr(desc1), _ptr(count1), _ptr(desc2), _ptr(count2), _ptr(cls1), _ptr(cls2),
                                                 cap, P, int(pair_stride), float(np.float32(nn_thresh)), _ptr(ws), _ptr(match),
                                                 _ptr(n_match), _stream()))
        else:
            _check(lib.ssp_match_two_way(_ptr(desc1), _ptr(count1), _ptr(desc2), _ptr(count2), cap, P, int(pair_stride),
                                         float(np.float32(nn_thresh)), _ptr(ws), _ptr(match), _ptr(n_match), _stream()))
    return match, n_match


# ---- point tracks over a frame sequence (PointTracker.update / get_tracks) ----
def track_table(max_length, point_cap, device):
    """An empty device track table for frames of at most point_cap points: {"ids": int32 [row_cap,L], "tid": int32 [row_cap],
    "score": float64 [row_cap], "state": int32 [2+L] = n_rows, track_count, point counts of the L retained frames} plus the
    host-known sizes "L", "point_cap", "row_cap" = L * point_cap and a "ws" workspace shared by the table's successors."""
    lib = load_library()
    L, point_cap = int(max_length), int(point_cap)
    if not 2 <= L <= TRACK_MAX_LENGTH:
        raise ValueError("2 <= max_length <= %d required (got %d)" % (TRACK_MAX_LENGTH, L))
    if not 1 <= point_cap <= MATCH_MAX_POINTS:
        raise ValueError("1 <= point_cap <= %d points per frame (got %d)" % (MATCH_MAX_POINTS, point_cap))
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("track_table needs a HIP device: the MI355X path has no CPU fallback")
    row_cap = L * point_cap
    wsb = lib.ssp_track_workspace_bytes(L, point_cap, row_cap)
    if wsb == 0:
        _check(-1)
    t = _track_arrays(L, row_cap, device)
    t["state"].zero_()
    t.update(L=L, point_cap=point_cap, row_cap=row_cap, ws=torch.empty(wsb, dtype=torch.uint8, device=device))
    return t


def _track_arrays(L, row_cap, device):
    return {"ids": torch.empty(row_cap, L, dtype=torch.int32, device=device),
            "tid": torch.empty(row_cap, dtype=torch.int32, device=device),
            "score": torch.empty(row_cap, dtype=torch.float64, device=device),
            "state": torch.empty(2 + L, dtype=torch.int32, device=device)}


def op_track_update(table, match, n_match, n_points, match_score64=None, out=None):
    """One PointTracker.update on the device (ssp_op_track_update).  table: a track_table() or the result of an earlier call;
    match: float32 [>= point_cap rows, 3] (i, j, distance) with n_match int32 [1] rows, as op_match_two_way returns them for
    (previous frame, new frame); n_points: int32 [1] points of the new frame; match_score64: optional float64 [point_cap]
    distances used instead of column 2.  Returns the updated table in `out` (another table of the same sizes, default: new
    arrays); the input table is left as it was.  No host synchronisation."""
    lib = load_library()
    L, point_cap, row_cap = table["L"], table["point_cap"], table["row_cap"]
    _tensor(match, "match", torch.float32, ((point_cap, None), 3), "rows (i, j, distance)")
    for t, nm in ((n_match, "n_match"), (n_points, "n_points")):
        _need_gpu(t, nm)
        if t.dtype != torch.int32:
            raise ValueError("%s must be an int32 device scalar" % nm)
    if match_score64 is not None:
        _need_gpu(match_score64, "match_score64")
        if match_score64.dtype != torch.float64 or match_score64.numel() < point_cap:
            raise ValueError("match_score64 must be float64 [>= %d]" % point_cap)
    dev = table["ids"].device
    if out is None:
        out = _track_arrays(L, row_cap, dev)
    elif out["ids"].shape != table["ids"].shape or out["ids"].data_ptr() == table["ids"].data_ptr():
        raise ValueError("out must be another table of the same sizes")
    out.update(L=L, point_cap=point_cap, row_cap=row_cap, ws=table["ws"])
    with torch.cuda.device(dev):
        _check(lib.ssp_op_track_update(_ptr(table["ids"]), _ptr(table["tid"]), _ptr(table["score"]), _ptr(table["state"]),
                                       _ptr(match), _ptr(match_score64), _ptr(n_match), _ptr(n_points), L, point_cap, row_cap,
                                       _ptr(table["ws"]), _ptr(out["ids"]), _ptr(out["tid"]), _ptr(out["score"]),
                                       _ptr(out["state"]), _stream()))
    return out


def op_track_select(table, min_length):
    """get_tracks(min_length) on the device (ssp_op_track_select): (tracks float64 [row_cap, 2+L] rows (track id, score, ids),
    n_tracks int32 [1]) as device tensors; min_length = 0 returns every row of the table."""
    lib = load_library()
    L, row_cap = table["L"], table["row_cap"]
    dev = table["ids"].device
    tracks = torch.empty(row_cap, 2 + L, dtype=torch.float64, device=dev)
    n = torch.empty(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _check(lib.ssp_op_track_select(_ptr(table["ids"]), _ptr(table["tid"]), _ptr(table["score"]), _ptr(table["state"]), L,
                                       row_cap, int(min_length), _ptr(table["ws"]), _ptr(tracks), _ptr(n), _stream()))
    return tracks, n


def tracks_to_numpy(tracks, n_tracks):
    """Device (tracks, n_tracks) of op_track_select -> the reference's float64 [M, 2+L] matrix (one host synchronisation)."""
    return tracks[:int(n_tracks.item())].cpu().numpy()


def op_track_points(tracks, n_tracks, pts, state, first_slot=0):
    """Coordinates of the points a tracks matrix names (ssp_op_track_points).  tracks: float64 [track_cap, 2+L] with n_tracks
    int32 [1] rows; pts: float64 [L, point_cap, 2] (x, y), retained frame c in slot (first_slot + c) % L; state: the table's
    state vector.  Returns float64 [track_cap, L, 2], NaN where the id is -1 (rows >= n_tracks are undefined)."""
    lib = load_library()
    _need_gpu(tracks, "tracks")
    L = tracks.shape[1] - 2
    _tensor(tracks, "tracks", torch.float64, (None, 2 + L), "rows (track id, score, L ids)")
    _tensor(pts, "pts", torch.float64, (L, None, 2), "L from tracks [M, 2+L]")
    _count(state, "state", 2 + L, hint="2+L, L from tracks")
    _need_gpu(n_tracks, "n_tracks")
    if n_tracks.dtype != torch.int32:
        raise ValueError("n_tracks must be an int32 device scalar")
    xy = torch.empty(tracks.shape[0], L, 2, dtype=torch.float64, device=tracks.device)
    if tracks.shape[0] == 0:
        return xy
    with torch.cuda.device(tracks.device):
        _check(lib.ssp_op_track_points(_ptr(tracks), _ptr(n_tracks), _ptr(pts), _ptr(state), L, pts.shape[1], tracks.shape[0],
                                       int(first_slot), _ptr(xy), _stream()))
    return xy


# ---- detector evaluation against ground-truth corners (evaluations/detector_evaluation.py:15-136) ----
def detector_eval_r2(distance_thresh):
    """The largest integer d2 with np.sqrt(np.float64(d2)) <= distance_thresh: the reference's `dist <= distance_thresh` on
    integer pixel offsets as an integer compare (-1: nothing matches)."""
    d = float(distance_thresh)
    if not d >= 0.0:
        return -1
    r2 = int(min(d, 1e4) ** 2) + 1
    while r2 >= 0 and not np.sqrt(np.float64(r2)) <= np.float64(d):
        r2 -= 1
    return r2


def detector_eval_state(device):
    """An empty evaluation state block: int64 [DET_EVAL_STATE_WORDS] (records, n_gt, overflow flag, rows outside the image, d2
    histogram)."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("detector_eval_state needs a HIP device: the MI355X path has no CPU fallback")
    return torch.zeros(DET_EVAL_STATE_WORDS, dtype=torch.int64, device=device)


def _det_eval_args(labels, keys, state, remove_zero, r2, prob_thresh, simplified):
    _need_gpu(labels, "labels")
    if labels.dtype not in (torch.float32, torch.uint8):
        raise ValueError("labels must be float32 or uint8 (nonzero = ground truth)")
    if labels.dim() == 4 and labels.shape[1] == 1:
        labels = labels[:, 0]
    if labels.dim() != 3:
        raise ValueError("labels must be [B,H,W] (or [B,1,H,W])")
    _tensor(keys, "keys", torch.int64, ((1, None),), "its length is the record capacity")
    _count(state, "state", DET_EVAL_STATE_WORDS, torch.int64)
    B, H, W = labels.shape
    p = SspDetEvalParams(H, W, float(np.float32(remove_zero)), int(r2), float(np.float32(prob_thresh)), int(bool(simplified)))
    return labels, p


def _det_eval_ws(lib, p, B, cap, ws, device):
    wsb = lib.ssp_det_eval_workspace_bytes(C.byref(p), int(B), int(cap))
    if wsb == 0:
        _check(-1)
    if ws is None or ws.numel() < wsb:
        ws = torch.empty(wsb, dtype=torch.uint8, device=device)
    return ws


def op_detector_tp_fp(prob, labels, keys, state, remove_zero=1e-4, r2=4, prob_thresh=0.5, simplified=False, ws=None):
    """compute_tp_fp for one batch on the device (ssp_op_det_tp_fp).  prob: float32 [B,H,W] (or [B,1,H,W]), labels: float32 or
    uint8 of the same shape; the pixels with prob > remove_zero are appended to `keys` (int64 [capacity]) as records
    prob bits << 32 | record << 1 | tp, and `state` (detector_eval_state) is advanced: records, n_gt, overflow flag and the
    d2 histogram of compute_loc_error.  r2: detector_eval_r2(distance_thresh).  Returns the workspace (pass it back as `ws`
    to reuse it).  No host synchronisation."""
    lib = load_library()
    _need_gpu(prob, "prob")
    labels, p = _det_eval_args(labels, keys, state, remove_zero, r2, prob_thresh, simplified)
    B, H, W = labels.shape
    if prob.dtype != torch.float32 or prob.numel() != labels.numel() or tuple(prob.shape[-2:]) != (H, W):
        raise ValueError("prob must be float32 with the labels' shape [%d,%d,%d]" % (B, H, W))
    ws = _det_eval_ws(lib, p, B, 0, ws, prob.device)
    with torch.cuda.device(prob.device):
        _check(lib.ssp_op_det_tp_fp(_ptr(prob), _ptr(labels), int(labels.dtype == torch.uint8), C.byref(p), B, _ptr(ws),
                                    _ptr(keys), keys.numel(), _ptr(state), _stream()))
    return ws


def op_detector_tp_fp_points(pts, count, labels, keys, state, remove_zero=1e-4, r2=4, prob_thresh=0.5, simplified=False, ws=None):
    """op_detector_tp_fp for point lists (ssp_op_det_tp_fp_points): pts float32 [B,cap,5] rows (x, y, confidence, ..) with count
    int32 [B], as Engine.describe_points / op_heatmap_points produce them.  The rows < count with confidence > remove_zero are
    the candidates, in list order; rows outside the image are skipped and counted in state word DET_EVAL_OUTSIDE."""
    lib = load_library()
    labels, p = _det_eval_args(labels, keys, state, remove_zero, r2, prob_thresh, simplified)
    B = labels.shape[0]
    _tensor(pts, "pts", torch.float32, (B, (1, None), 5), "cap >= 1 rows (x, y, confidence, sx, sy) per image of labels")
    _count(count, "count", B)
    cap = pts.shape[1]
    ws = _det_eval_ws(lib, p, B, cap, ws, pts.device)
    with torch.cuda.device(pts.device):
        _check(lib.ssp_op_det_tp_fp_points(_ptr(pts), _ptr(count), cap, _ptr(labels), int(labels.dtype == torch.uint8),
                                           C.byref(p), B, _ptr(ws), _ptr(keys), keys.numel(), _ptr(state), _stream()))
    return ws


def op_detector_pr_curve(sorted_keys, state):
    """compute_pr + compute_mAP over keys sorted in descending order (ssp_op_det_pr_curve; torch.sort(keys[:n], descending=True)
    is the sort: the keys are unique).  Returns device tensors {"prob": float32 [n], "tp": uint8 [n], "precision", "recall":
    float64 [n+2], "mAP": float64 [1]}."""
    lib = load_library()
    _tensor(sorted_keys, "sorted_keys", torch.int64, (None,))
    _count(state, "state", DET_EVAL_STATE_WORDS, torch.int64)
    n, dev = sorted_keys.numel(), sorted_keys.device
    wsb = lib.ssp_det_pr_curve_workspace_bytes(n)
    if wsb == 0:
        _check(-1)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    out = {"prob": torch.empty(n, dtype=torch.float32, device=dev), "tp": torch.empty(n, dtype=torch.uint8, device=dev),
           "precision": torch.empty(n + 2, dtype=torch.float64, device=dev),
           "recall": torch.empty(n + 2, dtype=torch.float64, device=dev), "mAP": torch.empty(1, dtype=torch.float64, device=dev)}
    with torch.cuda.device(dev):
        _check(lib.ssp_op_det_pr_curve(_ptr(sorted_keys) if n else None, n, _ptr(state), _ptr(ws), _ptr(out["prob"]) if n else None,
                                       _ptr(out["tp"]) if n else None, _ptr(out["precision"]), _ptr(out["recall"]),
                                       _ptr(out["mAP"]), _stream()))
    return out


def _eval_points(pts, counts, name, count_name):
    _tensor(pts, name, torch.float64, (None, None, 3), "rows (x, y, confidence)")
    _count(counts, count_name, pts.shape[0], hint="one per image of " + name)
    if not 1 <= pts.shape[1] <= MATCH_MAX_POINTS:
        raise ValueError("%s: 1 <= cap <= %d points per image (got %d)" % (name, MATCH_MAX_POINTS, pts.shape[1]))


def op_eval_repeatability(pts1, n1, pts2, n2, hom, hom_inv, height, width, keep_k=1000, dist_thresh=3.0, pair_stride=1,
                          n_pairs=None):
    """compute_repeatability (evaluations/detector_evaluation.py:153-275) and the matching score's unwarped-point count
    (evaluation.py:194-216) for P pairs on the device.  pts1, pts2: float64 [P*pair_stride, cap, 3] rows (x, y, conf),
    n1, n2: int32 counts (pair p uses entry p*pair_stride), hom / hom_inv: float64 [P,3,3] (hom_inv from np.linalg.inv).
    Returns float64 [P,8] = N1, N2, count1, count2, sum1, sum2, n_unwarped, 0 (device tensor)."""
    lib = load_library()
    _eval_points(pts1, n1, "pts1", "n1")
    _eval_points(pts2, n2, "pts2", "n2")
    cap = pts1.shape[1]
    if pts2.shape[1] != cap:
        raise ValueError("pts1 and pts2 need the same cap")
    P = n_pairs if n_pairs is not None else pts1.shape[0] // pair_stride
    if P < 1 or (P - 1) * pair_stride >= min(pts1.shape[0], pts2.shape[0]):
        raise ValueError("%d pairs at stride %d do not fit the point arrays" % (P, pair_stride))
    _tensor(hom, "hom", torch.float64, (P, 3, 3), "P from pts1, pair_stride and n_pairs")
    _tensor(hom_inv, "hom_inv", torch.float64, (P, 3, 3), "P from pts1, pair_stride and n_pairs")
    out = torch.empty(P, 8, dtype=torch.float64, device=pts1.device)
    with torch.cuda.device(pts1.device):
        _check(lib.ssp_eval_repeatability(_ptr(pts1), _ptr(n1), _ptr(pts2), _ptr(n2), cap, P, int(pair_stride), _ptr(hom),
                                          _ptr(hom_inv), int(height), int(width), int(keep_k), float(dist_thresh),
                                          _ptr(out), _stream()))
    return out


def op_eval_ransac(pts1, pts2, match, n_match, seeds, pair_stride=1, want_ap=False):
    """RANSAC homography of P pairs' matches on the device (the cv2.findHomography step of the reference's evaluation,
    restated: DESIGN.md section 13).  pts1, pts2: float64 [P*pair_stride, cap, 3] rows (x, y, conf); match: float32
    [P, cap, 3] rows (i, j, distance) as op_match_two_way returns them, n_match: int32 [P], seeds: int64 [P].
    Returns device tensors {"H": float64 [P,3,3], "mask": uint8 [P,cap], "n_inliers": int32 [P], "status": int32 [P]
    (1 = no model), "ap": float64 [P] when want_ap}."""
    lib = load_library()
    P, cap, _ = _pair_inputs(pts1, pts2, match, n_match, pair_stride, pt_stride=3)
    _count(seeds, "seeds", P, torch.int64)
    wsb = lib.ssp_eval_ransac_workspace_bytes(cap, P)
    if wsb == 0:
        _check(-1)
    dev = match.device
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    o = {"H": torch.empty(P, 3, 3, dtype=torch.float64, device=dev),
         "mask": torch.empty(P, cap, dtype=torch.uint8, device=dev),
         "n_inliers": torch.empty(P, dtype=torch.int32, device=dev),
         "status": torch.empty(P, dtype=torch.int32, device=dev)}
    if want_ap:
        o["ap"] = torch.empty(P, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _check(lib.ssp_eval_ransac(_ptr(pts1), _ptr(pts2), cap, P, int(pair_stride), _ptr(match), _ptr(n_match),
                                   _ptr(seeds), _ptr(ws), _ptr(o["H"]), _ptr(o["mask"]), _ptr(o["n_inliers"]),
                                   _ptr(o["status"]), _ptr(o.get("ap")), _stream()))
    return o


def op_epipolar_ransac(pts1, pts2, match, n_match, seeds, thresh=1.0, pair_stride=1, groups=0):
    """Fundamental-matrix RANSAC of P pairs' matches on the device (ssp_epi_ransac): b^T F a = 0 for
    a = pts1 row i, b = pts2 row j of a match.  pts1, pts2: float64 [>= (P-1)*pair_stride+1, cap, pt_stride >= 2] rows starting
    (x, y) (the evaluator's [.,cap,3] arrays or the tracker's [.,cap,2] ring); match: float32 [P, cap, 3] rows (i, j, distance)
    as op_match_two_way returns them, n_match: int32 [P], seeds: int64 [P]; thresh: the Sampson distance of an inlier in
    pixels; groups: workgroups per pair (0 = the library's choice; the result does not depend on it).
    Returns device tensors {"F": float64 [P,3,3] (unit Frobenius norm, rank 2), "mask": uint8 [P,cap], "n_inliers": int32 [P],
    "status": int32 [P] (1 = no model), "winner": int32 [P] (the hypothesis, -1), "err": float64 [P] (RMS Sampson distance
    of the inliers)}.  No host synchronisation."""
    lib = load_library()
    P, cap, _ = _pair_inputs(pts1, pts2, match, n_match, pair_stride)
    _count(seeds, "seeds", P, torch.int64)
    wsb = lib.ssp_epi_ransac_workspace_bytes(cap, P)
    if wsb == 0:
        _check(-1)
    dev = match.device
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    o = {"F": torch.empty(P, 3, 3, dtype=torch.float64, device=dev),
         "mask": torch.empty(P, cap, dtype=torch.uint8, device=dev),
         "n_inliers": torch.empty(P, dtype=torch.int32, device=dev),
         "status": torch.empty(P, dtype=torch.int32, device=dev),
         "winner": torch.empty(P, dtype=torch.int32, device=dev),
         "err": torch.empty(P, dtype=torch.float64, device=dev)}
    with torch.cuda.device(dev):
        _check(lib.ssp_epi_ransac(_ptr(pts1), _ptr(pts2), int(pts1.shape[2]), cap, P, int(pair_stride), _ptr(match),
                                  _ptr(n_match), _ptr(seeds), float(thresh), int(groups), _ptr(ws), _ptr(o["F"]),
                                  _ptr(o["mask"]), _ptr(o["n_inliers"]), _ptr(o["status"]), _ptr(o["winner"]), _ptr(o["err"]),
                                  _stream()))
    return o


def op_filter_matches(match, n_match, mask, status, n_inliers, min_inliers):
    """The match rows a geometric check kept (ssp_op_filter_matches): match float32 [P, cap, 3] (or [cap, 3] for one pair),
    n_match int32 [P], and the mask uint8 [P, cap], status int32 [P], n_inliers int32 [P] of op_epipolar_ransac or
    op_eval_ransac.  Returns (match_out, n_match_out): the rows whose mask byte is set, in order (zero rows behind them); a
    pair with status != 0 or fewer than min_inliers inliers passes through unchanged.  That decision is taken on the device:
    no host synchronisation."""
    lib = load_library()
    P, cap, m3 = _pair_inputs(None, None, match, n_match, single=True, points=False)
    _count(mask, "mask", P * cap, torch.uint8, (P, cap), "P and cap from match")
    _count(status, "status", P, hint="P from match")
    _count(n_inliers, "n_inliers", P, hint="P from match")
    out = torch.empty_like(m3)
    n_out = torch.empty(P, dtype=torch.int32, device=m3.device)
    with torch.cuda.device(m3.device):
        _check(lib.ssp_op_filter_matches(_ptr(m3), _ptr(n_match), _ptr(mask), _ptr(status), _ptr(n_inliers), int(min_inliers),
                                         cap, P, _ptr(out), _ptr(n_out), _stream()))
    return (out if match.dim() == 3 else out[0]), n_out


POSE_KEYS = ("R", "t", "E", "cand", "counts", "n_front", "status", "front", "depth", "X")
# the outputs of op_two_view_pose and op_homography_pose for P pairs of cap matches
POSE_SPEC = (("P", "cap"), {"R": (torch.float64, ("P", 3, 3)), "t": (torch.float64, ("P", 3)), "E": (torch.float64, ("P", 3, 3)),
             "cand": (torch.int32, ("P",)), "counts": (torch.int32, ("P", 4)), "n_front": (torch.int32, ("P",)),
             "status": (torch.int32, ("P",)), "front": (torch.uint8, ("P", "cap")), "depth": (torch.float64, ("P", "cap", 2)),
             "X": (torch.float64, ("P", "cap", 3)), "model": (torch.int32, ("P",)), "normal": (torch.float64, ("P", 3)),
             "normals2": (torch.float64, ("P", 2, 3))})


def op_two_view_pose(geometry, pts1, pts2, match, n_match, intrinsics, pair_stride=1):
    """The camera motion of P calibrated pairs from their epipolar check (ssp_pose_from_fundamental).
    geometry: the dict of op_epipolar_ransac ("F", "mask", "n_inliers", "status"); pts1, pts2, match, n_match, pair_stride: what
    that call was given.  intrinsics: float64 [1, 2, 4] (shared by all pairs) or [P, 2, 4] rows (fx, fy, cx, cy) of view 1 and
    view 2.  Camera model X2 = R X1 + t.  Returns device tensors {"R": float64 [P,3,3], "t": float64 [P,3] (unit length), "E":
    float64 [P,3,3] (singular values 1, 1, 0), "cand": int32 [P] (the winning candidate, -1), "counts": int32 [P,4], "n_front":
    int32 [P], "status": int32 [P] (1 = no pose, 2 = ambiguous), "front": uint8 [P,cap], "depth": float64 [P,cap,2] = (z1, z2),
    "X": float64 [P,cap,3] (the point in camera 1's frame, the baseline as the unit)}; the per-row outputs are aligned with
    the UNFILTERED match rows, as the mask is.  No host synchronisation."""
    lib = load_library()
    P, cap, _ = _pair_inputs(pts1, pts2, match, n_match, pair_stride)
    F, mask, n_inl, status = _model_inputs(geometry, "F", "geometry", P, cap)
    n_intr = _intrinsics(intrinsics, "intrinsics", (2, 4), P)
    dev = match.device
    o = _alloc(POSE_SPEC, (P, cap), dev, POSE_KEYS, zero=False)
    with torch.cuda.device(dev):
        _check(lib.ssp_pose_from_fundamental(_ptr(F), _ptr(mask), _ptr(n_inl), _ptr(status), _ptr(pts1), _ptr(pts2),
                                             int(pts1.shape[2]), cap, P, int(pair_stride), _ptr(match), _ptr(n_match),
                                             _ptr(intrinsics), n_intr, *[_ptr(o[k]) for k in POSE_KEYS], _stream()))
    return o


def pose_state(device, n_seq=None):
    """The state of a new pose chain: float64 [POSE_STATE_WORDS] (or [n_seq, .]) = (0 frames, s = 1, Rw = identity, tw = 0)."""
    st = torch.zeros(POSE_STATE_WORDS, dtype=torch.float64)
    st[1] = st[2] = st[6] = st[10] = 1.0
    return (st if n_seq is None else st.repeat(n_seq, 1)).to(device)


def pose_table(capacity, device, n_seq=None):
    """An empty trajectory table: float64 [capacity, POSE_ROW_WORDS] (or [n_seq, ., .]) of zeros."""
    shape = (capacity, POSE_ROW_WORDS) if n_seq is None else (n_seq, capacity, POSE_ROW_WORDS)
    return torch.zeros(*shape, dtype=torch.float64, device=device)


def op_pose_chain(prev, cur, match_prev, match_cur, n_match_prev, n_match_cur, state, table):
    """One frame of the scale chain and the trajectory on the device (ssp_pose_chain).  prev / cur: the
    op_two_view_pose dicts of the pairs (f-1, f) and (f, f+1) of S sequences (S = their leading dimension); match_* float32
    [S, cap, 3] and n_match_* int32 [S]: the UNFILTERED matches those calls were given (the two pairs may have different
    caps).  prev = None: there is no pair before `cur` (match_prev and n_match_prev are ignored).  state: pose_state(), table:
    pose_table(); both are updated in place: the scale s <- s * ratio (or carried), Rw <- R Rw, tw <- R tw + s t, and the row
    (Rw [9], C [3], s, n_shared, flags, ratio) is appended at row state[0].  Flag bit 0 (POSE_FLAG_NO_POSE): cur has no pose
    (the centre repeats); bit 1 (POSE_FLAG_SCALE_CARRIED): the scale was carried, not measured.  Returns (state, table).  No
    host synchronisation."""
    lib = load_library()
    S = cur["front"].shape[0]

    def pair(d, m, nm, what):  # the two pairs may have different caps
        _, cap, _ = _pair_inputs(None, None, m, nm, what="_" + what, S=(S, "S sequences from cur['front']"), points=False)
        _tensor(d["front"], "%s['front']" % what, torch.uint8, (S, cap), "cap from match_" + what)
        _tensor(d["depth"], "%s['depth']" % what, torch.float64, (S, cap, 2), "S from cur['front'], cap from match_" + what)
        _count(d["status"], "%s['status']" % what, S, hint="S from cur['front']")
        return cap

    cap = pair(cur, match_cur, n_match_cur, "cur")
    cap_prev = pair(prev, match_prev, n_match_prev, "prev") if prev is not None else 0
    _count(cur["R"], "cur['R']", S * 9, torch.float64, (S, 3, 3), "S from cur['front']")
    _count(cur["t"], "cur['t']", S * 3, torch.float64, (S, 3), "S from cur['front']")
    capacity = _chain_arrays(state, table, S)
    have = prev is not None
    with torch.cuda.device(state.device):
        _check(lib.ssp_pose_chain(_ptr(prev["front"]) if have else None, _ptr(prev["depth"]) if have else None,
                                  _ptr(prev["status"]) if have else None, _ptr(match_prev) if have else None,
                                  _ptr(n_match_prev) if have else None, cap_prev, _ptr(cur["front"]), _ptr(cur["depth"]),
                                  _ptr(cur["status"]), _ptr(cur["R"]), _ptr(cur["t"]), _ptr(match_cur), _ptr(n_match_cur), cap, S,
                                  _ptr(state), _ptr(table), capacity, _stream()))
    return state, table


# ---- homography pose and model selection ----
HOMOGRAPHY_POSE_KEYS = ("R", "t", "cand", "counts", "n_front", "status", "front", "depth", "X", "model", "normal", "normals2")


def op_homography_pose(geometry_h, pts1, pts2, match, n_match, intrinsics, prior=None, rotation_eps=0.02, normal_margin=0.01,
                       pair_stride=1, use_h=None, out=None):
    """The camera motion of P calibrated pairs from their homography (ssp_pose_from_homography): a plane
    seen twice or a camera that only rotates, the pairs a fundamental matrix does not describe.  geometry_h: the dict of
    op_eval_ransac ("H", "mask", "n_inliers", "status"); pts1, pts2, match, n_match, intrinsics, pair_stride as for
    op_two_view_pose (any pt_stride >= 2).  prior: float64 [P, 2, 3], the "normals2" of the pair before, or None.  rotation_eps:
    the spread sqrt(w1) - sqrt(w3) of the normalised homography up to which the pair is a rotation; normal_margin: the lead in
    N . prior that decides between the two poses of a plane.  use_h: int32 [P] of op_model_select or None; pairs whose entry is 0
    keep what `out` holds.  out: the dict of op_two_view_pose to write over (its "E" stays), or None for new tensors.  Returns
    `out` (or a new dict) with op_two_view_pose's keys but "E", and "model": int32 [P] (0 none, 1 plane, 2 rotation), "normal":
    float64 [P,3], "normals2": float64 [P,2,3] (the next pair's prior).  status 2 = the two poses of the plane could not be
    told apart (the one whose normal points more along the optical axis is written).  No host synchronisation."""
    lib = load_library()
    P, cap, _ = _pair_inputs(pts1, pts2, match, n_match, pair_stride)
    H, mask, n_inl, status = _model_inputs(geometry_h, "H", "geometry_h", P, cap)
    n_intr = _intrinsics(intrinsics, "intrinsics", (2, 4), P)
    if prior is not None:
        _tensor(prior, "prior", torch.float64, (P, 2, 3), "the normals2 of the pair before")
    if use_h is not None:
        _count(use_h, "use_h", P)
    if not (rotation_eps >= 0.0 and normal_margin >= 0.0):
        raise ValueError("rotation_eps and normal_margin must be non-negative")
    dev, dims = match.device, (P, cap)
    kept, new = HOMOGRAPHY_POSE_KEYS[:9], HOMOGRAPHY_POSE_KEYS[9:]  # what op_two_view_pose wrote ("E" aside), what only this call writes
    if out is None:
        if use_h is not None:
            raise ValueError("use_h needs out: the pairs that keep the fundamental matrix keep its pose")
        o = _alloc(POSE_SPEC, dims, dev, kept, zero=False)
    else:
        o, shapes = out, _shapes(POSE_SPEC, dims)
        for k in kept:  # held by shape alone, and a strided tensor is refused with the others: a ValueError
            if k not in o or o[k].shape != shapes[k] or not o[k].is_contiguous():
                raise ValueError("out[%r] must be the contiguous tensor of op_two_view_pose for these pairs" % k)
            _need_gpu(o[k], "out[%r]" % k)
    o.update(_alloc(POSE_SPEC, dims, dev, new, zero=False))
    with torch.cuda.device(dev):
        _check(lib.ssp_pose_from_homography(_ptr(H), _ptr(mask), _ptr(n_inl), _ptr(status), _ptr(pts1), _ptr(pts2),
                                            int(pts1.shape[2]), cap, P, int(pair_stride), _ptr(match), _ptr(n_match),
                                            _ptr(intrinsics), n_intr, _ptr(prior), _ptr(use_h), float(rotation_eps),
                                            float(normal_margin), *[_ptr(o[k]) for k in HOMOGRAPHY_POSE_KEYS], _stream()))
    return o


def op_model_select(geometry_f, geometry_h, pts1, pts2, match, n_match, model_ratio=0.40, pair_stride=1):
    """Whether P pairs obey their fundamental matrix or their homography (ssp_model_select).  geometry_f: the
    dict of op_epipolar_ransac, geometry_h: the dict of op_eval_ransac; pts1, pts2, match, n_match, pair_stride: what those calls
    were given (any pt_stride >= 2).  Each model is scored over the unfiltered matches by its truncated squared distances in both
    images (5.99 - d^2 below the chi-square threshold of one pixel, 5.99 for the transfer and 3.84 for the epipolar line); the
    homography is used when it has a model and the fundamental matrix has none or S_H >= model_ratio (S_H + S_F).  Returns device
    tensors {"scores": float64 [P,2] = (S_H, S_F), "use_h": int32 [P], "mask": uint8 [P,cap], "n_inliers": int32 [P], "status":
    int32 [P]}, the last three copied from the selected model.  No host synchronisation."""
    lib = load_library()
    P, cap, _ = _pair_inputs(pts1, pts2, match, n_match, pair_stride)
    F, f_mask, f_n, f_status = _model_inputs(geometry_f, "F", "geometry_f", P, cap)
    H, h_mask, h_n, h_status = _model_inputs(geometry_h, "H", "geometry_h", P, cap)
    if not 0.0 <= model_ratio <= 1.0:
        raise ValueError("0 <= model_ratio <= 1 required")
    dev = match.device
    o = {"scores": torch.empty(P, 2, dtype=torch.float64, device=dev), "use_h": torch.empty(P, dtype=torch.int32, device=dev),
         "mask": torch.empty(P, cap, dtype=torch.uint8, device=dev), "n_inliers": torch.empty(P, dtype=torch.int32, device=dev),
         "status": torch.empty(P, dtype=torch.int32, device=dev)}
    with torch.cuda.device(dev):
        _check(lib.ssp_model_select(_ptr(F), _ptr(f_mask), _ptr(f_n), _ptr(f_status), _ptr(H), _ptr(h_mask), _ptr(h_n), _ptr(h_status),
                                    _ptr(pts1), _ptr(pts2), int(pts1.shape[2]), cap, P, int(pair_stride), _ptr(match), _ptr(n_match),
                                    float(model_ratio), _ptr(o["scores"]), _ptr(o["use_h"]), _ptr(o["mask"]), _ptr(o["n_inliers"]),
                                    _ptr(o["status"]), _stream()))
    return o


# ---- landmarks from tracks ----
LANDMARK_ROW_KEYS = ("X", "n_views", "rms", "cos_parallax", "status")
LANDMARK_SPEC = (("L", "row_cap"), {"cams": (torch.float64, ("L", CAM_WORDS)), "X": (torch.float64, ("row_cap", 3)),
                 "n_views": (torch.int32, ("row_cap",)), "rms": (torch.float64, ("row_cap",)),
                 "cos_parallax": (torch.float64, ("row_cap",)), "status": (torch.int32, ("row_cap",)),
                 "landmarks": (torch.float64, ("row_cap", LANDMARK_WORDS)), "n_landmarks": (torch.int32, (1,))})


def landmark_buffers(max_length, row_cap, device):
    """The device arrays of the landmark operators for a track table of row_cap rows of max_length ids, zeroed: {"cams": float64
    [L, CAM_WORDS], "X": float64 [row_cap, 3], "n_views": int32 [row_cap], "rms", "cos_parallax": float64 [row_cap], "status":
    int32 [row_cap], "landmarks": float64 [row_cap, LANDMARK_WORDS], "n_landmarks": int32 [1], "ws": the scratch of
    op_landmarks_select}.  Pass it as `out` to keep the operators from allocating."""
    lib = load_library()
    L, row_cap = int(max_length), int(row_cap)
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("landmark_buffers needs a HIP device: the MI355X path has no CPU fallback")
    wsb = lib.ssp_landmark_workspace_bytes(L, row_cap)
    if wsb == 0:
        _check(-1)
    out = _alloc(LANDMARK_SPEC, (L, row_cap), device)
    out["ws"] = torch.empty(wsb, dtype=torch.uint8, device=device)
    return out


def _landmark_out(out, what, keys, L, row_cap, device):
    if out is None:
        return landmark_buffers(L, row_cap, device)
    return _check_family(out, what, LANDMARK_SPEC, (L, row_cap), keys, "landmark_buffers")


def op_map_window(state, table, intrinsics, max_length, n_frames=None, out=None):
    """The cameras of the max_length retained frames of one sequence (ssp_map_window).  state: float64
    [POSE_STATE_WORDS] and table: float64 [capacity, POSE_ROW_WORDS] of op_pose_chain; intrinsics: float64 [1, 4] (shared) or
    [max_length, 4] rows (fx, fy, cx, cy), one per retained frame, oldest first.  n_frames: the number of frames given so far when
    the caller counted them (the state's own count stops when the table is full); None reads the state.  Returns float64
    [max_length, CAM_WORDS] records (Rw [9], C [3], fx, fy, cx, cy, valid, 3 spare) in out["cams"]; a frame outside the newest
    consistent window, one the table does not hold, or one whose focal lengths are not finite and positive, is a zero record.
    No host synchronisation."""
    lib = load_library()
    L = int(max_length)
    if not 2 <= L <= TRACK_MAX_LENGTH:
        raise ValueError("2 <= max_length <= %d required (got %d)" % (TRACK_MAX_LENGTH, L))
    _tensor(state, "state", torch.float64, (POSE_STATE_WORDS,), "pose_state of one sequence")
    _tensor(table, "table", torch.float64, (None, POSE_ROW_WORDS), "pose_table of one sequence")
    n_intr = _intrinsics(intrinsics, "intrinsics", (4,), L)
    if n_frames is not None and int(n_frames) < 0:
        raise ValueError("n_frames must be non-negative (None: the state's count)")
    if out is None:
        out = _alloc(LANDMARK_SPEC, (L, 0), state.device, ("cams",))
    cams = _landmark_out(out, "out", ("cams",), L, 0, state.device)["cams"]
    with torch.cuda.device(state.device):
        _check(lib.ssp_map_window(_ptr(state), _ptr(table), int(table.shape[0]), _ptr(intrinsics), n_intr, L,
                                  -1 if n_frames is None else int(n_frames), _ptr(cams), _stream()))
    return cams


def _window_inputs(table, pts, first_slot, cams):
    """A track table with its window's point ring and cameras, as the triangulation and the bundle adjustment take them."""
    L, point_cap, row_cap = table["L"], table["point_cap"], table["row_cap"]
    _tensor(table["ids"], "table['ids']", torch.int32, (row_cap, L), "track_table")
    _count(table["state"], "table['state']", 2 + L)
    _tensor(pts, "pts", torch.float64, (L, point_cap, 2), "L and point_cap of table")
    _tensor(cams, "cams", torch.float64, (L, CAM_WORDS), "op_map_window")
    if not 0 <= int(first_slot) < L:
        raise ValueError("0 <= first_slot < %d required (got %d)" % (L, first_slot))
    return L, point_cap, row_cap


def op_triangulate_tracks(table, pts, first_slot, cams, min_views=2, min_parallax_deg=1.0, max_reproj=2.0, out=None):
    """One point in the world frame per row of a track table (ssp_op_triangulate_tracks).  table: the dict
    of track_table / op_track_update; pts: float64 [L, point_cap, 2] ring of (x, y), retained frame c in slot (first_slot + c) %
    L; cams: float64 [L, CAM_WORDS] of op_map_window.  min_views >= 2 observations, min_parallax_deg: the largest angle between
    two rays of the track must reach it (its cosine is taken here, on the host), max_reproj: pixels of rms reprojection error.
    Returns the per-row device tensors {"X": float64 [row_cap, 3], "n_views": int32, "rms": float64, "cos_parallax": float64,
    "status": int32 [row_cap] (LANDMARK_OK, _FEW_VIEWS, _DEGENERATE, _BEHIND, _REPROJ)} aligned with the table's rows (`out`: a
    landmark_buffers dict; rows at or past the table's n_rows are left as they were).  No host synchronisation."""
    lib = load_library()
    L, point_cap, row_cap = _window_inputs(table, pts, first_slot, cams)
    if int(min_views) < 2:
        raise ValueError("min_views >= 2 required (got %d)" % min_views)
    if not (0.0 <= float(min_parallax_deg) <= 180.0) or not float(max_reproj) >= 0.0:
        raise ValueError("0 <= min_parallax_deg <= 180 and max_reproj >= 0 required")
    out = _landmark_out(out, "out", LANDMARK_ROW_KEYS, L, row_cap, pts.device)
    with torch.cuda.device(pts.device):
        _check(lib.ssp_op_triangulate_tracks(_ptr(table["ids"]), _ptr(table["state"]), _ptr(pts), int(first_slot), _ptr(cams), L,
                                             point_cap, row_cap, int(min_views), math.cos(math.radians(float(min_parallax_deg))),
                                             float(max_reproj), *[_ptr(out[k]) for k in LANDMARK_ROW_KEYS], _stream()))
    return {k: out[k] for k in LANDMARK_ROW_KEYS}


def op_landmarks_select(table, rows, out=None):
    """The accepted rows of op_triangulate_tracks in table order (ssp_op_landmarks_select): (landmarks float64 [row_cap,
    LANDMARK_WORDS] rows (track id, X, Y, Z, n_views, rms, cos_parallax, index of the track's point in the newest frame or -1),
    n_landmarks int32 [1]) as device tensors.  rows: the dict op_triangulate_tracks returned for `table`; `out`: a
    landmark_buffers dict.  No host synchronisation."""
    lib = load_library()
    L, point_cap, row_cap = table["L"], table["point_cap"], table["row_cap"]
    dev = table["ids"].device
    _landmark_out(rows, "rows", LANDMARK_ROW_KEYS, L, row_cap, dev)
    for k in ("ids", "tid", "state"):
        _need_gpu(table[k], "table[%r]" % k)
    if out is None:
        out = landmark_buffers(L, row_cap, dev)
    _landmark_out(out, "out", ("landmarks", "n_landmarks"), L, row_cap, dev)
    if "ws" not in out:
        raise ValueError("out must be the dict of landmark_buffers (no 'ws')")
    _need_gpu(out["ws"], "out['ws']")
    if out["ws"].numel() < lib.ssp_landmark_workspace_bytes(L, row_cap):
        raise ValueError("out['ws'] is smaller than ssp_landmark_workspace_bytes(%d, %d)" % (L, row_cap))
    with torch.cuda.device(dev):
        _check(lib.ssp_op_landmarks_select(_ptr(table["ids"]), _ptr(table["tid"]), _ptr(table["state"]), _ptr(rows["status"]),
                                           _ptr(rows["X"]), _ptr(rows["n_views"]), _ptr(rows["rms"]), _ptr(rows["cos_parallax"]), L,
                                           point_cap, row_cap, _ptr(out["ws"]), _ptr(out["landmarks"]), _ptr(out["n_landmarks"]),
                                           _stream()))
    return out["landmarks"], out["n_landmarks"]


def landmarks_to_numpy(landmarks, n_landmarks):
    """Device (landmarks, n_landmarks) of op_landmarks_select -> float64 [M, LANDMARK_WORDS] (one host synchronisation)."""
    return landmarks[:int(n_landmarks.item())].cpu().numpy()


# ---- absolute pose from landmarks ----
PNP_KEYS = ("Rw", "C", "mask", "n_inliers", "winner", "rms", "status")
PNP_SPEC = (("P", "cap"), {"corr": (torch.float64, ("P", "cap", CORR_WORDS)), "n": (torch.int32, ("P", 2)),
            "Rw": (torch.float64, ("P", 3, 3)),
            "C": (torch.float64, ("P", 3)), "mask": (torch.uint8, ("P", "cap")), "n_inliers": (torch.int32, ("P",)),
            "winner": (torch.int32, ("P",)), "rms": (torch.float64, ("P",)), "status": (torch.int32, ("P",))})


def pnp_buffers(n_problems, cap, device):
    """The device arrays of the absolute-pose operators for n_problems problems of cap correspondence rows: {"corr": float64
    [n_problems, cap, CORR_WORDS], "n": int32 [n_problems, 2] (rows, valid rows), "Rw": float64 [n_problems, 3, 3], "C": float64
    [n_problems, 3], "mask": uint8 [n_problems, cap], "n_inliers" / "winner" / "status": int32 [n_problems], "rms": float64
    [n_problems], "ws": the scratch of op_pnp_ransac}.  Pass it as `out` to keep the operators from allocating."""
    lib = load_library()
    P, cap = int(n_problems), int(cap)
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("pnp_buffers needs a HIP device: the MI355X path has no CPU fallback")
    if not 1 <= cap <= MATCH_MAX_POINTS:
        raise ValueError("1 <= cap <= %d rows per problem (got %d)" % (MATCH_MAX_POINTS, cap))
    wsb = lib.ssp_pnp_workspace_bytes(P)
    if wsb == 0:
        _check(-1)
    out = _alloc(PNP_SPEC, (P, cap), device)
    out["ws"] = torch.zeros(wsb, dtype=torch.uint8, device=device)
    return out


def _pnp_out(out, keys, P, cap, device, sizes):
    if out is None:
        return pnp_buffers(P, cap, device)
    return _check_family(out, "out", PNP_SPEC, (P, cap), keys, "pnp_buffers" + sizes)


def _landmark_rows(landmarks, n_landmarks):
    """(landmarks, n_landmarks) of op_landmarks_select; returns row_cap."""
    _tensor(landmarks, "landmarks", torch.float64, (None, LANDMARK_WORDS), "op_landmarks_select")
    _count(n_landmarks, "n_landmarks", 1)
    return landmarks.shape[0]


def _frame_matches(match, n_match, pts_new, cap=None):
    """One pair's match rows against a frame's points: match float32 [cap, 3], n_match int32 [1], pts_new float64 [point_cap, >= 2];
    returns (cap, point_cap)."""
    _tensor(match, "match", torch.float32, (cap, 3), None if cap is None else "loop['cap'] rows")
    _count(n_match, "n_match", 1)
    _tensor(pts_new, "pts_new", torch.float64, (None, (2, None)), "rows starting (x, y)")
    return match.shape[0], pts_new.shape[0]


def op_landmark_matches(landmarks, n_landmarks, match, n_match, pts_new, out=None):
    """The 3-D to 2-D correspondences of a new frame (ssp_op_landmark_matches): the landmarks of the window
    ending at the previous frame (landmarks float64 [row_cap, LANDMARK_WORDS], n_landmarks int32 [1] of op_landmarks_select) joined
    with the UNFILTERED matches of the pair (previous, new) (match float32 [cap, 3] rows (i, j, distance), n_match int32 [1]) and
    the new frame's points pts_new float64 [point_cap, >= 2].  The landmark of point i is the lowest landmark row whose eighth word
    is i.  Returns (corr float64 [cap, CORR_WORDS] rows (X, Y, Z, px, py, landmark row, valid, 0) aligned with the match rows, n
    int32 [2] = (rows, valid rows)); `out`: a pnp_buffers dict of one problem (its "corr" and "n" are filled and views of them
    returned).  No host synchronisation."""
    lib = load_library()
    row_cap = _landmark_rows(landmarks, n_landmarks)
    cap, point_cap = _frame_matches(match, n_match, pts_new)
    if not (1 <= cap <= MATCH_MAX_POINTS and 1 <= point_cap <= MATCH_MAX_POINTS and 1 <= row_cap <= TRACK_MAX_LENGTH * MATCH_MAX_POINTS):
        raise ValueError("1 <= cap, point_cap <= %d and 1 <= row_cap <= %d required" % (MATCH_MAX_POINTS, TRACK_MAX_LENGTH * MATCH_MAX_POINTS))
    out = _pnp_out(out, ("corr", "n"), 1, cap, match.device, " of one problem, cap from match")
    with torch.cuda.device(match.device):
        _check(lib.ssp_op_landmark_matches(_ptr(landmarks), _ptr(n_landmarks), row_cap, _ptr(match), _ptr(n_match), cap, _ptr(pts_new),
                                           int(pts_new.shape[1]), point_cap, _ptr(out["corr"]), _ptr(out["n"]), _stream()))
    return out["corr"][0], out["n"][0]


def op_pnp_ransac(corr, n, intrinsics, seeds, thresh=2.0, min_inliers=6, groups=0, out=None):
    """The cameras of P problems from their 3-D to 2-D correspondences (ssp_pnp_ransac): a P3P RANSAC of 512
    hypotheses, a Gauss-Newton refit over the winner's inliers, the final mask.  corr: float64 [P, cap, CORR_WORDS] (or [cap, .]
    for one problem) rows (X, Y, Z, px, py, landmark row, valid, 0); n: int32 [P] rows used; intrinsics: float64 [1, 4] (shared) or
    [P, 4] rows (fx, fy, cx, cy); seeds: int64 [P]; thresh: the reprojection error of an inlier in pixels; min_inliers: what a pose
    needs (never below 4); groups: workgroups per problem (0 = the library's choice; the result does not depend on it).  Camera
    model y = Rw (X - C).  Returns device tensors {"Rw": float64 [P,3,3], "C": float64 [P,3], "mask": uint8 [P,cap], "n_inliers":
    int32 [P], "winner": int32 [P] (the hypothesis, -1), "rms": float64 [P] (pixels), "status": int32 [P] (1 = no pose: Rw = I,
    C = 0, empty mask)}; `out`: a pnp_buffers dict.  No host synchronisation."""
    lib = load_library()
    _need_gpu(corr, "corr")
    c3 = corr[None] if corr.dim() == 2 else corr
    _tensor(c3, "corr", torch.float64, (None, None, CORR_WORDS), "[cap, CORR_WORDS] for one problem")
    P, cap = c3.shape[0], c3.shape[1]
    if not 1 <= cap <= MATCH_MAX_POINTS:
        raise ValueError("1 <= cap <= %d rows per problem (got %d)" % (MATCH_MAX_POINTS, cap))
    _count(n, "n", P, hint="one per problem of corr")
    _count(seeds, "seeds", P, torch.int64)
    n_intr = _intrinsics(intrinsics, "intrinsics", (4,), P)
    if int(min_inliers) < 4:
        raise ValueError("min_inliers >= 4 required (got %d)" % int(min_inliers))
    out = _pnp_out(out, PNP_KEYS, P, cap, c3.device, ", P and cap from corr")
    if "ws" not in out or out["ws"].numel() < lib.ssp_pnp_workspace_bytes(P):
        raise ValueError("out['ws'] is smaller than ssp_pnp_workspace_bytes(%d)" % P)
    with torch.cuda.device(c3.device):
        _check(lib.ssp_pnp_ransac(_ptr(c3), _ptr(n), cap, P, _ptr(intrinsics), n_intr, _ptr(seeds), float(thresh),
                                  int(min_inliers), int(groups), _ptr(out["ws"]), *[_ptr(out[k]) for k in PNP_KEYS], _stream()))
    return {k: out[k] for k in PNP_KEYS}


def _absolute_pose(absolute, S=None, keys=("Rw", "C", "status")):
    """The op_pnp_ransac dict of S problems (None: as many as its "status" holds), its members held by their lengths; returns S."""
    for k in keys:
        if k not in absolute:
            raise ValueError("absolute must be the dict of op_pnp_ransac (no %r)" % k)
    if S is None:
        _need_gpu(absolute["status"], "absolute['status']")
        S = absolute["status"].numel()
    _count(absolute["status"], "absolute['status']", S, hint="one per sequence")
    _count(absolute["Rw"], "absolute['Rw']", S * 9, torch.float64, (S, 3, 3), "one per entry of absolute['status']")
    _count(absolute["C"], "absolute['C']", S * 3, torch.float64, (S, 3), "one per entry of absolute['status']")
    return S


def op_pose_repair(absolute, state, table):
    """The newest trajectory row and the chain state rewritten from an absolute pose (ssp_pose_repair).
    absolute: the dict of op_pnp_ransac for S problems, one per sequence; state: float64 [S, POSE_STATE_WORDS] (or
    [POSE_STATE_WORDS]) and table: float64 [S, capacity, POSE_ROW_WORDS] (or [capacity, .]) of op_pose_chain, updated in place.
    Acts on row n - 1 of a table holding 1 <= n < capacity rows when that row carries POSE_FLAG_NO_POSE or
    POSE_FLAG_SCALE_CARRIED and the absolute pose has status 0: Rw and C are replaced, tw = -(Rw C), s = the distance to the
    previous centre when that is above 1/64 of the previous s (else s is kept and POSE_FLAG_SCALE_CARRIED stays as it was),
    POSE_FLAG_NO_POSE is cleared and POSE_FLAG_ABSOLUTE set.  Otherwise nothing changes.  Returns (state, table).  No host
    synchronisation."""
    lib = load_library()
    S = _absolute_pose(absolute)
    capacity = _chain_arrays(state, table, S)
    with torch.cuda.device(state.device):
        _check(lib.ssp_pose_repair(_ptr(absolute["Rw"]), _ptr(absolute["C"]), _ptr(absolute["status"]), S, _ptr(state), _ptr(table),
                                   capacity, _stream()))
    return state, table


# ---- windowed bundle adjustment ----
BA_KEYS = ("cams", "X", "rms", "info")
BA_SPEC = (("L", "row_cap"), {"cams": (torch.float64, ("L", CAM_WORDS)), "X": (torch.float64, ("row_cap", 3)),
           "rms": (torch.float64, ("row_cap",)), "info": (torch.float64, (BA_INFO_WORDS,))})


def ba_buffers(max_length, row_cap, device):
    """The device arrays of op_bundle_adjust for a track table of row_cap rows of max_length ids, zeroed: {"cams": float64 [L,
    CAM_WORDS], "X": float64 [row_cap, 3], "rms": float64 [row_cap], "info": float64 [BA_INFO_WORDS], "ws": its scratch}.  Pass it
    as `out` to keep the operator from allocating."""
    lib = load_library()
    L, row_cap = int(max_length), int(row_cap)
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("ba_buffers needs a HIP device: the MI355X path has no CPU fallback")
    wsb = lib.ssp_ba_workspace_bytes(L, row_cap)
    if wsb == 0:
        _check(-1)
    out = _alloc(BA_SPEC, (L, row_cap), device)
    out["ws"] = torch.zeros(wsb, dtype=torch.uint8, device=device)
    return out


def op_bundle_adjust(table, pts, first_slot, cams, rows, iterations=10, out=None):
    """The cameras of the window and the accepted landmarks refined together (ssp_bundle_adjust):
    Levenberg-Marquardt on the pixel reprojection error over (w, dC) of every valid view but the first and X of every row with
    status 0, plain least squares.  table, pts, first_slot, cams: as for op_triangulate_tracks; rows: the dict it returned for
    them ("X" and "status" are read).  1 <= iterations <= BA_MAX_ITERATIONS fixes the number of launches.  Returns device tensors
    {"cams": float64 [L, CAM_WORDS] (invalid views zero), "X": float64 [row_cap, 3] (rows not used are copies), "rms": float64
    [row_cap] (0 where the row is not used), "info": float64 [BA_INFO_WORDS] = (status, cost before, cost after, n_obs, rows used,
    accepted steps, refused V solves, final lambda)}; status BA_ADJUSTED, BA_NOTHING (nothing to adjust) or BA_NO_STEP (no step
    accepted): under the last two the outputs are copies of the inputs.  `out`: a ba_buffers dict (not the inputs' own arrays).
    No host synchronisation."""
    lib = load_library()
    L, point_cap, row_cap = _window_inputs(table, pts, first_slot, cams)
    dims = (L, row_cap)
    _check_family(rows, "rows", LANDMARK_SPEC, dims, ("X", "status"), "op_triangulate_tracks")
    if not 1 <= int(iterations) <= BA_MAX_ITERATIONS:
        raise ValueError("1 <= iterations <= %d required (got %d)" % (BA_MAX_ITERATIONS, int(iterations)))
    if out is None:
        out = ba_buffers(L, row_cap, pts.device)
    _check_family(out, "out", BA_SPEC, dims, BA_KEYS, "ba_buffers")
    if "ws" not in out:
        raise ValueError("out must be the dict of ba_buffers (no 'ws')")
    _need_gpu(out["ws"], "out['ws']")
    if out["ws"].dtype != torch.uint8 or out["ws"].numel() < lib.ssp_ba_workspace_bytes(L, row_cap):
        raise ValueError("out['ws'] is smaller than ssp_ba_workspace_bytes(%d, %d)" % (L, row_cap))
    if out["cams"].data_ptr() == cams.data_ptr() or out["X"].data_ptr() == rows["X"].data_ptr():
        raise ValueError("out must not share its arrays with cams or rows['X']")
    with torch.cuda.device(pts.device):
        _check(lib.ssp_bundle_adjust(_ptr(table["ids"]), _ptr(table["state"]), _ptr(pts), int(first_slot), _ptr(cams), L, point_cap,
                                     row_cap, _ptr(rows["X"]), _ptr(rows["status"]), int(iterations), _ptr(out["cams"]),
                                     _ptr(out["X"]), _ptr(out["rms"]), _ptr(out["info"]), _ptr(out["ws"]), _stream()))
    return {k: out[k] for k in BA_KEYS}


def op_ba_apply(adjusted, state, table, max_length, n_frames=None):
    """The adjusted cameras written back into the trajectory (ssp_ba_apply).  adjusted: the dict of
    op_bundle_adjust ("info" float64 [S, BA_INFO_WORDS] and "cams" float64 [S, L, CAM_WORDS] for S sequences; the leading
    dimension may be missing for one); state: float64 [S, POSE_STATE_WORDS] and table: float64 [S, capacity, POSE_ROW_WORDS] of
    op_pose_chain, updated in place; n_frames as for op_map_window (one count for every sequence).  Acts only where info has
    status BA_ADJUSTED: every valid view c other than the first valid one, with frame f = n - L + c inside the table, gives row f
    its Rw and C and POSE_FLAG_ADJUSTED; s becomes the distance to the previous view's centre when that view is valid and the
    distance is finite and above 1/64 of the row's s; the state follows row n - 1 when that is its newest frame and the table is
    not full.  Returns (state, table).  No host synchronisation."""
    lib = load_library()
    L = int(max_length)
    if not 2 <= L <= TRACK_MAX_LENGTH:
        raise ValueError("2 <= max_length <= %d required (got %d)" % (TRACK_MAX_LENGTH, L))
    for k in ("info", "cams"):
        if k not in adjusted:
            raise ValueError("adjusted must be the dict of op_bundle_adjust (no %r)" % k)
    info, cams = adjusted["info"], adjusted["cams"]
    _need_gpu(info, "adjusted['info']")
    if info.dtype != torch.float64 or info.numel() % BA_INFO_WORDS or info.numel() == 0:
        raise ValueError("adjusted['info'] must be float64 [S, %d]" % BA_INFO_WORDS)
    S = info.numel() // BA_INFO_WORDS
    _count(cams, "adjusted['cams']", S * L * CAM_WORDS, torch.float64, (S, L, CAM_WORDS), "S from adjusted['info'], L = max_length")
    capacity = _chain_arrays(state, table, S)
    if n_frames is not None and int(n_frames) < 0:
        raise ValueError("n_frames must be non-negative (None: the states' counts)")
    with torch.cuda.device(state.device):
        _check(lib.ssp_ba_apply(_ptr(info), _ptr(cams), L, S, -1 if n_frames is None else int(n_frames), _ptr(state), _ptr(table),
                                capacity, _stream()))
    return state, table


# ---- world map ----
WORLD_MAX_ROWS = 65536  # SSP_WORLD_MAX_ROWS (include/ssp_hip.h)
WORLD_STATE_WORDS = 8  # SSP_WORLD_STATE_WORDS: n_rows, anchored, lost_frames, streak, dropped (full), dropped (tid), appended, updated
POSE_FLAG_WORLD = 16  # SSP_POSE_FLAG_WORLD: the trajectory row was rewritten from a pose against the world map
WORLD_KEYS = ("X", "desc", "tid", "n_views", "first_frame", "last_frame", "rms", "slot_of_tid", "state")
WORLD_SPEC = (("map_cap", "tid_cap"), {"X": (torch.float64, ("map_cap", 3)), "desc": (torch.float32, ("map_cap", 256)),
              "tid": (torch.int32, ("map_cap",)),
              "n_views": (torch.int32, ("map_cap",)), "first_frame": (torch.int32, ("map_cap",)), "last_frame": (torch.int32, ("map_cap",)),
              "rms": (torch.float64, ("map_cap",)), "slot_of_tid": (torch.int32, ("tid_cap",)), "state": (torch.int32, (WORLD_STATE_WORDS,))})


def world_buffers(map_cap=WORLD_MAX_ROWS, tid_cap=1 << 22, device="cuda"):
    """An empty world map of one sequence, zeroed: {"X": float64 [map_cap, 3], "desc": float32 [map_cap, 256],
    "tid" / "n_views" / "first_frame" / "last_frame": int32 [map_cap], "rms": float64 [map_cap], "slot_of_tid": int32 [tid_cap],
    "state": int32 [WORLD_STATE_WORDS] = (n_rows, anchored, lost_frames, streak, rows dropped because the map was full, rows dropped
    because tid >= tid_cap, rows appended by the last insert, rows updated by it)} plus the host-known sizes "map_cap", "tid_cap"
    and the scratch "ws" of op_world_insert and op_match_world.  Track t is in the map iff s = slot_of_tid[t] has 0 <= s < n_rows
    and tid[s] == t, so zeroed memory is an empty map and state[0] = 0 clears one."""
    lib = load_library()
    map_cap, tid_cap = int(map_cap), int(tid_cap)
    if not 1 <= map_cap <= WORLD_MAX_ROWS:
        raise ValueError("1 <= map_cap <= %d required (got %d)" % (WORLD_MAX_ROWS, map_cap))
    if not 1 <= tid_cap < 2 ** 31:
        raise ValueError("1 <= tid_cap < 2^31 required (got %d)" % tid_cap)
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("world_buffers needs a HIP device: the MI355X path has no CPU fallback")
    wsb = max(lib.ssp_match_world_workspace_bytes(map_cap, MATCH_MAX_POINTS),
              lib.ssp_world_insert_workspace_bytes(TRACK_MAX_LENGTH * MATCH_MAX_POINTS))
    if wsb == 0:
        _check(-1)
    world = _alloc(WORLD_SPEC, (map_cap, tid_cap), device)
    world.update(ws=torch.zeros(wsb, dtype=torch.uint8, device=device), map_cap=map_cap, tid_cap=tid_cap)
    return world


def _world_map(world):
    """checks a world_buffers dict; -> (map_cap, tid_cap)"""
    if not isinstance(world, dict) or any(k not in world for k in WORLD_KEYS + ("ws", "map_cap", "tid_cap")):
        raise ValueError("world must be the dict of world_buffers")
    map_cap, tid_cap = int(world["map_cap"]), int(world["tid_cap"])
    _check_family(world, "world", WORLD_SPEC, (map_cap, tid_cap), WORLD_KEYS, "world_buffers")
    _need_gpu(world["ws"], "world['ws']")
    if not 1 <= map_cap <= WORLD_MAX_ROWS or tid_cap < 1:
        raise ValueError("1 <= map_cap <= %d and tid_cap >= 1 required" % WORLD_MAX_ROWS)
    return map_cap, tid_cap


def op_world_insert(world, landmarks, n_landmarks, desc_new, count_new, table, n_frames, patience=30):
    """One frame's landmarks into the world map (ssp_op_world_insert), in place.  world: the dict of
    world_buffers; landmarks float64 [row_cap, LANDMARK_WORDS] and n_landmarks int32 [1] of op_landmarks_select for the window
    ending at the newest frame; desc_new float32 [point_cap, 256] and count_new int32 [1] of that frame; table float64 [capacity,
    POSE_ROW_WORDS] of op_pose_chain; n_frames: the frames seen so far (the newest row is n_frames - 1).  Call it after every
    rewrite of that row.  Anchor rule from the row's flag word F: ok = (F & 3) == 0; anchored' = ok and (n_rows == 0 or anchored or
    streak >= 2); while the map has rows and is not anchored lost_frames counts up and past `patience` the map is cleared.  Rows are
    inserted only when anchored': a row whose newest-frame index p has 0 <= p < count, whose track id lies in [0, tid_cap) and
    whose X is finite replaces X, n_views, rms, last_frame and the descriptor of its track's row, or is appended in landmark order
    while there is room (dropped and counted past map_cap).  Track ids must be unique within a call.  Returns world.  No host
    synchronisation."""
    lib = load_library()
    map_cap, tid_cap = _world_map(world)
    row_cap = _landmark_rows(landmarks, n_landmarks)
    _tensor(desc_new, "desc_new", torch.float32, (None, 256), "unit rows of the newest frame")
    _count(count_new, "count_new", 1)
    _tensor(table, "table", torch.float64, (None, POSE_ROW_WORDS), "pose_table of one sequence")
    point_cap = desc_new.shape[0]
    if not (1 <= row_cap <= TRACK_MAX_LENGTH * MATCH_MAX_POINTS and 1 <= point_cap <= MATCH_MAX_POINTS):
        raise ValueError("1 <= row_cap <= %d and 1 <= point_cap <= %d required" % (TRACK_MAX_LENGTH * MATCH_MAX_POINTS, MATCH_MAX_POINTS))
    if int(n_frames) < 0 or int(patience) < 0:
        raise ValueError("n_frames and patience must be non-negative")
    if world["ws"].numel() < lib.ssp_world_insert_workspace_bytes(row_cap):
        raise ValueError("world['ws'] is smaller than ssp_world_insert_workspace_bytes(%d)" % row_cap)
    with torch.cuda.device(landmarks.device):
        _check(lib.ssp_op_world_insert(_ptr(landmarks), _ptr(n_landmarks), row_cap, _ptr(desc_new), _ptr(count_new), point_cap,
                                       _ptr(table), int(table.shape[0]), int(n_frames), int(patience), map_cap, tid_cap,
                                       _ptr(world["X"]), _ptr(world["desc"]), _ptr(world["tid"]), _ptr(world["n_views"]),
                                       _ptr(world["first_frame"]), _ptr(world["last_frame"]), _ptr(world["rms"]),
                                       _ptr(world["slot_of_tid"]), _ptr(world["state"]), _ptr(world["ws"]), _stream()))
    return world


def op_match_world(world, desc2, count2, nn_thresh, out=None):
    """A frame's descriptors against the whole world map (ssp_match_world): op_match_two_way's rules with
    side 1 = the map's n_rows rows (world["state"][0] on the device) and side 2 = the count2 (int32 [1]) rows of desc2 (float32
    [cap, 256] unit rows, cap <= MATCH_MAX_POINTS).  Bit-identical to op_match_two_way wherever both apply.  Returns (match float32
    [cap, 3] rows (map row, frame row, distance) in ascending map row, n_match int32 [1]); `out`: such a pair to fill.  The map's
    "ws" is the scratch: no allocation with `out`, no host synchronisation."""
    lib = load_library()
    map_cap, _ = _world_map(world)
    if nn_thresh < 0.0:
        raise ValueError("'nn_thresh' should be non-negative")
    _tensor(desc2, "desc2", torch.float32, (None, 256), "unit rows")
    cap = desc2.shape[0]
    if not 1 <= cap <= MATCH_MAX_POINTS:
        raise ValueError("1 <= cap <= %d frame rows (got %d)" % (MATCH_MAX_POINTS, cap))
    _count(count2, "count2", 1)
    if world["ws"].numel() < lib.ssp_match_world_workspace_bytes(map_cap, cap):
        raise ValueError("world['ws'] is smaller than ssp_match_world_workspace_bytes(%d, %d)" % (map_cap, cap))
    if out is None:
        out = (torch.empty(cap, 3, dtype=torch.float32, device=desc2.device), torch.empty(1, dtype=torch.int32, device=desc2.device))
    match, n_match = out
    _tensor(match, "out[0]", torch.float32, (cap, 3), "cap rows of desc2")
    _count(n_match, "out[1]", 1)
    with torch.cuda.device(desc2.device):
        _check(lib.ssp_match_world(_ptr(world["desc"]), _ptr(world["state"]), map_cap, _ptr(desc2), _ptr(count2), cap,
                                   float(np.float32(nn_thresh)), _ptr(world["ws"]), _ptr(match), _ptr(n_match), _stream()))
    return match, n_match


def op_world_correspondences(world, match, n_match, pts_new, count_new, out=None):
    """The 3-D to 2-D correspondences of a frame against the world map (ssp_op_world_correspondences): the
    rows of op_match_world (match float32 [cap, 3], n_match int32 [1]) joined with the map's X and the frame's points pts_new
    float64 [point_cap, >= 2] (count_new int32 [1] of them).  Returns (corr float64 [cap, CORR_WORDS] rows (X, Y, Z, px, py, map
    row, valid, 0), n int32 [2] = (rows, valid rows)), the input of op_pnp_ransac; `out`: a pnp_buffers dict of one problem.  A row
    is valid iff it lies below n_match, its map row is below n_rows, its frame point below count_new and the five values are
    finite; every other row is zero.  No host synchronisation."""
    lib = load_library()
    map_cap, _ = _world_map(world)
    cap, point_cap = _frame_matches(match, n_match, pts_new)
    _count(count_new, "count_new", 1)
    if not (1 <= cap <= MATCH_MAX_POINTS and 1 <= point_cap <= MATCH_MAX_POINTS):
        raise ValueError("1 <= cap, point_cap <= %d required" % MATCH_MAX_POINTS)
    out = _pnp_out(out, ("corr", "n"), 1, cap, match.device, " of one problem, cap from match")
    with torch.cuda.device(match.device):
        _check(lib.ssp_op_world_correspondences(_ptr(world["X"]), _ptr(world["state"]), map_cap, _ptr(match), _ptr(n_match), cap,
                                                _ptr(pts_new), int(pts_new.shape[1]), _ptr(count_new), point_cap, _ptr(out["corr"]),
                                                _ptr(out["n"]), _stream()))
    return out["corr"][0], out["n"][0]


def op_world_repair(world, absolute, state, table):
    """op_pose_repair's rule with the world map's firing condition (ssp_world_repair), one sequence.
    absolute: the dict of op_pnp_ransac for the frame's correspondences against the map; state float64 [POSE_STATE_WORDS] and table
    float64 [capacity, POSE_ROW_WORDS] of op_pose_chain, updated in place.  Row n - 1 (1 <= n < capacity rows) is rewritten when
    the pose has status 0 and is finite and either the row carries POSE_FLAG_NO_POSE or POSE_FLAG_SCALE_CARRIED or the map is lost
    (it has rows and is not anchored).  The row gets POSE_FLAG_ABSOLUTE | POSE_FLAG_WORLD; the map's streak of consecutive
    rewritten frames grows by one, and a call that writes nothing zeroes it.  Returns (state, table).  No host synchronisation."""
    lib = load_library()
    map_cap, _ = _world_map(world)
    _absolute_pose(absolute, 1)
    capacity = _chain_arrays(state, table, 1)
    with torch.cuda.device(state.device):
        _check(lib.ssp_world_repair(_ptr(absolute["Rw"]), _ptr(absolute["C"]), _ptr(absolute["status"]), _ptr(state), _ptr(table),
                                    capacity, map_cap, _ptr(world["state"]), _stream()))
    return state, table


# ---- world map upkeep ----
WORLD_UPKEEP_REPORT_WORDS = 8  # SSP_WORLD_UPKEEP_REPORT_WORDS: rows before, merged, culled, evicted, rows after, fired, protected, skipped
UPKEEP_KEYS = ("report", "totals")
UPKEEP_SPEC = ((), {"report": (torch.int32, (WORLD_UPKEEP_REPORT_WORDS,)), "totals": (torch.int64, (4,))})


def world_upkeep_buffers(map_cap=WORLD_MAX_ROWS, device="cuda"):
    """The device arrays of op_world_upkeep for a map of map_cap rows, zeroed: {"ws": its scratch (the
    staging store of the compaction: about 1.1 KB per row), "report": int32 [WORLD_UPKEEP_REPORT_WORDS] of the last call, "totals":
    int64 [4] = the running sums of (merged, culled, evicted, calls), added to on the device} plus the host-known "map_cap"."""
    lib = load_library()
    map_cap = int(map_cap)
    if not 1 <= map_cap <= WORLD_MAX_ROWS:
        raise ValueError("1 <= map_cap <= %d required (got %d)" % (WORLD_MAX_ROWS, map_cap))
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("world_upkeep_buffers needs a HIP device: the MI355X path has no CPU fallback")
    wsb = lib.ssp_world_upkeep_workspace_bytes(map_cap)
    if wsb == 0:
        _check(-1)
    upkeep = _alloc(UPKEEP_SPEC, (), device)
    upkeep.update(ws=torch.zeros(wsb, dtype=torch.uint8, device=device), map_cap=map_cap)
    return upkeep


def op_world_upkeep(world, match, n_match, landmarks, n_landmarks, pts_new, count_new, table, n_frames, intrinsics, upkeep,
                    merge=True, merge_thresh=2.0, cull_age=-1, cull_min_views=3, high_water=-1, low_water=0):
    """Upkeep of the world map (ssp_op_world_upkeep), in place, right after op_world_insert and with its
    arguments: world, landmarks, n_landmarks, count_new, table, n_frames as given to the insert; match float32 [cap, 3] / n_match
    int32 [1] of op_match_world for this frame, computed before the insert; pts_new float64 [point_cap, >= 2], the frame's points;
    intrinsics float64 of 4 entries (fx, fy, cx, cy); upkeep: the dict of world_upkeep_buffers(world["map_cap"]).  With f =
    n_frames - 1, and only when the map is anchored, has rows and row f exists (else report[7] = 1 and nothing changes):
    merge: match row (r, p) whose point p is the newest observation of landmark row q with track t', r' = the slot of t', merges iff
    r' != r, last_frame[r] < f, last_frame[r'] == f and X[r] lies in front of frame f's camera and reprojects within merge_thresh
    pixels of pts_new[p]; the lower slot survives with r''s row and the smaller first_frame.  cull (cull_age >= 0): a row dies iff
    last_frame < f - cull_age and n_views < cull_min_views.  evict (high_water >= 0; 0 <= low_water <= high_water <= map_cap): when
    more than high_water rows are alive, the min(alive - low_water, rows not seen in f) rows of smallest (min(n_views, 255),
    last_frame, 65535 - slot) die.  compact: survivors keep their order, slot_of_tid follows, state[0] is the new count.
    upkeep["report"] = (rows before, merged, culled, evicted, rows after, eviction fired, rows wanted but protected, skipped);
    upkeep["totals"] += (merged, culled, evicted, 1).  Returns world.  No host synchronisation."""
    lib = load_library()
    map_cap, tid_cap = _world_map(world)
    if not isinstance(upkeep, dict) or any(k not in upkeep for k in UPKEEP_KEYS + ("ws", "map_cap")):
        raise ValueError("upkeep must be the dict of world_upkeep_buffers")
    _check_family(upkeep, "upkeep", UPKEEP_SPEC, (), UPKEEP_KEYS, "world_upkeep_buffers")
    _need_gpu(upkeep["ws"], "upkeep['ws']")
    row_cap = _landmark_rows(landmarks, n_landmarks)
    cap, point_cap = _frame_matches(match, n_match, pts_new)
    _count(count_new, "count_new", 1)
    _tensor(table, "table", torch.float64, (None, POSE_ROW_WORDS), "pose_table of one sequence")
    _count(intrinsics, "intrinsics", 4, torch.float64, hint="(fx, fy, cx, cy) of the one camera")
    if not (1 <= row_cap <= TRACK_MAX_LENGTH * MATCH_MAX_POINTS and 1 <= point_cap <= MATCH_MAX_POINTS and 1 <= cap <= MATCH_MAX_POINTS):
        raise ValueError("1 <= row_cap <= %d and 1 <= cap, point_cap <= %d required" % (TRACK_MAX_LENGTH * MATCH_MAX_POINTS,
                                                                                      MATCH_MAX_POINTS))
    if int(n_frames) < 0:
        raise ValueError("n_frames must be non-negative")
    merge_thresh = float(merge_thresh)
    if merge and not (merge_thresh >= 0.0 and np.isfinite(merge_thresh)):
        raise ValueError("merge_thresh must be finite and non-negative")
    high_water, low_water = int(high_water), int(low_water)
    if high_water >= 0 and not 0 <= low_water <= high_water <= map_cap:
        raise ValueError("0 <= low_water <= high_water <= map_cap required, or a negative high_water for no eviction (low_water %d, "
                         "high_water %d, map_cap %d)" % (low_water, high_water, map_cap))
    if upkeep["ws"].numel() < lib.ssp_world_upkeep_workspace_bytes(map_cap):
        raise ValueError("upkeep['ws'] is smaller than ssp_world_upkeep_workspace_bytes(%d)" % map_cap)
    prm = SspWorldUpkeepParams(1 if merge else 0, merge_thresh, int(cull_age), int(cull_min_views), high_water, low_water)
    with torch.cuda.device(match.device):
        _check(lib.ssp_op_world_upkeep(_ptr(match), _ptr(n_match), cap, _ptr(landmarks), _ptr(n_landmarks), row_cap, _ptr(pts_new),
                                       int(pts_new.shape[1]), _ptr(count_new), point_cap, _ptr(table), int(table.shape[0]),
                                       int(n_frames), _ptr(intrinsics), C.c_void_p(C.addressof(prm)), map_cap, tid_cap,
                                       _ptr(world["X"]), _ptr(world["desc"]), _ptr(world["tid"]), _ptr(world["n_views"]),
                                       _ptr(world["first_frame"]), _ptr(world["last_frame"]), _ptr(world["rms"]),
                                       _ptr(world["slot_of_tid"]), _ptr(world["state"]), _ptr(upkeep["report"]),
                                       _ptr(upkeep["totals"]), _ptr(upkeep["ws"]), _stream()))
    return world


# ---- world map classes ----
WORLD_CLASS_KEYS = ("votes",)
WORLD_CLASS_SPEC = (("tid_cap",), {"votes": (torch.uint16, ("tid_cap",))})


def world_class_buffers(tid_cap=1 << 22, device="cuda"):
    """The class votes of a world map, zeroed: {"votes": uint16 [tid_cap], one entry per TRACK ID: the low
    byte is the class, the high byte the vote count; zero = no class yet} plus the host-known "tid_cap" (the map's)."""
    tid_cap = int(tid_cap)
    if not 1 <= tid_cap < 2 ** 31:
        raise ValueError("1 <= tid_cap < 2^31 required (got %d)" % tid_cap)
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("world_class_buffers needs a HIP device: the MI355X path has no CPU fallback")
    classes = _alloc(WORLD_CLASS_SPEC, (tid_cap,), device)
    classes.update(tid_cap=tid_cap)
    return classes


def _world_classes(classes, tid_cap=None):
    """checks a world_class_buffers dict (against the map's tid_cap where given); -> tid_cap"""
    if not isinstance(classes, dict) or any(k not in classes for k in WORLD_CLASS_KEYS + ("tid_cap",)):
        raise ValueError("classes must be the dict of world_class_buffers")
    own = int(classes["tid_cap"])
    if own < 1 or (tid_cap is not None and own != tid_cap):
        raise ValueError("classes must be the dict of world_class_buffers(tid_cap) with the map's tid_cap%s (got %d)"
                         % ("" if tid_cap is None else " = %d" % tid_cap, own))
    _check_family(classes, "classes", WORLD_CLASS_SPEC, (own,), WORLD_CLASS_KEYS, "world_class_buffers")
    return own


def _keep_words(mask, name="map_keep"):
    """the eight 32-bit words of a class_mask as a ctypes array; None = every class"""
    words = [0xFFFFFFFF] * 8 if mask is None else [int(w) for w in mask]
    if len(words) != 8 or any(not 0 <= w < 1 << 32 for w in words):
        raise ValueError("%s must be eight 32-bit words (class_mask)" % name)
    return (C.c_uint32 * 8)(*words)


def op_track_class_votes(classes, landmarks, n_landmarks, cls_new, count_new):
    """One frame's class votes (ssp_op_track_class_votes), in place.  classes: the dict of
    world_class_buffers; landmarks float64 [row_cap, LANDMARK_WORDS], n_landmarks int32 [1] and count_new int32 [1] as given to
    op_world_insert; cls_new uint8 [point_cap]: the class of every point of the newest frame.  A landmark row of track t whose
    newest-frame index p has 0 <= p < count, with 0 <= t < tid_cap and c = cls_new[p] != CLASS_NONE, votes: no votes yet -> (c, 1);
    the same class -> one vote more (at most 255); another class -> one vote less, the class kept.  Track ids must be unique within
    a call.  Returns classes.  No host synchronisation."""
    lib = load_library()
    tid_cap = _world_classes(classes)
    row_cap = _landmark_rows(landmarks, n_landmarks)
    _tensor(cls_new, "cls_new", torch.uint8, (None,), "the classes of the newest frame's points")
    _count(count_new, "count_new", 1)
    point_cap = cls_new.shape[0]
    if not (1 <= row_cap <= TRACK_MAX_LENGTH * MATCH_MAX_POINTS and 1 <= point_cap <= MATCH_MAX_POINTS):
        raise ValueError("1 <= row_cap <= %d and 1 <= point_cap <= %d required" % (TRACK_MAX_LENGTH * MATCH_MAX_POINTS, MATCH_MAX_POINTS))
    with torch.cuda.device(landmarks.device):
        _check(lib.ssp_op_track_class_votes(_ptr(landmarks), _ptr(n_landmarks), row_cap, _ptr(cls_new), _ptr(count_new), point_cap,
                                            _ptr(classes["votes"]), tid_cap, _stream()))
    return classes


def op_world_classes(world, classes, out=None):
    """The map as a labelled point cloud (ssp_op_world_classes): uint8 [map_cap], the voted class of the
    track of every map row below n_rows (CLASS_NONE while it has no votes) and CLASS_NONE past that; `out`: such a tensor to fill.
    No host synchronisation."""
    lib = load_library()
    map_cap, tid_cap = _world_map(world)
    _world_classes(classes, tid_cap)
    if out is None:
        out = torch.empty(map_cap, dtype=torch.uint8, device=world["tid"].device)
    _tensor(out, "out", torch.uint8, (map_cap,), "map_cap of world")
    with torch.cuda.device(out.device):
        _check(lib.ssp_op_world_classes(_ptr(world["tid"]), _ptr(world["state"]), map_cap, _ptr(classes["votes"]), tid_cap, _ptr(out),
                                        _stream()))
    return out


def op_match_world_classes(world, classes, desc2, cls2, count2, nn_thresh, map_keep=None, out=None):
    """op_match_world restricted to pairs of one class (ssp_match_world_classes).  classes: the dict of
    world_class_buffers beside the map; cls2 uint8 [cap]: the class of every row of desc2; map_keep: a class_mask of the map classes
    that take part (None: all).  Map row i and frame row j are a candidate iff the class voted for row i's track equals cls2[j], is
    not CLASS_NONE and is kept; any other pair takes part in neither nearest-neighbour search.  With every class equal, known and
    kept the result is bit-identical to op_match_world's.  Returns (match, n_match) as op_match_world does.  No host
    synchronisation."""
    lib = load_library()
    map_cap, tid_cap = _world_map(world)
    _world_classes(classes, tid_cap)
    if nn_thresh < 0.0:
        raise ValueError("'nn_thresh' should be non-negative")
    keep = _keep_words(map_keep)
    _tensor(desc2, "desc2", torch.float32, (None, 256), "unit rows")
    cap = desc2.shape[0]
    if not 1 <= cap <= MATCH_MAX_POINTS:
        raise ValueError("1 <= cap <= %d frame rows (got %d)" % (MATCH_MAX_POINTS, cap))
    _tensor(cls2, "cls2", torch.uint8, (cap,), "one class per row of desc2")
    _count(count2, "count2", 1)
    if world["ws"].numel() < lib.ssp_match_world_workspace_bytes(map_cap, cap):
        raise ValueError("world['ws'] is smaller than ssp_match_world_workspace_bytes(%d, %d)" % (map_cap, cap))
    if out is None:
        out = (torch.empty(cap, 3, dtype=torch.float32, device=desc2.device), torch.empty(1, dtype=torch.int32, device=desc2.device))
    match, n_match = out
    _tensor(match, "out[0]", torch.float32, (cap, 3), "cap rows of desc2")
    _count(n_match, "out[1]", 1)
    with torch.cuda.device(desc2.device):
        _check(lib.ssp_match_world_classes(_ptr(world["desc"]), _ptr(world["tid"]), _ptr(world["state"]), map_cap,
                                           _ptr(classes["votes"]), tid_cap, _ptr(desc2), _ptr(cls2), _ptr(count2), cap, keep,
                                           float(np.float32(nn_thresh)), _ptr(world["ws"]), _ptr(match), _ptr(n_match), _stream()))
    return match, n_match


# ---- trajectory evaluation ----
TRAJ_GT_WORDS = 12  # SSP_TRAJ_GT_WORDS: the row-major 3x4 camera-to-world matrix (R | C), a row of a KITTI poses file
TRAJ_SIM_WORDS = 16  # SSP_TRAJ_SIM_WORDS: s, R [9], t [3], n_valid, status, sigma_p^2
TRAJ_STATS_WORDS = 8  # SSP_TRAJ_STATS_WORDS: n, rmse, mean, std, min, max, median, sse
TRAJ_INFO_WORDS = 4  # SSP_TRAJ_INFO_WORDS: counted, end invalid, no end, first frames inside the sequence
TRAJ_MAX_LENGTHS = 8  # SSP_TRAJ_MAX_LENGTHS
TRAJ_MAX_FRAMES = 1 << 20  # SSP_TRAJ_MAX_FRAMES
TRAJ_MAX_PROBLEMS = 65535  # SSP_TRAJ_MAX_PROBLEMS
TRAJ_MODES = {"se3": 0, "sim3": 1, "origin": 2, "origin_scale": 3}
TRAJ_OK, TRAJ_FEW, TRAJ_COLLINEAR = 0, 1, 2  # sim[14]
KITTI_LENGTHS = (100.0, 200.0, 300.0, 400.0, 500.0, 600.0, 700.0, 800.0)
TRAJ_PAIR_KEYS = ("err_t", "err_r", "valid")
TRAJ_SEG_KEYS = ("lengths", "dist", "seg", "summary", "info")
TRAJ_SPEC = (("P", "capacity", "n_first", "n_len", "n_summary", "n_stat"),
             {"sim": (torch.float64, ("P", TRAJ_SIM_WORDS)), "err_t": (torch.float64, ("P", "capacity")),
              "err_r": (torch.float64, ("P", "capacity")), "valid": (torch.int32, ("P", "capacity")),
              "lengths": (torch.float64, ("n_len",)), "dist": (torch.float64, ("P", "capacity")),
              "seg": (torch.float64, ("P", "n_first", "n_len", 4)), "summary": (torch.float64, ("P", "n_summary")),
              "info": (torch.int32, ("P", TRAJ_INFO_WORDS)), "stats": (torch.float64, ("n_stat", "P", TRAJ_STATS_WORDS))})


def _traj_dims(traj):
    if not isinstance(traj, dict) or any(k not in traj for k in ("capacity", "n_problems", "n_len", "step", "n_stat")):
        raise ValueError("traj must be the dict of traj_eval_buffers")
    n_len, step, capacity = int(traj["n_len"]), int(traj["step"]), int(traj["capacity"])
    return (int(traj["n_problems"]), capacity, -(-capacity // step), n_len, 2 + 3 * n_len, int(traj["n_stat"]))


def traj_eval_buffers(capacity, n_problems=1, n_len=len(KITTI_LENGTHS), step=10, device="cuda", n_stat=4):
    """The device arrays of the trajectory evaluation for n_problems tables of capacity rows, zeroed: "sim"
    [P, TRAJ_SIM_WORDS]; "err_t" / "err_r" float64 and "valid" int32 [P, capacity], the per-frame output of op_traj_ape or
    op_traj_rpe_delta; "lengths" [n_len], "dist" [P, capacity], "seg" [P, cdiv(capacity, step), n_len, 4], "summary" [P, 2 + 3 n_len]
    and "info" int32 [P, TRAJ_INFO_WORDS] of op_traj_rpe_segments; "stats" [n_stat, P, TRAJ_STATS_WORDS], a row of op_traj_stats per
    slot; plus the host-known "capacity", "n_problems", "n_len", "step" and "n_stat"."""
    capacity, n_problems, n_len, step, n_stat = int(capacity), int(n_problems), int(n_len), int(step), int(n_stat)
    if not 1 <= capacity <= TRAJ_MAX_FRAMES:
        raise ValueError("1 <= capacity <= %d required (got %d)" % (TRAJ_MAX_FRAMES, capacity))
    if not 1 <= n_problems <= TRAJ_MAX_PROBLEMS:
        raise ValueError("1 <= n_problems <= %d required (got %d)" % (TRAJ_MAX_PROBLEMS, n_problems))
    if not 1 <= n_len <= TRAJ_MAX_LENGTHS:
        raise ValueError("1 <= n_len <= %d required (got %d)" % (TRAJ_MAX_LENGTHS, n_len))
    if not 1 <= step <= TRAJ_MAX_FRAMES or n_stat < 1:
        raise ValueError("1 <= step <= %d and n_stat >= 1 required (got %d, %d)" % (TRAJ_MAX_FRAMES, step, n_stat))
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("traj_eval_buffers needs a HIP device: the MI355X path has no CPU fallback")
    traj = dict(capacity=capacity, n_problems=n_problems, n_len=n_len, step=step, n_stat=n_stat)
    traj.update(_alloc(TRAJ_SPEC, _traj_dims(traj), device))
    return traj


def _traj_inputs(table, n_frames, gt, index, traj, skip_flags):
    """The arguments the trajectory operators share, checked -> (P, capacity, n_gt, gt_stride).  table float64 [P, capacity,
    POSE_ROW_WORDS] (or [capacity, .] for P = 1); n_frames int32 of P entries; gt float64 [n_gt, TRAJ_GT_WORDS] shared by all tables
    or [P, n_gt, .]; index int32 [capacity] or None."""
    dims = _traj_dims(traj)
    P, capacity = dims[0], dims[1]
    _need_gpu(table, "table")
    if (table.dtype != torch.float64 or table.dim() not in (2, 3) or tuple(table.shape[-2:]) != (capacity, POSE_ROW_WORDS)
            or table.numel() != P * capacity * POSE_ROW_WORDS):
        raise ValueError("table must be float64 [%d, %d, %d] (n_problems and capacity of traj_eval_buffers; got %s %s)"
                         % (P, capacity, POSE_ROW_WORDS, str(table.dtype)[6:], list(table.shape)))
    _count(n_frames, "n_frames", P, hint="one per table")
    _need_gpu(gt, "gt")
    if gt.dtype != torch.float64 or gt.dim() not in (2, 3) or gt.shape[-1] != TRAJ_GT_WORDS or (gt.dim() == 3 and gt.shape[0] != P):
        raise ValueError("gt must be float64 [n_gt, %d] or [%d, n_gt, %d] (got %s %s)" % (TRAJ_GT_WORDS, P, TRAJ_GT_WORDS,
                                                                                       str(gt.dtype)[6:], list(gt.shape)))
    n_gt = int(gt.shape[-2])
    if not 1 <= n_gt <= TRAJ_MAX_FRAMES:
        raise ValueError("1 <= n_gt <= %d ground-truth rows required (got %d)" % (TRAJ_MAX_FRAMES, n_gt))
    if index is not None:
        _tensor(index, "index", torch.int32, (capacity,), "the ground-truth row of each frame, -1 for none")
    skip_flags = int(skip_flags)
    if skip_flags < 0:
        raise ValueError("skip_flags must be non-negative")
    return P, capacity, n_gt, (n_gt if gt.dim() == 3 else 0), skip_flags


def _traj_scale(scale, P):
    """(pointer, stride) of the scales of P problems: None (1), a sim tensor [P, TRAJ_SIM_WORDS] (its first column) or float64 [P]."""
    if scale is None:
        return None, 0
    _need_gpu(scale, "scale")
    if scale.dtype == torch.float64 and tuple(scale.shape) == (P, TRAJ_SIM_WORDS):
        return _ptr(scale), TRAJ_SIM_WORDS
    _count(scale, "scale", P, torch.float64, hint="one per table, or the sim tensor of op_traj_align")
    return _ptr(scale), 1


def op_traj_align(table, n_frames, gt, traj, index=None, mode="sim3", skip_flags=POSE_FLAG_NO_POSE):
    """The similarity between the estimated and the true camera centres (ssp_op_traj_align) -> traj["sim"]
    [P, TRAJ_SIM_WORDS] = (s, R [9], t [3], n_valid, status, sigma_p^2) with q ~ s R p + t.  mode: "se3", "sim3", "origin" (the first
    valid frame's pose) or "origin_scale".  status TRAJ_FEW / TRAJ_COLLINEAR give the identity.  No host synchronisation."""
    lib = load_library()
    if mode not in TRAJ_MODES:
        raise ValueError("mode must be one of %s (got %r)" % (sorted(TRAJ_MODES), mode))
    P, capacity, n_gt, gt_stride, skip_flags = _traj_inputs(table, n_frames, gt, index, traj, skip_flags)
    _check_family(traj, "traj", TRAJ_SPEC, _traj_dims(traj), ("sim",), "traj_eval_buffers")
    with torch.cuda.device(table.device):
        _check(lib.ssp_op_traj_align(_ptr(table), capacity, _ptr(n_frames), capacity, _ptr(gt), gt_stride, n_gt, _ptr(index), skip_flags,
                                     TRAJ_MODES[mode], P, _ptr(traj["sim"]), _stream()))
    return traj["sim"]


def op_traj_ape(table, n_frames, gt, traj, index=None, skip_flags=POSE_FLAG_NO_POSE):
    """The absolute pose error of every frame under traj["sim"] (ssp_op_traj_ape) -> (traj["err_t"], traj["err_r"], traj["valid"]),
    [P, capacity]: |q - (s R p + t)|, the angle of R_gt^T (R Rw^T) in degrees, and the frame's validity.  No host synchronisation."""
    lib = load_library()
    P, capacity, n_gt, gt_stride, skip_flags = _traj_inputs(table, n_frames, gt, index, traj, skip_flags)
    _check_family(traj, "traj", TRAJ_SPEC, _traj_dims(traj), ("sim",) + TRAJ_PAIR_KEYS, "traj_eval_buffers")
    with torch.cuda.device(table.device):
        _check(lib.ssp_op_traj_ape(_ptr(table), capacity, _ptr(n_frames), capacity, _ptr(gt), gt_stride, n_gt, _ptr(index), skip_flags, P,
                                   _ptr(traj["sim"]), _ptr(traj["err_t"]), _ptr(traj["err_r"]), _ptr(traj["valid"]), _stream()))
    return traj["err_t"], traj["err_r"], traj["valid"]


def op_traj_rpe_delta(table, n_frames, gt, traj, index=None, delta=1, scale=None, skip_flags=POSE_FLAG_NO_POSE):
    """The relative pose error between frames f and f + delta (ssp_op_traj_rpe_delta) -> (traj["err_t"], traj["err_r"],
    traj["valid"]), [P, capacity], the rotation in degrees.  scale: None (1), traj["sim"] (its s) or float64 [P]; of an alignment
    only the scale enters.  No host synchronisation."""
    lib = load_library()
    P, capacity, n_gt, gt_stride, skip_flags = _traj_inputs(table, n_frames, gt, index, traj, skip_flags)
    _check_family(traj, "traj", TRAJ_SPEC, _traj_dims(traj), TRAJ_PAIR_KEYS, "traj_eval_buffers")
    delta = int(delta)
    if not 1 <= delta <= capacity:
        raise ValueError("1 <= delta <= capacity required (delta %d, capacity %d)" % (delta, capacity))
    sp, ss = _traj_scale(scale, P)
    with torch.cuda.device(table.device):
        _check(lib.ssp_op_traj_rpe_delta(_ptr(table), capacity, _ptr(n_frames), capacity, _ptr(gt), gt_stride, n_gt, _ptr(index), skip_flags,
                                         P, sp, ss, delta, _ptr(traj["err_t"]), _ptr(traj["err_r"]), _ptr(traj["valid"]), _stream()))
    return traj["err_t"], traj["err_r"], traj["valid"]


def op_traj_rpe_segments(table, n_frames, gt, traj, index=None, scale=None, skip_flags=POSE_FLAG_NO_POSE):
    """The KITTI devkit's segment errors (ssp_op_traj_rpe_segments) for the lengths in traj["lengths"] and first frames every
    traj["step"] -> (traj["seg"], traj["summary"], traj["info"]); traj["dist"] holds the cumulative ground-truth path length.
    summary[:, 0] is the mean translation error per metre (x 100: percent), summary[:, 1] the mean rotation error in radians per
    metre.  No host synchronisation."""
    lib = load_library()
    P, capacity, n_gt, gt_stride, skip_flags = _traj_inputs(table, n_frames, gt, index, traj, skip_flags)
    _check_family(traj, "traj", TRAJ_SPEC, _traj_dims(traj), TRAJ_SEG_KEYS, "traj_eval_buffers")
    sp, ss = _traj_scale(scale, P)
    with torch.cuda.device(table.device):
        _check(lib.ssp_op_traj_rpe_segments(_ptr(table), capacity, _ptr(n_frames), capacity, _ptr(gt), gt_stride, n_gt, _ptr(index),
                                            skip_flags, P, sp, ss, _ptr(traj["lengths"]), int(traj["n_len"]), int(traj["step"]),
                                            _ptr(traj["dist"]), _ptr(traj["seg"]), _ptr(traj["summary"]), _ptr(traj["info"]), _stream()))
    return traj["seg"], traj["summary"], traj["info"]


def op_traj_stats(err, valid, out):
    """(n, rmse, mean, std, min, max, median, sse) of the valid entries of err (ssp_op_traj_stats): err float64 and valid int32
    [P, capacity], out float64 [P, TRAJ_STATS_WORDS] (a slot of traj["stats"]).  The errors are non-negative and finite where valid;
    the median is numpy.median's, selected exactly.  Returns out.  No host synchronisation."""
    lib = load_library()
    _tensor(err, "err", torch.float64, ((1, TRAJ_MAX_PROBLEMS), (1, TRAJ_MAX_FRAMES)), "[P, capacity]")
    P, capacity = int(err.shape[0]), int(err.shape[1])
    _tensor(valid, "valid", torch.int32, (P, capacity), "as err")
    _tensor(out, "out", torch.float64, (P, TRAJ_STATS_WORDS), "a slot of traj['stats']")
    with torch.cuda.device(err.device):
        _check(lib.ssp_op_traj_stats(_ptr(err), _ptr(valid), capacity, P, _ptr(out), _stream()))
    return out


# ---- loop closure ----
LOOP_MAX_EDGES = 256  # SSP_LOOP_MAX_EDGES (include/ssp_hip.h)
LOOP_EDGE_WORDS = 16  # SSP_LOOP_EDGE_WORDS: i, j, R [9], t [3], log sigma, weight
LOOP_STATE_WORDS = 8  # SSP_LOOP_STATE_WORDS: edges, last accepted frame, refused, dropped, accepted, anchor, inliers, non-finite map rows
LOOP_CAND_WORDS = 16  # SSP_LOOP_CAND_WORDS: frame, anchor, inliers, shared depths, sigma, angle of R_c, |t_c|, accepted, reason
LOOP_MAX_INNER = 8  # SSP_LOOP_MAX_INNER: both-ends-free loop edges one solve folds in
LOOP_INFO_WORDS = 8  # SSP_LOOP_INFO_WORDS: status, cost before, cost after, nodes, edges, accepted steps, edges left out, lambda
LOOP_MAX_ITERATIONS = 64  # SSP_LOOP_MAX_ITERATIONS
POSE_FLAG_LOOP = 32  # SSP_POSE_FLAG_LOOP: the trajectory row was rewritten by a loop closure
LOOP_KEYS = ("corr", "xnew", "n", "edges", "state", "cand", "Rw", "C", "sigma", "info")
LOOP_SPEC = (("cap", "capacity"), {"corr": (torch.float64, ("cap", CORR_WORDS)), "xnew": (torch.float64, ("cap", 4)), "n": (torch.int32, (3,)),
             "edges": (torch.float64, (LOOP_MAX_EDGES, LOOP_EDGE_WORDS)), "state": (torch.int32, (LOOP_STATE_WORDS,)),
             "cand": (torch.float64, (LOOP_CAND_WORDS,)), "Rw": (torch.float64, ("capacity", 9)), "C": (torch.float64, ("capacity", 3)),
             "sigma": (torch.float64, ("capacity",)), "info": (torch.float64, (LOOP_INFO_WORDS,))})


def loop_buffers(cap, capacity, device="cuda"):
    """The device arrays of the loop-closure operators for match tables of cap rows and a trajectory table of capacity rows, zeroed
    (DESIGN.md section 31): {"corr": float64 [cap, CORR_WORDS], "xnew": float64 [cap, 4], "n": int32 [3], "edges": float64
    [LOOP_MAX_EDGES, LOOP_EDGE_WORDS], "state": int32 [LOOP_STATE_WORDS], "cand": float64 [LOOP_CAND_WORDS], "Rw": float64
    [capacity, 9], "C": float64 [capacity, 3], "sigma": float64 [capacity], "info": float64 [LOOP_INFO_WORDS], "ws": the scratch of
    op_pose_graph} plus the host-known "cap" and "capacity".  Zeroed memory is an empty edge table."""
    lib = load_library()
    cap, capacity = int(cap), int(capacity)
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("loop_buffers needs a HIP device: the MI355X path has no CPU fallback")
    if not 1 <= cap <= MATCH_MAX_POINTS:
        raise ValueError("1 <= cap <= %d rows (got %d)" % (MATCH_MAX_POINTS, cap))
    if capacity < 2:
        raise ValueError("capacity >= 2 required (got %d)" % capacity)
    wsb = lib.ssp_pose_graph_workspace_bytes(capacity)
    if wsb == 0:
        _check(-1)
    loop = _alloc(LOOP_SPEC, (cap, capacity), device)
    loop.update(ws=torch.zeros(wsb, dtype=torch.uint8, device=device), cap=cap, capacity=capacity)
    return loop


def _loop_bufs(loop):
    """checks a loop_buffers dict; -> (cap, capacity)"""
    if not isinstance(loop, dict) or any(k not in loop for k in LOOP_KEYS + ("ws", "cap", "capacity")):
        raise ValueError("loop must be the dict of loop_buffers")
    cap, capacity = int(loop["cap"]), int(loop["capacity"])
    _check_family(loop, "loop", LOOP_SPEC, (cap, capacity), LOOP_KEYS, "loop_buffers")
    _need_gpu(loop["ws"], "loop['ws']")
    if not 1 <= cap <= MATCH_MAX_POINTS or capacity < 2:
        raise ValueError("1 <= cap <= %d and capacity >= 2 required" % MATCH_MAX_POINTS)
    return cap, capacity


def _loop_table(table, capacity):
    _tensor(table, "table", torch.float64, (capacity, POSE_ROW_WORDS), "pose_table of one sequence, loop['capacity'] rows")


def op_loop_correspondences(world, match, n_match, pts_new, count_new, landmarks, n_landmarks, frame, min_gap, loop):
    """op_world_correspondences restricted to OLD map rows, and the frame points' window landmarks (ssp_op_loop_correspondences;
    DESIGN.md section 31).  world, match, n_match, pts_new, count_new as for op_world_correspondences; landmarks float64 [row_cap,
    LANDMARK_WORDS] and n_landmarks int32 [1] of op_landmarks_select for the window ending at `frame`; a match row is old iff
    last_frame[map row] <= frame - min_gap.  Fills and returns (loop["corr"], loop["xnew"], loop["n"]): corr as op_pnp_ransac takes
    it (zero for every row that is not a valid old row), xnew = (X of the lowest landmark row naming the row's frame point, 1) or
    zero, n = (rows, valid old rows, valid old rows with a landmark).  No host synchronisation."""
    lib = load_library()
    map_cap, _ = _world_map(world)
    cap, _ = _loop_bufs(loop)
    _, point_cap = _frame_matches(match, n_match, pts_new, cap)
    _count(count_new, "count_new", 1)
    row_cap = _landmark_rows(landmarks, n_landmarks)
    if not (1 <= point_cap <= MATCH_MAX_POINTS and 1 <= row_cap <= TRACK_MAX_LENGTH * MATCH_MAX_POINTS):
        raise ValueError("1 <= point_cap <= %d and 1 <= row_cap <= %d required" % (MATCH_MAX_POINTS, TRACK_MAX_LENGTH * MATCH_MAX_POINTS))
    if int(frame) < 0 or int(min_gap) < 1:
        raise ValueError("frame >= 0 and min_gap >= 1 required (got %d, %d)" % (int(frame), int(min_gap)))
    with torch.cuda.device(match.device):
        _check(lib.ssp_op_loop_correspondences(_ptr(world["X"]), _ptr(world["last_frame"]), _ptr(world["state"]), map_cap, _ptr(match),
                                               _ptr(n_match), cap, _ptr(pts_new), int(pts_new.shape[1]), _ptr(count_new), point_cap,
                                               _ptr(landmarks), _ptr(n_landmarks), row_cap, int(frame), int(min_gap),
                                               _ptr(loop["corr"]), _ptr(loop["xnew"]), _ptr(loop["n"]), _stream()))
    return loop["corr"], loop["xnew"], loop["n"]


def op_loop_edge(world, absolute, table, frame, loop, min_inliers=12, cooldown=32, weight=1.0):
    """One candidate loop edge from the pose of `frame` against the old rows (ssp_loop_edge).  absolute: the
    dict of op_pnp_ransac on loop["corr"] (one problem); table float64 [loop["capacity"], POSE_ROW_WORDS].  Anchor a = the largest
    last_frame over the inlier rows; sigma = the ratio of the sums of the inliers' depths under the loop pose and of their window
    landmarks' depths under row `frame` (op_pose_chain's statistic: at least 8 shared points, finite, positive).  Accepted iff the
    pose has status 0 and is finite, inliers >= min_inliers, the scale rule holds, 0 <= a < frame, frame - (frame of the last
    accepted edge) >= cooldown and the table has room; then the row (a, frame, R, t, log sigma, weight) is appended to
    loop["edges"].  loop["state"] counts and loop["cand"] describes the candidate.  Returns (edges, state, cand).  No host
    synchronisation."""
    lib = load_library()
    map_cap, _ = _world_map(world)
    cap, capacity = _loop_bufs(loop)
    _loop_table(table, capacity)
    _absolute_pose(absolute, 1, ("Rw", "C", "mask", "status"))
    _count(absolute["mask"], "absolute['mask']", cap, torch.uint8, hint="loop['cap'] rows")
    if int(frame) < 0 or int(min_inliers) < 4 or int(cooldown) < 0:
        raise ValueError("frame >= 0, min_inliers >= 4 and cooldown >= 0 required")
    if not (float(weight) > 0.0 and np.isfinite(float(weight))):
        raise ValueError("'weight' should be finite and positive")
    with torch.cuda.device(table.device):
        _check(lib.ssp_loop_edge(_ptr(absolute["Rw"]), _ptr(absolute["C"]), _ptr(absolute["mask"]), _ptr(absolute["status"]),
                                 _ptr(loop["corr"]), _ptr(loop["xnew"]), _ptr(loop["n"]), cap, _ptr(world["last_frame"]), map_cap,
                                 _ptr(table), capacity, int(frame), int(min_inliers), int(cooldown), float(weight), _ptr(loop["edges"]),
                                 _ptr(loop["state"]), _ptr(loop["cand"]), _stream()))
    return loop["edges"], loop["state"], loop["cand"]


def op_pose_graph(table, frame, loop, iterations=10):
    """The Sim(3) pose graph over the trajectory rows a + 1 .. frame, a = the anchor of the edge the last op_loop_edge accepted
    (ssp_pose_graph): chain edges between consecutive rows as the table holds them, every stored loop edge
    ending in (a, frame], Levenberg-Marquardt of `iterations` steps whose normal equations (block tridiagonal plus one rank-7 term
    per loop edge with both ends free, at most LOOP_MAX_INNER) are solved by block cyclic reduction and the Woodbury identity.
    Fills and returns {"Rw": loop["Rw"], "C": loop["C"], "sigma": loop["sigma"], "info": loop["info"]}: copies of the table's rows
    (sigma 1) with the free rows replaced under status 0; info = (status, cost before, cost after, nodes, edges used, accepted steps,
    both-ends-free edges left out, lambda); status 1: nothing to do, 2: no step accepted.  No host synchronisation."""
    lib = load_library()
    _, capacity = _loop_bufs(loop)
    _loop_table(table, capacity)
    if int(frame) < 0:
        raise ValueError("frame >= 0 required (got %d)" % int(frame))
    if not 1 <= int(iterations) <= LOOP_MAX_ITERATIONS:
        raise ValueError("1 <= iterations <= %d required (got %d)" % (LOOP_MAX_ITERATIONS, int(iterations)))
    if loop["ws"].numel() < lib.ssp_pose_graph_workspace_bytes(capacity):
        raise ValueError("loop['ws'] is smaller than ssp_pose_graph_workspace_bytes(%d)" % capacity)
    with torch.cuda.device(table.device):
        _check(lib.ssp_pose_graph(_ptr(table), capacity, _ptr(loop["edges"]), _ptr(loop["state"]), int(frame), int(iterations),
                                  _ptr(loop["ws"]), _ptr(loop["Rw"]), _ptr(loop["C"]), _ptr(loop["sigma"]), _ptr(loop["info"]),
                                  _stream()))
    return {k: loop[k] for k in ("Rw", "C", "sigma", "info")}


def op_loop_apply(world, state, table, frame, loop):
    """The pose graph's result written back (ssp_loop_apply), in place, only under status 0: trajectory rows
    a + 1 .. frame take the corrected Rw and C, s = |C_k - C_(k-1)| when that is finite and above 1/64 of the row's s, and
    POSE_FLAG_LOOP; the chain state (float64 [POSE_STATE_WORDS]) follows row `frame` when that is its newest frame and the table is
    not full; a map row last seen in frame k of (a, frame] becomes C'_k + sigma_k R'_k^T R_k (X - C_k), and a non-finite result
    leaves it unchanged and is counted in loop["state"][7].  Returns (state, table, world).  No host synchronisation."""
    lib = load_library()
    map_cap, _ = _world_map(world)
    _, capacity = _loop_bufs(loop)
    _loop_table(table, capacity)
    _count(state, "state", POSE_STATE_WORDS, torch.float64, hint="pose_state of one sequence")
    if int(frame) < 0:
        raise ValueError("frame >= 0 required (got %d)" % int(frame))
    with torch.cuda.device(table.device):
        _check(lib.ssp_loop_apply(_ptr(loop["info"]), _ptr(loop["Rw"]), _ptr(loop["C"]), _ptr(loop["sigma"]), _ptr(loop["state"]),
                                  int(frame), _ptr(state), _ptr(table), capacity, _ptr(world["X"]), _ptr(world["last_frame"]),
                                  _ptr(world["state"]), map_cap, _stream()))
    return state, table, world


def op_eval_pixel_homographies(hn, height, width):
    """The trainer's normalised homographies (sample["homographies"]: float32 [P,3,3] on the device) as pixel matrices of a
    height x width image: (hom, hom_inv), float64 [P,3,3] device tensors.  hom = Tinv @ (Hn @ T) (homography_scaling,
    utils/utils.py:291-294, in closed form); hom_inv = adj(hom) / det(hom), which is not np.linalg.inv bit for bit
    (DESIGN.md section 21).  No host synchronisation."""
    lib = load_library()
    _tensor(hn, "hn", torch.float32, ((1, None), 3, 3))
    P = hn.shape[0]
    hom = torch.empty(P, 3, 3, dtype=torch.float64, device=hn.device)
    inv = torch.empty(P, 3, 3, dtype=torch.float64, device=hn.device)
    with torch.cuda.device(hn.device):
        _check(lib.ssp_eval_pixel_homographies(_ptr(hn), P, int(height), int(width), _ptr(hom), _ptr(inv), _stream()))
    return hom, inv


def eval_metrics_state(capacity, device):
    """(rows float64 [capacity, EVAL_ROW_WORDS], state float64 [EVAL_STATE_WORDS]) of op_eval_accumulate, zeroed = empty."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("eval_metrics_state needs a HIP device: the MI355X path has no CPU fallback")
    if int(capacity) < 1:
        raise ValueError("capacity >= 1 pairs required (got %d)" % capacity)
    return (torch.zeros(int(capacity), EVAL_ROW_WORDS, dtype=torch.float64, device=device),
            torch.zeros(EVAL_STATE_WORDS, dtype=torch.float64, device=device))


def op_eval_accumulate(rows, state, first_pair, rep=None, ransac=None, ap=None, n1=None, pair_stride=1, hom=None,
                       corner_shape=(240, 320), thresholds=(1, 3, 5, 10, 20, 50)):
    """Per-pair rows and running sums of the descriptor metrics (ssp_eval_accumulate, include/ssp_hip.h) for the P <=
    EVAL_ACC_MAX_PAIRS pairs of a call, numbered first_pair, first_pair + 1, ...  rows / state: eval_metrics_state.
    rep: float64 [P,8] of op_eval_repeatability, or None (repeatability off).  ransac: the dict of the crossCheck
    op_eval_ransac with ap (float64 [P], the nn call's), n1 (int32 image-side counts, pair p at p * pair_stride) and hom
    (float64 [P,3,3], the true pixel homographies), or None for all four (homography metrics off).  corner_shape: the
    (height, width) whose corners measure correctness.  Updates rows and state in place; no host synchronisation."""
    lib = load_library()
    _tensor(rows, "rows", torch.float64, ((1, None), EVAL_ROW_WORDS), "eval_metrics_state")
    _tensor(state, "state", torch.float64, (EVAL_STATE_WORDS,), "eval_metrics_state")
    group = (ransac, ap, n1, hom)
    if any(g is None for g in group) and not all(g is None for g in group):
        raise ValueError("ransac, ap, n1 and hom come together or not at all")
    if rep is None and ransac is None:
        raise ValueError("neither repeatability rows nor RANSAC results to accumulate")
    P = rep.shape[0] if rep is not None else ap.numel()
    if not 1 <= P <= EVAL_ACC_MAX_PAIRS:
        raise ValueError("1 <= P <= %d pairs per call (got %d)" % (EVAL_ACC_MAX_PAIRS, P))
    if int(first_pair) < 0:
        raise ValueError("first_pair >= 0 required")
    if len(thresholds) != 6 or len(corner_shape) != 2:
        raise ValueError("six thresholds and a (height, width) corner shape are required")
    src = "P from rep" if rep is not None else "P from ap"
    if rep is not None:
        _tensor(rep, "rep", torch.float64, (P, 8), "op_eval_repeatability")
    H = ninl = status = None
    if ransac is not None:
        H = _tensor(ransac["H"], "ransac['H']", torch.float64, (P, 3, 3), src)
        ninl = _tensor(ransac["n_inliers"], "ransac['n_inliers']", torch.int32, (P,), src)
        status = _tensor(ransac["status"], "ransac['status']", torch.int32, (P,), src)
        _tensor(ap, "ap", torch.float64, (P,), src)
        _tensor(hom, "hom", torch.float64, (P, 3, 3), src)
        if int(pair_stride) < 1:
            raise ValueError("pair_stride >= 1 required (got %d)" % int(pair_stride))
        _tensor(n1, "n1", torch.int32, (((P - 1) * int(pair_stride) + 1, None),), "an entry at p * pair_stride for each pair; " + src)
    thr = (C.c_double * 6)(*[float(t) for t in thresholds])
    with torch.cuda.device(rows.device):
        _check(lib.ssp_eval_accumulate(_ptr(rep), _ptr(H), _ptr(ninl), _ptr(status), _ptr(ap), _ptr(n1), int(pair_stride),
                                       _ptr(hom), P, int(corner_shape[0]), int(corner_shape[1]), thr, int(first_pair),
                                       _ptr(rows), rows.shape[0], _ptr(state), _stream()))


def points_to_numpy(pts, count, subpixel):
    """Device rows (x, y, conf, sx, sy) -> the reference's float64 [N,3] `pts` (one host synchronisation)."""
    n = int(count.item())
    a = pts[:n].cpu().numpy()
    out = np.zeros((n, 3), dtype=np.float64)
    out[:, 0], out[:, 1], out[:, 2] = a[:, 0], a[:, 1], a[:, 2]
    if subpixel:
        out[:, :2] = out[:, :2] + a[:, 3:5] - 2
    return out


# ---- pair construction for real data ----
def op_sample_homographies(B, seed, device, perspective=True, scaling=True, rotation=True, translation=True, n_scales=5,
                           n_angles=25, scaling_amplitude=0.1, perspective_amplitude_x=0.1, perspective_amplitude_y=0.1,
                           patch_ratio=0.5, max_angle=np.pi / 2, allow_artifacts=False, translation_overflow=0.0):
    """B homographies with the keyword names / defaults of utils/homographies.py:sample_homography_np, drawn on the
    device.  Returns (homographies, inv_homographies) [B,3,3] as the dataset stores them (Coco.py:342-350)."""
    lib = load_library()
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("op_sample_homographies needs a HIP device")
    p = SspHomographyParams(int(perspective), int(scaling), int(rotation), int(translation), int(allow_artifacts),
                            int(n_scales), int(n_angles), float(scaling_amplitude), float(perspective_amplitude_x),
                            float(perspective_amplitude_y), float(patch_ratio), float(max_angle), float(translation_overflow))
    h = torch.empty(B, 3, 3, dtype=torch.float32, device=device)
    inv = torch.empty_like(h)
    with torch.cuda.device(device):
        _check(lib.ssp_op_sample_homographies(int(seed), C.byref(p), B, _ptr(h), _ptr(inv), _stream()))
    return h, inv


def op_warp_labels_full(labels, hn, exact=True, outputs=(True, True, True)):
    """warpLabels(bilinear=True) on a keypoint map [B,1,H,W]: (labels [B,1,H,W], res [B,2,H,W], labels_bi [B,1,H,W]).
    Where several key points claim one pixel the winner is defined by the reference's write order, not by thread order: the
    points are taken in row-major order of the map; labels / res keep the last point that rounds to the pixel, labels_bi the
    later of the four neighbour lists (x,y), (x,y+1), (x+1,y), (x+1,y+1) and within a list the later point.  Two calls on the
    same inputs are bit-identical.  exact: see op_warp_labels.  outputs: which of the three maps to produce (None otherwise:
    the C ABI takes NULL for a map that is not wanted)."""
    lib = load_library()
    _need_gpu(labels, "labels")
    B, _, H, W = labels.shape
    lab = torch.empty_like(labels) if outputs[0] else None
    res = torch.empty(B, 2, H, W, dtype=torch.float32, device=labels.device) if outputs[1] else None
    bi = torch.empty_like(labels) if outputs[2] else None
    with torch.cuda.device(labels.device):
        if exact:
            hpx = scaled_homographies(hn, H, W).to(labels.device)
            _check(lib.ssp_op_warp_labels_full_px(_ptr(labels), _ptr(hpx), _ptr(lab), _ptr(res), _ptr(bi), B, H, W, _stream()))
        else:
            hn = hn.to(labels.device, torch.float32).contiguous()
            _check(lib.ssp_op_warp_labels_full(_ptr(labels), _ptr(hn), _ptr(lab), _ptr(res), _ptr(bi), B, H, W, _stream()))
    return lab, res, bi


def op_label_quantize(labels):
    """The reference's `*_gaussian` label maps (datasets/Coco.py:378,400): uint8 quantisation floor(x * 255) / 255 of a float map
    (the sigma-0.2 blur behind it is the identity on 8-bit data)."""
    lib = load_library()
    _need_gpu(labels, "labels")
    out = torch.empty_like(labels)
    with torch.cuda.device(labels.device):
        _check(lib.ssp_op_label_quantize(_ptr(labels), _ptr(out), labels.numel(), _stream()))
    return out


# ---- photometric augmentation of the images (utils/photometric.py) ----
def photometric_params_from_config(aug_cfg):
    """The `data.augmentation` dict of a training yaml -> SspPhotometricParams, parsed like ImgAugTransform.__init__ and
    customizedTransform.__call__ (utils/photometric.py:26-57, 109-112): a primitive is on when its key in
    `photometric.params` is truthy (the `primitives` list is never read there).  The enable fields are COUNTS, because the
    reference's parser can append one augmenter twice: with `motion_blur.max_kernel_size != 3` it assigns no augmenter and
    appends the PREVIOUS one again (count 2, no motion blur), or raises NameError when motion blur is the only primitive of
    the chain (:51-57).  Both outcomes are reproduced.  `GaussianBlur: {sigma}` as a photometric primitive is rejected.
    With `photometric.enable` false every count is zero."""
    p = SspPhotometricParams()
    p.struct_size = C.sizeof(SspPhotometricParams)
    p.shade_nb_ellipses, p.shade_transparency_lo, p.shade_transparency_hi, p.shade_kernel_lo, p.shade_kernel_hi = 20, -0.5, 0.8, 250, 350
    p.contrast_lo = p.contrast_hi = 1.0
    ph = (aug_cfg or {}).get("photometric") or {}
    if not ph.get("enable", False):
        return p
    params = ph.get("params") or {}
    last = None  # the reference's local variable `aug`
    if params.get("random_brightness", False):
        p.brightness_max_abs_change = int(params["random_brightness"]["max_abs_change"])
        p.random_brightness += 1
        last = "random_brightness"
    if params.get("random_contrast", False):
        p.contrast_lo, p.contrast_hi = (float(v) for v in params["random_contrast"]["strength_range"])
        p.random_contrast += 1
        last = "random_contrast"
    if params.get("additive_gaussian_noise", False):
        p.noise_std_lo, p.noise_std_hi = (float(v) for v in params["additive_gaussian_noise"]["stddev_range"])
        p.additive_gaussian_noise += 1
        last = "additive_gaussian_noise"
    if params.get("additive_speckle_noise", False):
        p.impulse_prob_lo, p.impulse_prob_hi = (float(v) for v in params["additive_speckle_noise"]["prob_range"])
        p.additive_speckle_noise += 1
        last = "additive_speckle_noise"
    if params.get("motion_blur", False):
        if int(params["motion_blur"]["max_kernel_size"]) == 3:
            p.motion_blur += 1
        elif last is None:
            raise NameError("name 'aug' is not defined (motion_blur.max_kernel_size != 3 assigns no augmenter: utils/photometric.py:51-57)")
        else:
            setattr(p, last, getattr(p, last) + 1)
    if params.get("GaussianBlur", False):
        raise ValueError("photometric primitive GaussianBlur {sigma} is not on the device path (no shipped training config uses it)")
    shade = params.get("additive_shade", False)
    if shade:
        shade = shade if isinstance(shade, dict) else {}
        p.shade_nb_ellipses = int(shade.get("nb_ellipses", 20))
        p.shade_transparency_lo, p.shade_transparency_hi = (float(v) for v in shade.get("transparency_range", (-0.5, 0.8)))
        p.shade_kernel_lo, p.shade_kernel_hi = (int(v) for v in shade.get("kernel_size_range", (250, 350)))
        p.additive_shade = 1
    return p


def op_photometric_draw(B, H, W, seed, params, device):
    """Every random decision of the photometric chain for B images of H x W from one seed: float32 [B, PHOTO_DRAW_STRIDE]
    (row layout: PHOTO_* above / include/ssp_hip.h).  params: SspPhotometricParams or the `data.augmentation` dict."""
    lib = load_library()
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("op_photometric_draw needs a HIP device")
    if not isinstance(params, SspPhotometricParams):
        params = photometric_params_from_config(params)
    draws = torch.empty(B, PHOTO_DRAW_STRIDE, dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        _check(lib.ssp_op_photometric_draw(int(seed) & 0xFFFFFFFFFFFFFFFF, C.byref(params), B, H, W, _ptr(draws), _stream()))
    return draws


def op_photometric_apply(img, draws):
    """ImgAugTransform + customizedTransform of img [B,1,H,W] (float32 in [0, 1]) with the rows `draws` [B, PHOTO_DRAW_STRIDE]:
    a pure function of the two (stage order and rounding: csrc/photo_kernels.hip.h)."""
    lib = load_library()
    _need_gpu(img, "img")
    _need_gpu(draws, "draws")
    B, _, H, W = img.shape
    if img.dtype != torch.float32 or draws.dtype != torch.float32 or tuple(draws.shape) != (B, PHOTO_DRAW_STRIDE):
        raise ValueError("op_photometric_apply: img float32 [B,1,H,W] and draws float32 [B,%d] required" % PHOTO_DRAW_STRIDE)
    out = torch.empty_like(img)
    with torch.cuda.device(img.device):
        _check(lib.ssp_op_photometric_apply(_ptr(img), _ptr(draws), _ptr(out), B, H, W, _stream()))
    return out


# ---- Synthetic Shapes (datasets/synthetic_dataset.py, datasets/SyntheticDataset_gaussian.py) ----
def shapes_gaussian_weights(blur_size):
    """The normalised float32 weights of cv2.GaussianBlur(img, (b, b), 0): sigma = 0.3 ((b - 1) / 2 - 1) + 0.8, weights
    exp(-(j - r)^2 / (2 sigma^2)) in float64, divided by their float64 sum, rounded to float32 (cv2's fixed tables for b <= 7
    are not used).  Computed on the host so that the device and a restatement hold the same bits."""
    b = int(blur_size)
    if b <= 1:
        return np.ones(1, np.float32)
    sigma = 0.3 * ((b - 1) * 0.5 - 1.0) + 0.8
    j = np.arange(b, dtype=np.float64) - (b - 1) // 2
    w = np.exp(-(j * j) / (2.0 * sigma * sigma))
    return (w / w.sum()).astype(np.float32)


def shapes_params_from_config(data_cfg):
    """The `data:` block of a MagicPoint yaml -> SspShapesParams: `generation` is the dataset class's default_config
    (SyntheticDataset_gaussian.py:59-73) merged with the user's, `preprocessing` its default (:74) merged likewise; the primitive
    weights are the `truncate` shares (a missing entry counts 1; a primitive outside `primitives` counts 0)."""
    d = data_cfg or {}
    gen = {"image_size": [960, 1280],
           "params": {"generate_background": {"min_kernel_size": 150, "max_kernel_size": 500, "min_rad_ratio": 0.02, "max_rad_ratio": 0.031},
                      "draw_stripes": {"transform_params": (0.1, 0.1)}, "draw_multiple_polygons": {"kernel_boundaries": (50, 100)}}}
    user = d.get("generation") or {}
    gen["image_size"] = list(user.get("image_size", gen["image_size"]))
    for k, v in (user.get("params") or {}).items():
        gen["params"][k] = dict(gen["params"].get(k, {}), **(v or {}))
    pre = dict({"resize": [240, 320], "blur_size": 11}, **(d.get("preprocessing") or {}))
    names = d.get("primitives", "all")
    names = SHAPES_PRIMITIVES if names == "all" else ([names] if isinstance(names, str) else list(names))
    for n in names:
        if n not in SHAPES_PRIMITIVES:
            raise ValueError("unknown primitive %r" % (n,))
    trunc = d.get("truncate") or {}
    p = SspShapesParams()
    p.struct_size = C.sizeof(SspShapesParams)
    p.gen_h, p.gen_w = (int(v) for v in gen["image_size"])
    p.out_h, p.out_w = (int(v) for v in pre["resize"])
    p.blur_size = int(pre["blur_size"])
    for k, n in enumerate(SHAPES_PRIMITIVES):
        p.weights[k] = float(trunc.get(n, 1.0)) if n in names else 0.0
    g = gen["params"]
    bg = g.get("generate_background", {})
    p.bg_nb_blobs = int(bg.get("nb_blobs", 100))
    p.bg_min_kernel, p.bg_max_kernel = int(bg.get("min_kernel_size", 50)), int(bg.get("max_kernel_size", 300))
    p.bg_min_rad_ratio, p.bg_max_rad_ratio = float(bg.get("min_rad_ratio", 0.01)), float(bg.get("max_rad_ratio", 0.05))
    p.lines_nb_lines = int(g.get("draw_lines", {}).get("nb_lines", 10))
    p.polygon_max_sides = int(g.get("draw_polygon", {}).get("max_sides", 8))
    mp = g.get("draw_multiple_polygons", {})
    p.multi_max_sides, p.multi_nb_polygons, p.multi_nb_blobs = int(mp.get("max_sides", 8)), int(mp.get("nb_polygons", 30)), int(mp.get("nb_blobs", 3000))
    p.multi_kernel_lo, p.multi_kernel_hi = (int(v) for v in mp.get("kernel_boundaries", (50, 100)))
    p.ellipses_nb = int(g.get("draw_ellipses", {}).get("nb_ellipses", 20))
    p.star_nb_branches = int(g.get("draw_star", {}).get("nb_branches", 6))
    cb = g.get("draw_checkerboard", {})
    p.checker_max_rows, p.checker_max_cols = int(cb.get("max_rows", 7)), int(cb.get("max_cols", 7))
    p.checker_transform[0], p.checker_transform[1] = (float(v) for v in cb.get("transform_params", (0.05, 0.15)))
    st = g.get("draw_stripes", {})
    p.stripes_max_nb_cols, p.stripes_min_width_ratio = int(st.get("max_nb_cols", 13)), float(st.get("min_width_ratio", 0.04))
    p.stripes_transform[0], p.stripes_transform[1] = (float(v) for v in st.get("transform_params", (0.05, 0.15)))
    cu = g.get("draw_cube", {})
    p.cube_min_size_ratio = float(cu.get("min_size_ratio", 0.2))
    p.cube_scale[0], p.cube_scale[1] = (float(v) for v in cu.get("scale_interval", (0.4, 0.6)))
    p.cube_trans[0], p.cube_trans[1] = (float(v) for v in cu.get("trans_interval", (0.5, 0.2)))
    p.resize_scale_y = float(np.float32(p.gen_h) / np.float32(p.out_h))
    p.resize_scale_x = float(np.float32(p.gen_w) / np.float32(p.out_w))
    if p.blur_size > SHAPES_MAX_BLUR or (p.blur_size > 1 and p.blur_size % 2 == 0):
        raise ValueError("preprocessing.blur_size must be odd and <= %d" % SHAPES_MAX_BLUR)
    for k, v in enumerate(shapes_gaussian_weights(p.blur_size)):
        p.gauss_w[k] = float(v)
    return p


_u8_lut = {}


def u8_to_unit_float(img):
    """load_as_float of a uint8 device tensor: k / 255 from a 256-entry table divided on the HOST (the device's division by a
    scalar multiplies by the reciprocal, which is not the correctly rounded float32 quotient in the last bit); one upload per device."""
    lut = _u8_lut.get(img.device)
    if lut is None:
        lut = _u8_lut[img.device] = (torch.arange(256, dtype=torch.float32) / 255.0).to(img.device)
    return lut[img.contiguous().long()]


def photometric_params_single_pass(aug_cfg):
    """photometric_params_from_config with every stage applied at most once.  The reference's parser appends the previous
    augmenter a second time when motion_blur.max_kernel_size != 3 (the shipped magicpoint yaml: 7 -> ImpulseNoise twice, no motion
    blur); the device chain applies a stage once and ssp_op_photometric_draw refuses a count of 2, so the single-view feed
    applies a doubled stage ONCE: a stated deviation."""
    p = photometric_params_from_config(aug_cfg)
    for f in ("random_brightness", "random_contrast", "additive_gaussian_noise", "additive_speckle_noise"):
        setattr(p, f, min(getattr(p, f), 1))
    return p


def op_shapes_draw(B, seed, params, device):
    """Scene tables int32 [B, SHAPES_ROW] of B Synthetic Shapes images from one seed (row layout: SHAPES_* above /
    include/ssp_hip.h).  params: SspShapesParams or the `data:` dict."""
    lib = load_library()
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("op_shapes_draw needs a HIP device")
    if not isinstance(params, SspShapesParams):
        params = shapes_params_from_config(params)
    table = torch.empty(B, SHAPES_ROW, dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        _check(lib.ssp_op_shapes_draw(int(seed) & 0xFFFFFFFFFFFFFFFF, C.byref(params), B, _ptr(table), _stream()))
    return table


def op_shapes_render(table, params):
    """Scene tables -> (image uint8 [B,1,h,w], points float32 [B, SHAPES_MAX_POINTS, 2] (x, y) scaled to (h, w), counts int32 [B]):
    a pure function of the two (rules: csrc/shapes_kernels.hip.h)."""
    lib = load_library()
    _need_gpu(table, "table")
    if table.dtype != torch.int32 or table.dim() != 2 or table.shape[1] != SHAPES_ROW:
        raise ValueError("op_shapes_render: table int32 [B,%d] required" % SHAPES_ROW)
    if not isinstance(params, SspShapesParams):
        params = shapes_params_from_config(params)
    B, dev = table.shape[0], table.device
    need = lib.ssp_shapes_workspace_bytes(C.byref(params), B)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)  # per call: torch's caching allocator orders reuse by stream
    img = torch.empty(B, 1, params.out_h, params.out_w, dtype=torch.uint8, device=dev)
    pts = torch.empty(B, SHAPES_MAX_POINTS, 2, dtype=torch.float32, device=dev)
    cnt = torch.empty(B, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _check(lib.ssp_op_shapes_render(_ptr(table), C.byref(params), B, _ptr(ws), _ptr(img), _ptr(pts), _ptr(cnt), _stream()))
    return img, pts, cnt


def op_warp_points_scatter(points, counts, H, W, hpx=None):
    """Float key points [B,N,2] (x, y) with counts [B] -> label map [B,1,H,W]: filter_points, warp with the pixel-space
    homographies hpx [B,3,3] (None: no warp), filter_points, round, clamp to (W - 1, H - 1), scatter
    (SyntheticDataset_gaussian.py:342-351, 376, 450-472)."""
    lib = load_library()
    _need_gpu(points, "points")
    _need_gpu(counts, "counts")
    B, N = points.shape[0], points.shape[1]
    if points.dtype != torch.float32 or counts.dtype != torch.int32 or tuple(points.shape) != (B, N, 2) or tuple(counts.shape) != (B,):
        raise ValueError("op_warp_points_scatter: points float32 [B,N,2] and counts int32 [B] required")
    if hpx is not None:
        hpx = hpx.to(points.device, torch.float32).contiguous()
        assert tuple(hpx.shape) == (B, 3, 3)
    out = torch.empty(B, 1, H, W, dtype=torch.float32, device=points.device)
    with torch.cuda.device(points.device):
        _check(lib.ssp_op_warp_points_scatter(_ptr(points), _ptr(counts), _ptr(hpx), _ptr(out), B, N, int(H), int(W), _stream()))
    return out


def op_sem_finalize(sem_warped, valid, n_classes=133):
    lib = load_library()
    _need_gpu(sem_warped, "sem")
    _need_gpu(valid, "valid")
    out = torch.empty(sem_warped.shape, dtype=torch.int64, device=sem_warped.device)
    with torch.cuda.device(sem_warped.device):
        _check(lib.ssp_op_sem_finalize(_ptr(sem_warped), _ptr(valid), _ptr(out), sem_warped.numel(), int(n_classes), _stream()))
    return out
