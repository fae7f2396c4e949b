"""ctypes binding of libegonn_hip.so (C ABI: include/egonn_hip.h).

The product path has NO fallback: if the HIP library is missing, or no MI355X is visible, every entry
point raises.  PyTorch is used only as the owner of device memory and of the current HIP stream.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Sequence

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libegonn_hip.so")

QUANT_CARTESIAN, QUANT_POLAR = 0, 1
FLAG_DISABLE_GLOBAL, FLAG_DISABLE_LOCAL, FLAG_IGNORE_KP_REGRESSOR, FLAG_BF16 = 1, 2, 4, 8
FLAG_POOL_SPOC, FLAG_POOL_MAC = 16, 32
MINKFPN_SPLIT_TOPDOWN = 1                 # egonn_minkfpn_forward: every top-down step as one launch on the fp16 matrix pipe
MINKFPN_BLOCKS = {'BasicBlock': 0, 'ECABasicBlock': 1}
MINKFPN_POOLING = {None: 0, 'GeM': 1, 'MAC': 2, 'SPoC': 3}

# every symbol include/egonn_hip.h declares: (name, restype, argtypes)
_P = C.c_void_p
_SIGS = [
    ("egonn_ctx_create", C.c_int, [C.POINTER(_P), C.c_int, C.c_int]),
    ("egonn_ctx_destroy", None, [_P]),
    ("egonn_last_error", C.c_char_p, []),
    ("egonn_debug_set_naive_conv", C.c_int, [_P, C.c_int]),
    ("egonn_debug_set_ksplit", C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    ("egonn_debug_set_resident", C.c_int, [_P, C.c_int, C.c_int]),
    ("egonn_debug_keep_level_features", C.c_int, [_P, C.c_int]),
    ("egonn_debug_set_trace", C.c_int, [_P]),
    ("egonn_prepare_maps", C.c_int, [_P, C.c_int, _P]),
    ("egonn_debug_rowgroup_tables", C.c_int, [_P, C.c_int, C.c_int, _P, _P, C.c_int64, C.POINTER(C.c_int64), _P]),
    ("egonn_debug_rowgroup_perm", C.c_int, [_P, C.c_int, C.c_int, _P, C.c_int64, C.POINTER(C.c_int64), _P]),
    ("egonn_debug_radix_sort_scratch_bytes", C.c_int64, [C.c_int64, C.c_int]),
    ("egonn_debug_radix_sort", C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int,
                                         C.POINTER(C.c_int32), _P, C.c_int64, _P]),
    ("egonn_debug_dense_group3", C.c_int, [_P, _P, _P, _P, _P, _P, _P]),
    ("egonn_debug_global_tail_scratch_bytes", C.c_int64, [C.c_int64]),
    ("egonn_debug_global_tail", C.c_int, [_P, _P, C.c_int, C.c_int64, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int, _P, _P, _P, C.c_int64, _P]),
    ("egonn_voxelize", C.c_int, [_P, _P, C.POINTER(C.c_int64), C.c_int, C.c_int, C.POINTER(C.c_float), _P]),
    ("egonn_ctx_reserve", C.c_int, [_P, C.c_int64, C.c_int, C.POINTER(C.c_int64)]),
    ("egonn_voxelize_device", C.c_int, [_P, _P, C.c_int64, _P, C.c_int, C.c_int, C.POINTER(C.c_float), _P]),
    ("egonn_plan_status", C.c_int, [_P, _P]),
    ("egonn_ctx_set_exact_fp32", C.c_int, [_P, C.c_int]),
    ("egonn_ctx_set_operand_autoscale", C.c_int, [_P, C.c_int]),
    ("egonn_level_capacity", C.c_int, [_P, C.c_int, C.POINTER(C.c_int64)]),
    ("egonn_graph_begin", C.c_int, [_P]),
    ("egonn_graph_end", C.c_int, [_P, C.POINTER(_P)]),
    ("egonn_graph_launch", C.c_int, [_P, _P]),
    ("egonn_graph_destroy", None, [_P]),
    ("egonn_coords_set", C.c_int, [_P, _P, C.c_int64, C.c_int, _P]),
    ("egonn_level_count", C.c_int, [_P, C.c_int, C.POINTER(C.c_int64)]),
    ("egonn_level_batch_offsets", C.c_int, [_P, C.c_int, C.POINTER(C.c_int64)]),
    ("egonn_level_coords", C.c_int, [_P, C.c_int, _P, _P]),
    ("egonn_input_index", C.c_int, [_P, _P, _P]),
    ("egonn_conv", C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, C.c_int, _P, C.c_int, _P, _P, C.c_int, _P, _P]),
    ("egonn_conv_transpose", C.c_int, [_P, C.c_int, _P, C.c_int, _P, C.c_int, _P, _P]),
    ("egonn_sparse_conv", C.c_int, [_P, C.c_int, C.c_int, _P, C.c_int, _P, C.c_int, C.c_int, _P, _P, C.c_int, _P, _P, _P]),
    ("egonn_map_groups", C.c_int, [_P, C.c_int, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64), _P]),
    ("egonn_global_avg_pool", C.c_int, [_P, C.c_int, _P, C.c_int, _P, _P]),
    ("egonn_bn_fold", C.c_int, [_P, _P, _P, _P, C.c_float, C.c_int, _P, _P, _P]),
    ("egonn_block_tail", C.c_int, [_P, C.c_int, _P, _P, C.c_int, _P, C.c_int, _P, _P]),
    ("egonn_gem", C.c_int, [_P, C.c_int, _P, C.c_int, _P, _P, _P]),
    ("egonn_global_max_pool", C.c_int, [_P, C.c_int, _P, C.c_int, _P, _P]),
    ("egonn_netvlad", C.c_int, [_P, C.c_int, _P, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int, _P, _P]),
    ("egonn_netvlad_train_forward", C.c_int, [_P, C.c_int, _P, C.c_int, C.c_int, _P, _P, _P, _P, C.c_float, C.c_float, _P, _P,
                                              _P, C.c_int, _P, _P, _P, _P, _P, _P, _P]),
    ("egonn_netvlad_train_backward", C.c_int, [_P, C.c_int, _P, C.c_int, C.c_int, _P, _P, _P, _P, C.c_int, _P, _P, _P, _P, _P,
                                               _P, _P, _P, _P, _P, _P, _P]),
    ("egonn_global_max_pool_argmax", C.c_int, [_P, C.c_int, _P, C.c_int, _P, _P, _P]),
    ("egonn_global_max_pool_backward", C.c_int, [_P, C.c_int, _P, _P, C.c_int, _P, _P]),
    ("egonn_sigmoid_gate", C.c_int, [_P, _P, _P, C.c_int64, _P, _P, _P, _P]),
    ("egonn_add", C.c_int, [_P, _P, C.c_int64, _P, _P]),
    ("egonn_gather_input", C.c_int, [_P, _P, C.c_int, _P, _P]),
    ("egonn_model_create", C.c_int, [C.POINTER(_P)]),
    ("egonn_model_destroy", None, [_P]),
    ("egonn_model_set_tensor", C.c_int, [_P, C.c_char_p, _P, C.c_int, C.POINTER(C.c_int64)]),
    ("egonn_model_finalize", C.c_int, [_P, _P]),
    ("egonn_forward", C.c_int, [_P, _P, _P, C.c_int, C.POINTER(C.c_float), C.c_int, _P, _P, _P, _P, _P]),
    ("egonn_forward_level_features", C.c_int, [_P, C.c_int, _P, C.c_int, _P]),
    ("egonn_minkfpn_finalize", C.c_int, [_P, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    ("egonn_minkfpn_out_level", C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int)]),
    ("egonn_minkfpn_forward", C.c_int, [_P, _P, C.c_int, _P, _P, _P]),
    ("egonn_topdown_step", C.c_int, [_P, C.c_int, _P, _P, _P, _P, C.c_int, C.c_int, _P, _P]),
    ("egonn_select_keypoints", C.c_int, [_P, _P, _P, _P, C.c_int, _P, _P, _P, _P, _P]),
    ("egonn_topk_rows", C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, _P]),
    ("egonn_triplet_loss_scratch_floats", C.c_int64, [C.c_int]),
    ("egonn_triplet_loss", C.c_int, [_P, C.c_int, C.c_int, _P, _P, C.c_float, _P, _P, _P, _P, _P]),
    ("egonn_nn_search", C.c_int, [_P, C.c_int64, _P, _P, C.c_int64, _P, _P, _P]),
    ("egonn_matrix_min", C.c_int, [_P, C.c_int64, C.c_int64, _P, _P, _P, _P, _P]),
    ("egonn_softmax_cross_entropy", C.c_int, [_P, C.c_int64, C.c_int64, _P, _P, _P, _P, _P]),
    ("egonn_local_loss_scratch_bytes", C.c_int64, [C.c_int, C.c_int64, C.c_int64, C.c_int]),
    ("egonn_local_loss", C.c_int, [C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int] + [_P] * 13 +
                                  [C.POINTER(C.c_float)] + [_P] * 9 + [C.c_int64, _P]),
    ("egonn_dense", C.c_int, [_P, C.c_int64, C.c_int, _P, C.c_int, _P, C.c_int, C.c_int, _P, _P]),
    ("egonn_dense_pack_fragments", C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P]),
    ("egonn_dense_pack_fragments_host", C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P]),
    ("egonn_debug_dense", C.c_int, [_P, C.c_int, C.c_int64, _P, C.c_int, C.c_int, _P, C.c_int, _P, _P, _P, _P, C.c_int, _P, C.c_int,
                                    _P, _P, C.c_int, _P, C.c_int, C.c_int, _P]),
    ("egonn_debug_dense_route", C.c_int, [C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32)]),
    ("egonn_debug_sconv_choice", C.c_int, [C.POINTER(C.c_int32), C.c_int64, C.POINTER(C.c_int32)]),
    ("egonn_dense_backward_weight", C.c_int, [_P, C.c_int, _P, C.c_int, C.c_int64, _P, _P, C.c_int64, _P]),
    ("egonn_conv_backward_weight", C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, _P, C.c_int, _P, _P,
                                             C.c_int64, _P]),
    ("egonn_col_stats", C.c_int, [C.c_int, _P, _P, _P, _P, C.c_int64, C.c_int, _P, _P, C.c_int64, _P]),
    ("egonn_bn_train_finalize", C.c_int, [_P, _P, C.c_double, C.c_int, _P, _P, C.c_float, C.c_float, _P, _P, _P, _P]),
    ("egonn_bn_backward_finalize", C.c_int, [_P, _P, C.c_double, C.c_int, _P, _P, _P, _P, _P]),
    ("egonn_affine_act", C.c_int, [_P, _P, _P, C.c_int64, C.c_int, C.c_int, _P, _P]),
    ("egonn_affine3", C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int64, C.c_int, _P, _P]),
    ("egonn_relu_backward", C.c_int, [_P, _P, C.c_int64, C.c_int, _P, _P]),
    ("egonn_contrastive_loss_scratch_floats", C.c_int64, [C.c_int]),
    ("egonn_contrastive_loss", C.c_int, [_P, C.c_int, C.c_int, _P, _P, C.c_float, C.c_float, _P, _P, _P, _P, _P]),
    ("egonn_se_gate", C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    ("egonn_se_gate_backward", C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P]),
    ("egonn_eca_gate", C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P]),
    ("egonn_eca_gate_backward", C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    ("egonn_act_backward", C.c_int, [C.c_int, _P, _P, C.c_int64, C.c_int, _P, _P]),
    ("egonn_l2_normalize", C.c_int, [_P, _P, C.c_int64, C.c_int, _P, _P]),
    ("egonn_gate_residual", C.c_int, [_P, C.c_int, _P, _P, _P, C.c_int, C.c_int, _P, _P]),
    ("egonn_gate_residual_backward", C.c_int, [_P, C.c_int, _P, _P, _P, C.c_int, _P, _P, _P]),
    ("egonn_segment_sums", C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P, _P, C.c_int, _P, _P, C.c_int64, _P]),
    ("egonn_segment_broadcast", C.c_int, [_P, C.c_int, _P, C.c_int, C.c_int, _P, _P]),
    ("egonn_gem_backward", C.c_int, [_P, C.c_int, _P, _P, _P, C.c_int, _P, _P]),
    ("egonn_filter_points_scratch_ints", C.c_int64, [C.c_int64]),
    ("egonn_filter_points", C.c_int, [_P, C.c_int64, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_float, _P, _P, _P,
                                      C.c_int64, _P]),
    ("egonn_knn", C.c_int, [_P, C.c_int64, _P, C.c_int64, C.c_int, C.c_int, _P, _P, _P, C.c_int64, _P]),
    ("egonn_recall_counts", C.c_int, [_P, _P, _P, C.c_int64, C.c_int, C.c_int, _P, C.c_int, _P, _P]),
    ("egonn_registration_scratch_bytes", C.c_int64, [C.c_int, C.c_int, C.c_int]),
    ("egonn_match_mutual_scratch_bytes", C.c_int64, [C.c_int, C.c_int]),
    ("egonn_match_mutual", C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, C.c_int64, _P]),
    ("egonn_ransac_pairs", C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_double, _P,
                                     C.c_int64, _P, _P, _P]),
    ("egonn_registration_finish", C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_double, _P,
                                            C.c_int64, _P, C.c_double, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    ("egonn_spectral_verify_scratch_bytes", C.c_int64, [C.c_int, C.c_int]),
    ("egonn_spectral_verify", C.c_int, [_P] * 6 + [C.c_int, C.c_int, C.c_double, C.c_int, C.c_double, C.c_double, _P, C.c_double,
                                        _P, C.c_int64] + [_P] * 15),
    ("egonn_voxel_downsample_scratch_bytes", C.c_int64, [C.c_int64, C.c_int]),
    ("egonn_voxel_downsample", C.c_int, [_P, C.c_int64, _P, C.c_int, C.c_double, C.POINTER(C.c_float), _P, _P, _P, _P, _P,
                                         C.c_int64, _P]),
    ("egonn_icp_scratch_bytes", C.c_int64, [C.c_int64, C.c_int64, C.c_int]),
    ("egonn_icp_pairs", C.c_int, [_P, C.c_int64, _P, _P, C.c_int64, _P, C.c_int, _P, C.c_double, C.c_int, C.c_double, C.c_double,
                                  _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int64, _P]),
    ("egonn_estimate_normals_scratch_bytes", C.c_int64, [C.c_int64, C.c_int]),
    ("egonn_estimate_normals", C.c_int, [_P, C.c_int64, _P, C.c_int, C.c_int, _P, _P, _P, _P, _P, C.c_int64, _P]),
    ("egonn_icp_plane_scratch_bytes", C.c_int64, [C.c_int64, C.c_int64, C.c_int]),
    ("egonn_icp_plane_pairs", C.c_int, [_P, C.c_int64, _P, _P, C.c_int64, _P, _P, C.c_int, _P, C.c_double, C.c_int, C.c_double,
                                        C.c_double, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int64, _P]),
    ("egonn_augment_scratch_bytes", C.c_int64, [C.c_int64, C.c_int]),
    ("egonn_augment_points", C.c_int, [_P, C.c_int64, _P, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int64, _P]),
    ("egonn_scan_context", C.c_int, [_P, C.c_int64, _P, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, _P, _P, _P]),
    ("egonn_scan_context_ringkey", C.c_int, [_P, C.c_int64, C.c_int, C.c_int, _P, _P]),
    ("egonn_scan_context_distance", C.c_int, [_P, C.c_int64, _P, C.c_int64, C.c_int, C.c_int, _P, C.c_int, _P, _P, _P]),
    ("egonn_scan_context_rerank", C.c_int, [_P, _P, _P, C.c_int64, C.c_int, _P, _P, _P, _P]),
    ("egonn_radius_count", C.c_int, [_P, C.c_int64, _P, C.c_int64, C.POINTER(C.c_double), C.c_int, C.c_int, _P, _P]),
    ("egonn_radius_fill", C.c_int, [_P, C.c_int64, _P, C.c_int64, C.c_double, C.c_int, _P, _P, C.c_int64, _P, _P]),
    ("egonn_pair_masks", C.c_int, [_P, C.c_int, _P, _P, C.c_int64, _P, _P, C.c_int64, C.c_int64, _P, _P, _P, _P]),
    ("egonn_relative_poses", C.c_int, [_P, C.c_int64, _P, _P, C.c_int64, C.c_int, _P, _P, _P]),
    ("egonn_gather_clouds", C.c_int, [_P, C.c_int64, _P, C.c_int64, _P, C.c_int, _P, C.c_int64, _P, _P, _P]),
    ("egonn_voxel_map_integrate_scratch_bytes", C.c_int64, [C.c_int64, C.c_int]),
    ("egonn_voxel_map_integrate", C.c_int, [_P, C.c_int64, _P, C.c_int64, _P, _P, C.c_int, C.POINTER(C.c_double), C.c_double,
                                            C.c_int64, _P, _P, _P, _P, C.c_int64, _P, _P, _P, C.c_int64, _P]),
    ("egonn_voxel_map_merge_scratch_bytes", C.c_int64, [C.c_int64, C.c_int64, C.c_int64]),
    ("egonn_voxel_map_merge", C.c_int, [_P, _P, _P, _P, _P, C.c_int64, _P, _P, _P, _P, _P, C.c_int64, _P, _P, _P, _P, C.c_int64,
                                        _P, _P, _P, C.c_int64, _P]),
    ("egonn_voxel_map_select_scratch_bytes", C.c_int64, [C.c_int64, C.c_int]),
    ("egonn_voxel_map_select", C.c_int, [_P, _P, _P, _P, _P, C.c_int64, C.POINTER(C.c_double), C.c_double, C.c_int, C.c_int, _P,
                                         C.c_int, C.c_int, _P, _P, _P, _P, C.c_int64, _P, _P, C.c_int64, _P]),
    ("egonn_voxel_map_integrate_moments_scratch_bytes", C.c_int64, [C.c_int64, C.c_int]),
    ("egonn_voxel_map_integrate_moments", C.c_int, [_P, C.c_int64, _P, C.c_int64, _P, _P, C.c_int, C.POINTER(C.c_double), C.c_double,
                                                    C.c_int64, _P, _P, _P, _P, _P, _P, C.c_int64, _P, _P, _P, C.c_int64, _P]),
    ("egonn_voxel_map_merge_moments_scratch_bytes", C.c_int64, [C.c_int64, C.c_int64, C.c_int64]),
    ("egonn_voxel_map_merge_moments", C.c_int, [_P] * 7 + [C.c_int64] + [_P] * 7 + [C.c_int64] + [_P] * 6 +
     [C.c_int64, _P, _P, _P, C.c_int64, _P]),
    ("egonn_voxel_map_subtract_scratch_bytes", C.c_int64, [C.c_int64, C.c_int64, C.c_int64]),
    ("egonn_voxel_map_subtract", C.c_int, [_P] * 7 + [C.c_int64] + [_P] * 7 + [C.c_int64] + [_P] * 6 +
     [C.c_int64, _P, _P, _P, C.c_int64, _P]),
    ("egonn_ndt_accumulate_scratch_bytes", C.c_int64, [C.c_int64, C.c_int]),
    ("egonn_ndt_accumulate", C.c_int, [_P, C.c_int64, _P, C.c_int64, _P, _P, C.c_int, C.POINTER(C.c_double), C.c_double, C.c_int64,
                                       _P, _P, C.c_int64, _P, _P, _P, _P, _P, _P, C.c_int64, _P]),
    ("egonn_ndt_finalize", C.c_int, [_P, _P, C.c_int64, _P, _P, _P, C.c_double, C.c_int, C.c_double, _P, _P, _P, _P, _P, _P, _P, _P]),
    ("egonn_ndt_register_scratch_bytes", C.c_int64, [C.c_int64, C.c_int]),
    ("egonn_ndt_register", C.c_int, [_P, C.c_int64, _P, C.c_int, _P, _P, _P, C.c_int64, _P, _P, _P, C.c_double, C.c_int, C.c_int,
                                     C.c_double, C.c_double, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int64, _P]),
    ("egonn_match_candidates_scratch_bytes", C.c_int64, [C.c_int, C.c_int, C.c_int]),
    ("egonn_match_candidates", C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P,
                                         C.c_int64, _P]),
    ("egonn_gather_candidates", C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P]),
    ("egonn_pick_candidates", C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int] + [_P] * 12),
    ("egonn_time_windows", C.c_int, [_P, C.c_int64, _P, C.c_int64, C.c_double, C.c_double, _P, _P, _P, _P]),
    ("egonn_knn_window_scratch_bytes", C.c_int64, [C.c_int64, C.c_int]),
    ("egonn_knn_window", C.c_int, [_P, C.c_int64, _P, C.c_int64, C.c_int, C.c_int, _P, _P, _P, _P, _P, C.c_int64, _P]),
    ("egonn_window_radius", C.c_int, [_P, C.c_int64, _P, C.c_int64, C.c_int, _P, _P, C.c_float, _P, _P, _P, _P]),
    ("egonn_pr_curve_scratch_bytes", C.c_int64, [C.c_int64]),
    ("egonn_pr_curve", C.c_int, [_P, _P, _P, C.c_int64, _P, _P, _P, _P, _P, _P, _P, C.c_int64, _P]),
    ("egonn_pose_graph_scratch_bytes", C.c_int64, [C.c_int64, C.c_int64, C.c_int]),
    ("egonn_pose_graph_odometry", C.c_int, [_P, C.c_int64, _P, _P, _P]),
    ("egonn_pose_graph_plan", C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_int64, _P, _P, _P, C.c_int64, _P]),
    ("egonn_pose_graph_cost", C.c_int, [_P, C.c_int64, C.c_int64, _P, C.c_double, _P, _P, _P, _P, _P, _P, _P, C.c_int64, _P]),
    ("egonn_pose_graph_hessvec", C.c_int, [_P, C.c_int64, C.c_int64, _P, C.c_double, C.c_double, _P, _P, _P, _P, C.c_int64, _P]),
    ("egonn_pose_graph_optimize", C.c_int, [_P, C.c_int64, C.c_int64, _P, C.c_double, C.c_int, C.c_int] + [C.c_double] * 6 +
     [_P] * 8 + [C.c_int64, _P]),
    ("egonn_loop_consistency_scratch_bytes", C.c_int64, [C.c_int64, C.c_int]),
    ("egonn_loop_consistency", C.c_int, [_P, C.c_int64, _P, _P, _P, C.c_int64, C.c_int] + [C.c_double] * 4 + [C.c_int] * 3 +
     [_P] * 8 + [C.c_int64, _P]),
    ("egonn_loop_cycle_errors", C.c_int, [_P, C.c_int64, _P, _P, C.c_int64, _P, C.c_int64, _P, _P]),
    ("egonn_profile_enable", C.c_int, [_P, C.c_int, C.c_char_p]),
    ("egonn_profile_fetch", C.c_int, [_P, C.c_int, C.POINTER(C.c_int), C.c_char_p, C.POINTER(C.c_float),
                                      C.POINTER(C.c_double), C.POINTER(C.c_double), _P]),
]
EXPORTED_SYMBOLS = [s[0] for s in _SIGS]

_lib = None


def load() -> C.CDLL:
    """Load libegonn_hip.so; loud failure if it has not been built (python __graft_entry__.py / make)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"egonn_amd: HIP library not found at {LIB_PATH}. Build it with "
            f"`python -c 'import __graft_entry__ as g; g.build()'` (hipcc --offload-arch=gfx950). "
            f"There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, res, args in _SIGS:
        fn = getattr(lib, name)          # AttributeError if the .so does not export it
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def _err(lib) -> str:
    msg = lib.egonn_last_error()
    return msg.decode() if msg else "unknown error"


class EgonnError(RuntimeError):
    """non-zero status of a libegonn_hip entry point; `.code` is the C status (include/egonn_hip.h EGONN_STATUS_*)"""

    def __init__(self, msg: str, code: int):
        super().__init__(msg)
        self.code = int(code)


class CapacityError(EgonnError):
    """status 5: the batch did not fit the capacities of egonn_ctx_reserve (the exact-size eager path still works)"""


class Fp16RangeError(EgonnError):
    """status 6: a kernel on the fp16-split pipe (fp32 sparse convolution or local heads) met an operand fp16 cannot hold
    (|x| >= 65520) or a non-finite input: the batch's outputs are invalid; Context.set_exact_fp32(True) and run it again
    (on the same plan: every forward clears this flag)"""


def check(rc: int):
    if rc != 0:
        cls = CapacityError if rc == 5 else (Fp16RangeError if rc == 6 else EgonnError)
        raise cls(f"libegonn_hip: {_err(load())} (code {rc})", rc)


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def call(device: torch.device, fn, *args):
    """The one way into the library for every entry point that ends in a stream: `fn(*args, stream)` on `device`'s current
    stream, raising on a non-zero status.  The device is switched only when it is not the current one already."""
    idx = device.index
    if idx is None or torch.cuda.current_device() == idx:       # common case: no device switch needed
        rc = fn(*args, _stream())
    else:
        with torch.cuda.device(device):
            rc = fn(*args, _stream())
    if rc != 0:
        check(rc)


def _dev_f32(t: torch.Tensor, device) -> torch.Tensor:
    return t.to(device=device, dtype=torch.float32).contiguous()


def as_dev(x, dev, dtype) -> torch.Tensor:
    """anything array-like as a contiguous tensor of `dtype` on `dev` (no copy when it is one already)"""
    return torch.as_tensor(x).to(device=dev, dtype=dtype).contiguous()


def scratch(nbytes: int, dev) -> torch.Tensor:
    """caller-owned scratch of at least `nbytes` (8 at the least: a *_scratch_bytes of -1 still yields a pointer, and the call
    it is handed to raises), 8-byte aligned: int64 elements, so `numel() * 8` is its size"""
    return torch.empty((max(int(nbytes), 8) + 7) // 8, dtype=torch.int64, device=dev)


# concatenated clouds: points (n, 3), cloud c = rows [offsets[c], offsets[c + 1])
def check_cloud(name, x):
    shape = tuple(getattr(x, "shape", ()))
    if len(shape) != 2 or shape[1] != 3:
        raise ValueError(f"{name}: expected (n, 3) points, got shape {shape}")


def check_offsets(name, off) -> int:
    """-> the number of clouds"""
    shape = tuple(getattr(off, "shape", (len(off),) if hasattr(off, "__len__") else ()))
    if len(shape) != 1 or shape[0] < 2:
        raise ValueError(f"{name}: offsets must be a 1-D sequence of n_clouds + 1 entries, got shape {shape}")
    return shape[0] - 1


def concat_clouds(clouds, dev):
    """per-scan (n,3) arrays -> (points (sum n, 3) f32 on the device, (len+1,) int64 offsets)"""
    ts = [torch.as_tensor(c) for c in clouds]
    for c in ts:
        check_cloud("cloud", c)
    off = [0]
    for c in ts:
        off.append(off[-1] + c.shape[0])
    pts = torch.cat([c.to(device=dev, dtype=torch.float32) for c in ts]) if ts else torch.zeros((0, 3), device=dev)
    return pts, torch.tensor(off, dtype=torch.int64, device=dev)


def dense_pack_fragments(weight, out_in: bool):
    """egonn_dense_pack_fragments(_host): a 1x1 kernel ((cin, cout), or (cout, cin) with out_in) in the dense kernels' LDS fragment
    order, cin * cout floats.  A numpy array is packed on the host (no device needed), a device tensor on the device."""
    lib = load()
    co, ci = (weight.shape if out_in else weight.shape[::-1])
    if isinstance(weight, np.ndarray):
        w = np.ascontiguousarray(weight, dtype=np.float32)
        out = np.empty(ci * co, dtype=np.float32)
        check(lib.egonn_dense_pack_fragments_host(w.ctypes.data, int(bool(out_in)), int(ci), int(co), out.ctypes.data))
        return out
    w = weight.contiguous()
    out = torch.empty(ci * co, dtype=torch.float32, device=w.device)
    call(w.device, lib.egonn_dense_pack_fragments, w.data_ptr(), int(bool(out_in)), int(ci), int(co), out.data_ptr())
    return out


def debug_dense(x, weight, out_in: bool, out, form: int, n_dev=None, packed=None, bias=None, scale=None, shift=None, act: int = 0,
                residual=None, gate=None, boff=None):
    """test hook (egonn_debug_dense): the forward's dense launcher on device tensors.  x (capacity, cin) and residual / out
    (capacity, cout) are fp32 or bf16 maps (by dtype); rows from n_dev[0] on are left as they are in `out`.  form 0 = the
    persistent LDS kernel, 1 = the streaming form (with `packed` from dense_pack_fragments, or gathering the weights)."""
    lib = load()
    cap, cin = x.shape
    cout = out.shape[1]
    B = 0 if boff is None else boff.numel() - 1
    bf = lambda t: int(t is not None and t.dtype == torch.bfloat16)
    call(x.device, lib.egonn_debug_dense, x.data_ptr(), bf(x), int(cap), _ptr(n_dev), int(cin), int(cout), weight.data_ptr(),
         int(bool(out_in)), _ptr(packed), _ptr(bias), _ptr(scale), _ptr(shift), int(act), _ptr(residual), bf(residual), _ptr(gate),
         _ptr(boff), B, out.data_ptr(), bf(out), int(form))
    return out


# codes of Context.set_naive_conv / egonn_debug_set_naive_conv (the table: include/egonn_hip.h)
CONV_PRODUCT, CONV_PLAIN, CONV_RING, CONV_COOP, CONV_RING2, CONV_DMA, CONV_DMA3, CONV_TRACED = 0, 1, 2, 4, 8, 16, 32, 128
CONV_SPLIT = 1000                      # + cfg: the split kernel in an explicit configuration
CFG_NW4, CFG_NW8, CFG_RESIDENT = 142, 182, 183
CFG_PARTS, CFG_TRACED = 400, 9000      # + CFG_PARTS * (1 + log2(column parts)), + CFG_TRACED
SCONV_ROUTES = ("plain", "split", "tail_split", "wg", "dma", "rg")     # SconvRoute of egonn_amd/csrc/kernels.h, from 0
SCONV_CHOICE_FIELDS = ("route", "kernel", "NW", "NSW", "KW", "KS", "GATED", "TRACE", "resident", "KSP", "D", "G", "SPLIT", "PIPE",
                       "gx", "gy", "gz", "block", "lds", "kparts")


def debug_sconv_choice(kind: int, level: int, cin: int, cout: int, cap_groups: int, *, code: int = 0, bf16: int = 0, gated: int = 0,
                       split_io: int = 0, residual: int = 0, split_max_level: int = 5, autoscale: int = 0, resident_mask: int = -1,
                       max_workgroups: int = 0, kparts: int = -1, kw: int = -1, col_parts: int = -1) -> dict:
    """test hook (egonn_debug_sconv_choice, no device needed): the launch a sparse-convolution layer gets under a setting, as a dict
    of SCONV_CHOICE_FIELDS (route and kernel by name)"""
    arg = (C.c_int32 * 16)(int(code), kind, level, cin, cout, int(bf16), int(gated), split_io, int(residual), split_max_level,
                           int(autoscale), resident_mask, max_workgroups, kparts, kw, col_parts)
    out = (C.c_int32 * 20)()
    check(load().egonn_debug_sconv_choice(arg, int(cap_groups), out))
    d = dict(zip(SCONV_CHOICE_FIELDS, out))
    d["route"], d["kernel"] = SCONV_ROUTES[d["route"]], SCONV_ROUTES[d["kernel"]]
    return d


DENSE_ROUTES = ("none", "stream", "lds", "small", "tile", "plain")      # DenseRoute of egonn_amd/csrc/kernels.h, from 0


def debug_dense_route(rows: int, cin: int, cout: int, form: int = -1, gate_scans: int = 0):
    """test hook (egonn_debug_dense_route, no device needed): -> (route name, grid x, grid y, dynamic LDS bytes, colblk) of the
    launch the dense launcher picks; raises its error for a form or a gate the shape does not have"""
    out = (C.c_int32 * 5)()
    check(load().egonn_debug_dense_route(int(rows), int(cin), int(cout), int(form), int(gate_scans), out))
    return (DENSE_ROUTES[out[0]],) + tuple(out[1:])


def debug_radix_sort(keys_in, vals_in, keys_out, vals_out, n: int, nbits: int, n_dev=None, seg_offsets=None, idx_bits: int = 0,
                     either_pair: bool = False, scratch_buf=None, scratch_bytes: Optional[int] = None) -> int:
    """test hook (egonn_debug_radix_sort): the flat radix sort of the first n (u64 key as int64, u32 value as int32) pairs,
    or with seg_offsets (device int64, segments + 1) the segmented one.  -> 0: the result is in (keys_in, vals_in), 1: in
    (keys_out, vals_out).  scratch_buf / scratch_bytes: a scratch of the caller's (default: one of the reported size)."""
    lib = load()
    B = 0 if seg_offsets is None else seg_offsets.numel() - 1
    need = lib.egonn_debug_radix_sort_scratch_bytes(int(n), B)
    if scratch_buf is None:
        scratch_buf = scratch(need, keys_in.device)
    pair = C.c_int32(-1)
    call(keys_in.device, lib.egonn_debug_radix_sort, keys_in.data_ptr(), vals_in.data_ptr(), keys_out.data_ptr(),
         vals_out.data_ptr(), int(n), int(nbits), _ptr(n_dev), _ptr(seg_offsets), B, int(idx_bits), int(bool(either_pair)),
         C.byref(pair), scratch_buf.data_ptr(), need if scratch_bytes is None else int(scratch_bytes))
    return pair.value


def debug_dense_group3(xs, capacities, counts, ws, packed: bool):
    """test hook (egonn_debug_dense_group3): three (capacity_q, 128) @ (128, 128) products in the grouped lateral launch, reading
    packed fragments or the raw (cin, cout) kernels.  xs[q] holds at least max(capacity_q, 1) rows; counts[q] is the live count.
    -> three (capacity_q, 128) outputs, -12345 in every row the launch did not write"""
    lib = load()
    dev = xs[0].device
    arr = lambda ptrs: (C.c_void_p * 3)(*ptrs)  # noqa: E731
    nds = [torch.tensor([int(c)], dtype=torch.int32, device=dev) for c in counts]
    pks = [dense_pack_fragments(w, False) for w in ws] if packed else [None] * 3
    bufs = [torch.full((max(int(c), 1), 128), -12345.0, dtype=torch.float32, device=dev) for c in capacities]
    call(dev, lib.egonn_debug_dense_group3, arr([x.data_ptr() for x in xs]), (C.c_int64 * 3)(*[int(c) for c in capacities]),
         arr([n.data_ptr() for n in nds]), arr([w.data_ptr() for w in ws]), arr([_ptr(p) for p in pks]),
         arr([b.data_ptr() for b in bufs]))
    return [b[:int(c)] for b, c in zip(bufs, capacities)]


GLOBAL_TAIL_POOLING = {"GeM": 1, "MAC": 2, "SPoC": 3}


def debug_global_tail(g5, row_offsets, n_dev, w0, b0, w1, b1, p, pooling: str, form: int):
    """test hook (egonn_debug_global_tail): descriptor decoder + global pooling on the fp32 rows g5 (capacity, 128) of the scans
    row_offsets (device int32, B + 1) below the live count n_dev (device int32).  form 0 = two dense launches + partial sums,
    1 = the fused launch.  -> (partial (B, 32, 256), pooled (B, 256))"""
    lib = load()
    B = row_offsets.numel() - 1
    cap = g5.shape[0]
    need = lib.egonn_debug_global_tail_scratch_bytes(int(cap))
    buf = scratch(need, g5.device)
    partial = torch.empty((B, 32, 256), dtype=torch.float32, device=g5.device)
    out = torch.empty((B, 256), dtype=torch.float32, device=g5.device)
    call(g5.device, lib.egonn_debug_global_tail, g5.data_ptr(), row_offsets.data_ptr(), B, int(cap), n_dev.data_ptr(), w0.data_ptr(),
         b0.data_ptr(), w1.data_ptr(), b1.data_ptr(), _ptr(p), GLOBAL_TAIL_POOLING[pooling], int(form), partial.data_ptr(),
         out.data_ptr(), buf.data_ptr(), need)
    return partial, out


def require_gpu() -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError("egonn_amd: no HIP device visible (torch.cuda.is_available() is False); "
                           "the descriptor-extraction path runs on MI355X only — there is no CPU fallback.")
    return torch.device("cuda", torch.cuda.current_device())


class Context:
    """egonn_ctx: coordinate plan + workspace of one device."""

    def __init__(self, device: Optional[torch.device] = None, coord_bits: int = 16):
        self.lib = load()
        self.device = torch.device(device) if device is not None else require_gpu()
        if self.device.type != "cuda":
            raise RuntimeError(f"egonn_amd: device {self.device} is not a HIP device; there is no CPU fallback.")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        h = _P()
        check(self.lib.egonn_ctx_create(C.byref(h), self.device.index, coord_bits))
        self.h = h
        self.batch_size = 0
        self._keep = []

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.lib.egonn_ctx_destroy(self.h)
                self.h = None
        except Exception:
            pass

    # ------------------------------------------------------------------ plan
    def voxelize(self, points: torch.Tensor, scan_offsets: Sequence[int], mode: int, step: Sequence[float]):
        assert points.is_cuda and points.dtype == torch.float32 and points.is_contiguous()
        assert points.dim() == 2 and points.shape[1] == 3
        B = len(scan_offsets) - 1
        off = (C.c_int64 * (B + 1))(*[int(o) for o in scan_offsets])
        st = (C.c_float * 3)(*([float(s) for s in step] + [0.0, 0.0])[:3])
        self._call(self.lib.egonn_voxelize, self.h, points.data_ptr(), off, B, mode, st)
        self.batch_size = B

    def reserve(self, max_points: int, batch_size: int, level_capacity: Optional[Sequence[int]] = None):
        """egonn_ctx_reserve: fixed capacities => later voxelize_device plans neither allocate nor synchronise."""
        caps = None
        if level_capacity is not None:
            assert len(level_capacity) == 8
            caps = (C.c_int64 * 8)(*[int(v) for v in level_capacity])
        with torch.cuda.device(self.device):
            check(self.lib.egonn_ctx_reserve(self.h, int(max_points), int(batch_size), caps))
        self.batch_size = int(batch_size)

    def voxelize_device(self, points: torch.Tensor, scan_offsets: torch.Tensor, batch_size: int, mode: int,
                        step: Sequence[float]):
        """points (n_rows,3) f32 and scan_offsets (B+1,) int64 both on the device; no host synchronisation."""
        assert points.is_cuda and points.dtype == torch.float32 and points.is_contiguous() and points.shape[1] == 3
        assert scan_offsets.is_cuda and scan_offsets.dtype == torch.int64 and scan_offsets.numel() == batch_size + 1
        st = (C.c_float * 3)(*([float(s) for s in step] + [0.0, 0.0])[:3])
        self._call(self.lib.egonn_voxelize_device, self.h, points.data_ptr(), points.shape[0], scan_offsets.data_ptr(),
                   int(batch_size), mode, st)
        self.batch_size = int(batch_size)

    def plan_status(self):
        """[SYNC] raises if the latest (replayed) plan left the coordinate range or the reserved capacities."""
        self._call(self.lib.egonn_plan_status, self.h)

    def level_capacity(self, level: int) -> int:
        n = C.c_int64()
        check(self.lib.egonn_level_capacity(self.h, level, C.byref(n)))
        return n.value

    def coords_set(self, coords: torch.Tensor, batch_size: int):
        assert coords.is_cuda and coords.dtype == torch.int32 and coords.is_contiguous()
        assert coords.dim() == 2 and coords.shape[1] == 4
        self._call(self.lib.egonn_coords_set, self.h, coords.data_ptr(), coords.shape[0], int(batch_size))
        self.batch_size = int(batch_size)

    def level_count(self, level: int) -> int:
        n = C.c_int64()
        check(self.lib.egonn_level_count(self.h, level, C.byref(n)))
        return n.value

    def level_batch_offsets(self, level: int) -> List[int]:
        off = (C.c_int64 * (self.batch_size + 1))()
        check(self.lib.egonn_level_batch_offsets(self.h, level, off))
        return list(off)

    def level_coords(self, level: int) -> torch.Tensor:
        out = torch.empty((self.level_count(level), 4), dtype=torch.int32, device=self.device)
        self._call(self.lib.egonn_level_coords, self.h, level, out.data_ptr())
        return out

    def input_index(self) -> torch.Tensor:
        out = torch.empty((self.level_count(0),), dtype=torch.int64, device=self.device)
        self._call(self.lib.egonn_input_index, self.h, out.data_ptr())
        return out

    # ------------------------------------------------------------------ operators
    def conv(self, level_in: int, level_out: int, kernel_size: int, x: torch.Tensor, kernel: torch.Tensor,
             scale: Optional[torch.Tensor] = None, shift: Optional[torch.Tensor] = None, relu: bool = False):
        kernel = _dev_f32(kernel, self.device)
        cin, cout = kernel.shape[-2], kernel.shape[-1]
        if x is None:
            assert kernel_size == 5 and cin == 1, "x=None (all-ones features) is the k=5 input layer only"
        else:
            x = _dev_f32(x, self.device)
            assert x.shape == (self.level_count(level_in), cin), (x.shape, self.level_count(level_in), cin)
        out = torch.empty((self.level_count(level_out), cout), dtype=torch.float32, device=self.device)
        sc = None if scale is None else _dev_f32(scale, self.device)
        sh = None if shift is None else _dev_f32(shift, self.device)
        self._call(self.lib.egonn_conv, self.h, level_in, level_out, kernel_size, _ptr(x), cin, kernel.data_ptr(), cout,
                   _ptr(sc), _ptr(sh), int(relu), out.data_ptr())
        return out

    def conv_transpose(self, level_in: int, x: torch.Tensor, kernel: torch.Tensor):
        x = _dev_f32(x, self.device)
        kernel = _dev_f32(kernel, self.device)
        cin, cout = kernel.shape[-2], kernel.shape[-1]
        assert x.shape == (self.level_count(level_in), cin)
        out = torch.empty((self.level_count(level_in - 1), cout), dtype=torch.float32, device=self.device)
        self._call(self.lib.egonn_conv_transpose, self.h, level_in, x.data_ptr(), cin, kernel.data_ptr(), cout, out.data_ptr())
        return out

    def sparse_conv(self, map_kind: int, level_out: int, x: torch.Tensor, kernel: torch.Tensor, scale=None, shift=None,
                    relu: bool = False, group_sums: bool = False):
        """egonn_sparse_conv: x fp32 or bf16 (the output has x's dtype).  map_kind 0: k=3, 1: k=2/s=2 into level_out,
        2: transposed onto level_out.  Returns out, or (out, sums) with the per-group column sums."""
        assert x.is_cuda and x.dtype in (torch.float32, torch.bfloat16) and x.is_contiguous()
        kernel = _dev_f32(kernel, self.device)
        cin, cout = kernel.shape[-2], kernel.shape[-1]
        assert x.shape[1] == cin
        out = torch.empty((self.level_count(level_out), cout), dtype=x.dtype, device=self.device)
        sc = None if scale is None else _dev_f32(scale, self.device)
        sh = None if shift is None else _dev_f32(shift, self.device)
        sums = None
        if group_sums:
            sums = torch.zeros((self.map_groups(map_kind, level_out)[0], cout), dtype=torch.float32, device=self.device)
        self._call(self.lib.egonn_sparse_conv, self.h, map_kind, level_out, x.data_ptr(), cin, kernel.data_ptr(), cout,
                   int(x.dtype == torch.bfloat16), _ptr(sc), _ptr(sh), int(relu), out.data_ptr(), _ptr(sums))
        return (out, sums) if group_sums else out

    def prepare_maps(self, with_level0_transpose: bool = False):
        """row-group tables of every kernel map of the plan in ONE launch (training steps, operator sequences)"""
        self._call(self.lib.egonn_prepare_maps, self.h, int(with_level0_transpose))

    def map_groups(self, map_kind: int, level_out: int):
        n = C.c_int64()
        first = (C.c_int64 * (self.batch_size + 1))()
        self._call(self.lib.egonn_map_groups, self.h, map_kind, level_out, C.byref(n), first)
        return n.value, list(first)

    def rowgroup_tables(self, map_kind: int, level_out: int, with_rows: bool = True):
        """measurement hook: (gmask [groups] int32 view of u32, snbr [groups, K, 16] int32) of a map's row-group tables."""
        ng, _ = self.map_groups(map_kind, level_out)
        K = 27 if map_kind == 0 else 8
        gm = torch.empty(ng, dtype=torch.int32, device=self.device)
        sn = torch.empty((ng, K, 16), dtype=torch.int32, device=self.device) if with_rows else None
        n = C.c_int64()
        self._call(self.lib.egonn_debug_rowgroup_tables, self.h, map_kind, level_out, gm.data_ptr(),
                   sn.data_ptr() if with_rows else None, ng, C.byref(n))
        return gm, sn

    def rowgroup_perm(self, map_kind: int, level_out: int):
        """test hook: perm [groups, 16] int32 of a map's row-group tables, the output row of every slot (-1 = padding)."""
        ng, _ = self.map_groups(map_kind, level_out)
        pm = torch.empty((ng, 16), dtype=torch.int32, device=self.device)
        n = C.c_int64()
        self._call(self.lib.egonn_debug_rowgroup_perm, self.h, map_kind, level_out, pm.data_ptr(), ng, C.byref(n))
        return pm

    def set_naive_conv(self, on):
        """tests / measurements only: True or CONV_PLAIN routes this context's sparse convolutions through the plain (non-MFMA)
        kernel; any other CONV_* code (or CONV_SPLIT + cfg) forces that kernel; False / CONV_PRODUCT = the product choice."""
        check(self.lib.egonn_debug_set_naive_conv(self.h, int(on)))

    def keep_level_features(self, on: bool):
        """tests only: materialise every level's block output (forward_level_features(1) then works)."""
        check(self.lib.egonn_debug_keep_level_features(self.h, int(bool(on))))

    def set_exact_fp32(self, on: bool):
        """fp32 maps: True = every sparse convolution on the exact fp32 kernels (full fp32 range); False (default) = levels <= 5 on
        the fp16-split matrix pipe (|activation| < 65504, guarded: plan_status raises with code 6)."""
        check(self.lib.egonn_ctx_set_exact_fp32(self.h, int(bool(on))))

    def set_operand_autoscale(self, on: bool):
        """fp16-split convolutions scale their input by a power of two per launch (max |in| -> [2^13, 2^14)): small operands
        (input gradients) keep their low parts.  Eager plans only: on a reserved context it raises (code 4)."""
        check(self.lib.egonn_ctx_set_operand_autoscale(self.h, int(bool(on))))

    def set_ksplit(self, map_class: int, level: int, kparts: int = -1, kw: int = -1, col_parts: int = -1):
        """tests / A-B only: offset-split rule of the fp32 sparse convolutions (map_class 0: k=3 maps, 1: 8-slot maps); -1 keeps a field."""
        check(self.lib.egonn_debug_set_ksplit(self.h, int(map_class), int(level), int(kparts), int(kw), int(col_parts)))

    def set_resident(self, mask: int = -1, max_workgroups: int = 0):
        """tests / A-B only: 32->32 split convolutions on the weight-resident form (bit 0: k=3 of level 1, bit 1: k=2,s=2 into
        level 1, bit 2: gated k=2,s=2 into level 2; -1: the product rule); workgroups per resident launch, 0 = default."""
        check(self.lib.egonn_debug_set_resident(self.h, int(mask), int(max_workgroups)))

    def global_avg_pool(self, level: int, x: torch.Tensor):
        x = _dev_f32(x, self.device)
        out = torch.empty((self.batch_size, x.shape[1]), dtype=torch.float32, device=self.device)
        self._call(self.lib.egonn_global_avg_pool, self.h, level, x.data_ptr(), x.shape[1], out.data_ptr())
        return out

    def bn_fold(self, bn: torch.nn.BatchNorm1d):
        """(scale, shift) of an eval-mode BatchNorm1d, computed on the device by the library."""
        c = bn.num_features
        w, b, rm, rv = (_dev_f32(t.detach(), self.device) for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var))
        scale = torch.empty(c, dtype=torch.float32, device=self.device)
        shift = torch.empty(c, dtype=torch.float32, device=self.device)
        self._call(self.lib.egonn_bn_fold, w.data_ptr(), b.data_ptr(), rm.data_ptr(), rv.data_ptr(), float(bn.eps), c,
                   scale.data_ptr(), shift.data_ptr())
        return scale, shift

    def block_tail(self, level: int, x: torch.Tensor, residual: torch.Tensor, eca_weight: Optional[torch.Tensor] = None):
        x, residual = _dev_f32(x, self.device), _dev_f32(residual, self.device)
        assert x.shape == residual.shape == (self.level_count(level), x.shape[1])
        out = torch.empty_like(x)
        ew = None if eca_weight is None else _dev_f32(eca_weight.detach().reshape(-1), self.device)
        self._call(self.lib.egonn_block_tail, self.h, level, x.data_ptr(), residual.data_ptr(), x.shape[1], _ptr(ew),
                   0 if ew is None else ew.numel(), out.data_ptr())
        return out

    def se_gate(self, mean: torch.Tensor, w1, b1, w2, b2, want_hidden: bool = False):
        """SELayer.fc on the (B, C) per-sample means: sigmoid(W2 relu(W1 mean + b1) + b2) -> gate (B, C) [, hidden (B, C/16)].
        w1 (C/16, C), b1, w2 (C, C/16), b2: the weights and biases of fc[0].linear and fc[2].linear."""
        mean = _dev_f32(mean, self.device)
        w1, b1, w2, b2 = (_dev_f32(t.detach(), self.device) for t in (w1, b1, w2, b2))
        B, c = mean.shape
        h = w1.shape[0]
        assert w1.shape == (h, c) and w2.shape == (c, h) and b1.shape == (h,) and b2.shape == (c,)
        gate = torch.empty_like(mean)
        hid = torch.empty((B, h), dtype=torch.float32, device=self.device) if want_hidden else None
        self._call(self.lib.egonn_se_gate, mean.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), B, c, h,
                   gate.data_ptr(), _ptr(hid))
        return (gate, hid) if want_hidden else gate

    def add(self, a: torch.Tensor, b: torch.Tensor):
        a, b = _dev_f32(a, self.device), _dev_f32(b, self.device)
        assert a.shape == b.shape
        out = torch.empty_like(a)
        self._call(self.lib.egonn_add, a.data_ptr(), b.data_ptr(), a.numel(), out.data_ptr())
        return out

    def topdown_step(self, level_out: int, x_coarse: torch.Tensor, w_tconv: torch.Tensor, x_lateral: Optional[torch.Tensor] = None,
                     w_lateral: Optional[torch.Tensor] = None, rows: Optional[int] = None):
        """egonn_topdown_step: x_coarse[parent] @ w_tconv[slot] (+ x_lateral @ w_lateral) onto `level_out`; `rows`: rows of the
        output (default: the level's count — a host synchronisation on a reserved plan; pass the capacity there)."""
        x_coarse, w_tconv = _dev_f32(x_coarse, self.device), _dev_f32(w_tconv, self.device)
        c = w_tconv.shape[-1]
        cl = 0
        if x_lateral is not None:
            x_lateral, w_lateral = _dev_f32(x_lateral, self.device), _dev_f32(w_lateral, self.device)
            cl = w_lateral.shape[0]
        n = self.level_count(level_out) if rows is None else int(rows)
        out = torch.empty((n, c), dtype=torch.float32, device=self.device)
        self._call(self.lib.egonn_topdown_step, self.h, level_out, x_coarse.data_ptr(), w_tconv.data_ptr(), _ptr(x_lateral),
                   _ptr(w_lateral), c, cl, out.data_ptr())
        return out

    def gather_input(self, feats: torch.Tensor):
        feats = _dev_f32(feats, self.device)
        out = torch.empty((self.level_count(0), feats.shape[1]), dtype=torch.float32, device=self.device)
        self._call(self.lib.egonn_gather_input, self.h, feats.data_ptr(), feats.shape[1], out.data_ptr())
        return out

    def gem(self, level: int, x: torch.Tensor, p: torch.Tensor):
        x = _dev_f32(x, self.device)
        pp = _dev_f32(p.detach().reshape(-1), self.device)
        out = torch.empty((self.batch_size, x.shape[1]), dtype=torch.float32, device=self.device)
        self._call(self.lib.egonn_gem, self.h, level, x.data_ptr(), x.shape[1], pp.data_ptr(), out.data_ptr())
        return out

    def global_max_pool(self, level: int, x: torch.Tensor):
        x = _dev_f32(x, self.device)
        out = torch.empty((self.batch_size, x.shape[1]), dtype=torch.float32, device=self.device)
        self._call(self.lib.egonn_global_max_pool, self.h, level, x.data_ptr(), x.shape[1], out.data_ptr())
        return out

    def netvlad(self, level: int, x: torch.Tensor, cluster_weights: torch.Tensor, cluster_weights2: torch.Tensor,
                bn1: torch.nn.BatchNorm1d, hidden1_weights: torch.Tensor, bn2: torch.nn.BatchNorm1d,
                gating_weights: Optional[torch.Tensor] = None, gate_bn: Optional[torch.nn.BatchNorm1d] = None):
        """NetVLADLoupe (layers/netvlad.py:18-112) in eval mode over the rows of `level`: (B, output_dim).  gating_weights /
        gate_bn given = 'netvladgc'.  The BatchNorms are folded on the device; no host synchronisation."""
        x = _dev_f32(x, self.device)
        assert x.dim() == 2 and x.shape[0] >= self.level_count(level), "netvlad: x must hold every row of the level"
        w = [_dev_f32(t.detach(), self.device) for t in (cluster_weights, cluster_weights2, hidden1_weights)]
        d = w[2].shape[-1]
        sc1, sh1 = self.bn_fold(bn1)
        sc2, sh2 = self.bn_fold(bn2)
        gating = gating_weights is not None
        gw = scg = shg = None
        if gating:
            gw = _dev_f32(gating_weights.detach(), self.device)
            scg, shg = self.bn_fold(gate_bn)
        out = torch.empty((self.batch_size, d), dtype=torch.float32, device=self.device)
        self._call(self.lib.egonn_netvlad, self.h, level, x.data_ptr(), x.shape[1], w[0].data_ptr(), w[1].data_ptr(),
                   sc1.data_ptr(), sh1.data_ptr(), w[2].data_ptr(), sc2.data_ptr(), sh2.data_ptr(), _ptr(gw), _ptr(scg),
                   _ptr(shg), d, int(gating), out.data_ptr())
        return out

    # ------------------------------------------------------------------ training-mode operators (egonn_amd/train.py)
    def scratch(self, nfloats: int) -> torch.Tensor:
        """caller-owned scratch for the two-stage reductions (grown on demand, reused)."""
        buf = getattr(self, "_scratch", None)
        if buf is None or buf.numel() < nfloats:
            buf = torch.empty(max(int(nfloats), 1 << 24), dtype=torch.float32, device=self.device)
            self._scratch = buf
        return buf

    def _call(self, fn, *args):
        call(self.device, fn, *args)

    def dense(self, x, weight, out_in: bool, bias=None, act: int = 0):
        x, weight = _dev_f32(x, self.device), _dev_f32(weight, self.device)
        cin, cout = (weight.shape[1], weight.shape[0]) if out_in else (weight.shape[0], weight.shape[1])
        assert x.dim() == 2 and x.shape[1] == cin, (x.shape, weight.shape, out_in)
        b = None if bias is None else _dev_f32(bias, self.device)
        out = torch.empty((x.shape[0], cout), dtype=torch.float32, device=self.device)
        self._call(self.lib.egonn_dense, x.data_ptr(), x.shape[0], cin, weight.data_ptr(), int(out_in), _ptr(b), cout,
                   act, out.data_ptr())
        return out

    def netvlad_train_forward(self, level: int, x: torch.Tensor, nmax: int, cluster_weights, cluster_weights2,
                              bn1: torch.nn.BatchNorm1d, hidden1_weights):
        """egonn_netvlad_train_forward: (y (B, D) before bn2, saved tensors for netvlad_train_backward); updates bn1's running
        statistics in place (num_batches_tracked is the caller's)."""
        x = _dev_f32(x, self.device)
        n, c = x.shape
        assert n == self.level_count(level), "netvlad: x must hold exactly the rows of the level"
        B, d = self.batch_size, hidden1_weights.shape[-1]
        f = dict(dtype=torch.float32, device=self.device)
        out = torch.empty((B, d), **f)
        saved = (torch.empty((n, 64), **f), torch.empty((4, 64), **f), torch.empty((B, c, 64), **f),
                 torch.empty((B, c // 16, 64), **f), torch.empty((B, 64), **f))
        mom = bn1.momentum if bn1.momentum is not None else 1.0 / float(int(bn1.num_batches_tracked) + 1)
        self._call(self.lib.egonn_netvlad_train_forward, self.h, level, x.data_ptr(), c, int(nmax), cluster_weights.data_ptr(),
                   cluster_weights2.data_ptr(), bn1.weight.data_ptr(), bn1.bias.data_ptr(), float(bn1.eps), float(mom),
                   bn1.running_mean.data_ptr(), bn1.running_var.data_ptr(), hidden1_weights.data_ptr(), d, out.data_ptr(),
                   *[t.data_ptr() for t in saved])
        return out, saved

    def netvlad_train_backward(self, level: int, x, nmax: int, cluster_weights, cluster_weights2, bn1_weight, hidden1_weights,
                               grad_out, saved):
        """egonn_netvlad_train_backward: (grad x, grad cluster_weights, grad cluster_weights2, grad bn1 weight, grad bn1 bias,
        grad hidden1_weights)"""
        x, g = _dev_f32(x, self.device), _dev_f32(grad_out, self.device)
        n, c = x.shape
        d = hidden1_weights.shape[-1]
        f = dict(dtype=torch.float32, device=self.device)
        dx, dwc, dw2 = torch.empty((n, c), **f), torch.empty((c, 64), **f), torch.empty((c, 64), **f)
        bn5, dh = torch.empty((5, 64), **f), torch.empty((c * 64, d), **f)
        self._call(self.lib.egonn_netvlad_train_backward, self.h, level, x.data_ptr(), c, int(nmax), cluster_weights.data_ptr(),
                   cluster_weights2.data_ptr(), bn1_weight.data_ptr(), hidden1_weights.data_ptr(), d, g.data_ptr(),
                   *[t.data_ptr() for t in saved], dx.data_ptr(), dwc.data_ptr(), dw2.data_ptr(), bn5.data_ptr(), dh.data_ptr())
        return dx, dwc, dw2, bn5[3], bn5[4], dh

    def global_max_pool_argmax(self, level: int, x: torch.Tensor):
        """MAC and the plan row of every maximum (ties: lowest row; -1 for an empty scan): ((B, C) f32, (B, C) int32)"""
        x = _dev_f32(x, self.device)
        assert x.shape[0] == self.level_count(level)
        out = torch.empty((self.batch_size, x.shape[1]), dtype=torch.float32, device=self.device)
        rows = torch.empty((self.batch_size, x.shape[1]), dtype=torch.int32, device=self.device)
        self._call(self.lib.egonn_global_max_pool_argmax, self.h, level, x.data_ptr(), x.shape[1], out.data_ptr(),
                   rows.data_ptr())
        return out, rows

    def global_max_pool_backward(self, level: int, grad_out, rows):
        g = _dev_f32(grad_out, self.device)
        dx = torch.empty((self.level_count(level), g.shape[1]), dtype=torch.float32, device=self.device)
        self._call(self.lib.egonn_global_max_pool_backward, self.h, level, g.data_ptr(), rows.data_ptr(), g.shape[1],
                   dx.data_ptr())
        return dx

    def sigmoid_gate(self, y, t, grad_out=None):
        """y * sigmoid(t), or with grad_out its backward (grad y, grad t)"""
        y, t = _dev_f32(y, self.device), _dev_f32(t, self.device)
        if grad_out is None:
            out = torch.empty_like(y)
            self._call(self.lib.egonn_sigmoid_gate, y.data_ptr(), t.data_ptr(), None, y.numel(), out.data_ptr(), None, None)
            return out
        g = _dev_f32(grad_out, self.device)
        dy, dt = torch.empty_like(y), torch.empty_like(y)
        self._call(self.lib.egonn_sigmoid_gate, y.data_ptr(), t.data_ptr(), g.data_ptr(), y.numel(), None, dy.data_ptr(),
                   dt.data_ptr())
        return dy, dt

    def dense_backward_weight(self, a, b):
        """a^T b over the rows: (ca, cb)."""
        a, b = _dev_f32(a, self.device), _dev_f32(b, self.device)
        assert a.shape[0] == b.shape[0]
        ca, cb = a.shape[1], b.shape[1]
        out = torch.empty((ca, cb), dtype=torch.float32, device=self.device)
        sc = self.scratch(64 * ca * cb)
        self._call(self.lib.egonn_dense_backward_weight, a.data_ptr(), ca, b.data_ptr(), cb, a.shape[0], out.data_ptr(),
                   sc.data_ptr(), sc.numel())
        return out

    def conv_backward_weight(self, level_in, level_out, kernel_size, transposed, x, grad_out, kernel_shape):
        g = _dev_f32(grad_out, self.device)
        xx = None if x is None else _dev_f32(x, self.device)
        cin, cout = kernel_shape[-2], kernel_shape[-1]
        out = torch.empty(tuple(kernel_shape), dtype=torch.float32, device=self.device)
        sc = self.scratch(16 * out.numel())
        self._call(self.lib.egonn_conv_backward_weight, self.h, level_in, level_out, kernel_size, int(transposed), _ptr(xx),
                   cin, g.data_ptr(), cout, out.data_ptr(), sc.data_ptr(), sc.numel())
        return out

    def col_stats(self, mode: int, a, b=None, mask=None, mean=None):
        a = _dev_f32(a, self.device)
        n, c = a.shape
        out = torch.empty((2, c), dtype=torch.float64, device=self.device)       # fp64 sums (egonn_col_stats)
        sc = self.scratch(4 * c * max(1024, n // 512 + 2))
        self._call(self.lib.egonn_col_stats, mode, a.data_ptr(), _ptr(b), _ptr(mask), _ptr(mean), n, c, out.data_ptr(),
                   sc.data_ptr(), sc.numel())
        return out

    def affine_act(self, x, scale, shift, relu: bool):
        x = _dev_f32(x, self.device)
        out = torch.empty_like(x)
        self._call(self.lib.egonn_affine_act, x.data_ptr(), scale.data_ptr(), shift.data_ptr(), x.shape[0], x.shape[1],
                   int(relu), out.data_ptr())
        return out

    def affine3(self, g, mask, x, A, B, Cc):
        g, x = _dev_f32(g, self.device), _dev_f32(x, self.device)
        out = torch.empty_like(x)
        self._call(self.lib.egonn_affine3, g.data_ptr(), _ptr(mask), x.data_ptr(), A.data_ptr(), B.data_ptr(),
                   Cc.data_ptr(), x.shape[0], x.shape[1], out.data_ptr())
        return out

    def relu_backward(self, grad_out, out):
        g = _dev_f32(grad_out, self.device)
        dx = torch.empty_like(g)
        self._call(self.lib.egonn_relu_backward, g.data_ptr(), out.data_ptr(), g.shape[0], g.shape[1], dx.data_ptr())
        return dx

    def act_backward(self, act: int, grad_out, out):
        g = _dev_f32(grad_out, self.device)
        dx = torch.empty_like(g)
        self._call(self.lib.egonn_act_backward, act, g.data_ptr(), out.data_ptr(), g.shape[0], g.shape[1], dx.data_ptr())
        return dx

    def l2_normalize(self, x, grad_out=None):
        x = _dev_f32(x, self.device)
        g = None if grad_out is None else _dev_f32(grad_out, self.device)
        out = torch.empty_like(x)
        self._call(self.lib.egonn_l2_normalize, x.data_ptr(), _ptr(g), x.shape[0], x.shape[1], out.data_ptr())
        return out

    def gate_residual(self, level, x, gate, residual, relu: bool = True):
        x = _dev_f32(x, self.device)
        assert x.shape[0] == self.level_count(level)
        out = torch.empty_like(x)
        self._call(self.lib.egonn_gate_residual, self.h, level, x.data_ptr(), _ptr(gate), _ptr(residual), x.shape[1],
                   int(relu), out.data_ptr())
        return out

    def gate_residual_backward(self, level, grad_out, out, gate, want_residual: bool = True):
        g = _dev_f32(grad_out, self.device)
        dx = torch.empty_like(g)
        dres = torch.empty_like(g) if want_residual else None
        self._call(self.lib.egonn_gate_residual_backward, self.h, level, g.data_ptr(), _ptr(out), _ptr(gate), g.shape[1],
                   dx.data_ptr(), _ptr(dres))
        return dx, dres

    def segment_sums(self, level, mode, a, b=None, x2=None, p=None):
        a = _dev_f32(a, self.device)
        c = a.shape[1]
        out = torch.empty((self.batch_size, c), dtype=torch.float32, device=self.device)
        sc = self.scratch(32 * self.batch_size * c)
        self._call(self.lib.egonn_segment_sums, self.h, level, mode, a.data_ptr(), _ptr(b), _ptr(x2), _ptr(p), c,
                   out.data_ptr(), sc.data_ptr(), sc.numel())
        return out

    def segment_broadcast(self, level, v, mean: bool):
        v = _dev_f32(v, self.device)
        out = torch.empty((self.level_count(level), v.shape[1]), dtype=torch.float32, device=self.device)
        self._call(self.lib.egonn_segment_broadcast, self.h, level, v.data_ptr(), v.shape[1], int(mean), out.data_ptr())
        return out

    def gem_backward(self, level, x, coef, p):
        x, coef = _dev_f32(x, self.device), _dev_f32(coef, self.device)
        dx = torch.empty_like(x)
        self._call(self.lib.egonn_gem_backward, self.h, level, x.data_ptr(), coef.data_ptr(), p.data_ptr(), x.shape[1],
                   dx.data_ptr())
        return dx

    # the operators below take their tensors as the train graph holds them (fp32, contiguous, on the device): raw pointers
    def eca_gate(self, mean, w):
        """sigmoid(Conv1d_k(mean)) over the channel axis of the (B, C) per-sample means; w (k,)"""
        B, c = mean.shape
        gate = torch.empty_like(mean)
        self._call(self.lib.egonn_eca_gate, mean.data_ptr(), w.data_ptr(), w.numel(), B, c, gate.data_ptr())
        return gate

    def eca_gate_backward(self, grad_out, gate, mean, w):
        """(grad mean, grad w (k,))"""
        B, c = mean.shape
        dmean = torch.empty_like(mean)
        dw = torch.empty(w.numel(), dtype=torch.float32, device=mean.device)
        self._call(self.lib.egonn_eca_gate_backward, grad_out.data_ptr(), gate.data_ptr(), mean.data_ptr(), w.data_ptr(),
                   w.numel(), B, c, dmean.data_ptr(), dw.data_ptr())
        return dmean, dw

    def se_gate_backward(self, grad_out, gate, hid, mean, w1, w2):
        """(grad mean, grad w1, grad b1, grad w2, grad b2) of se_gate"""
        B, c = mean.shape
        h = w1.shape[0]
        dmean, dw1, dw2 = torch.empty_like(mean), torch.empty_like(w1), torch.empty_like(w2)
        db1 = torch.empty(h, dtype=torch.float32, device=mean.device)
        db2 = torch.empty(c, dtype=torch.float32, device=mean.device)
        self._call(self.lib.egonn_se_gate_backward, grad_out.data_ptr(), gate.data_ptr(), hid.data_ptr(), mean.data_ptr(),
                   w1.data_ptr(), w2.data_ptr(), B, c, h, dmean.data_ptr(), dw1.data_ptr(), db1.data_ptr(), dw2.data_ptr(),
                   db2.data_ptr())
        return dmean, dw1, db1, dw2, db2

    def bn_train_finalize(self, sums, shift, total: float, weight, bias, eps: float, momentum: float, running_mean=None,
                          running_var=None):
        """(2, C) fp64 shifted sums of col_stats(3) -> (4, C): mean, invstd, folded scale, folded shift; updates the running
        statistics in place when given."""
        c = weight.numel()
        out4 = torch.empty((4, c), dtype=torch.float32, device=sums.device)
        self._call(self.lib.egonn_bn_train_finalize, sums.data_ptr(), shift.data_ptr(), total, c, weight.data_ptr(),
                   bias.data_ptr(), float(eps), float(momentum), _ptr(running_mean), _ptr(running_var), out4.data_ptr())
        return out4

    def bn_backward_finalize(self, sums, sums_all, total: float, weight, mean, invstd):
        """this rank's and the whole batch's (2, C) fp64 sums of col_stats(2) -> (5, C): A, B, C of affine3, dgamma, dbeta"""
        c = weight.numel()
        out5 = torch.empty((5, c), dtype=torch.float32, device=sums.device)
        self._call(self.lib.egonn_bn_backward_finalize, sums.data_ptr(), sums_all.data_ptr(), total, c, weight.data_ptr(),
                   mean.data_ptr(), invstd.data_ptr(), out5.data_ptr())
        return out5

    def forward_level_features(self, level: int, channels: int) -> torch.Tensor:
        out = torch.empty((self.level_count(level), channels), dtype=torch.float32, device=self.device)
        self._call(self.lib.egonn_forward_level_features, self.h, level, out.data_ptr(), channels)
        return out

    def select_keypoints(self, sigma: torch.Tensor, keypoints: torch.Tensor, descriptors: torch.Tensor, n_k: int):
        B = self.batch_size
        dev = self.device
        sel_kp = torch.empty((B, n_k, 3), dtype=torch.float32, device=dev)
        sel_desc = torch.empty((B, n_k, descriptors.shape[1]), dtype=torch.float32, device=dev)
        sel_rows = torch.empty((B, n_k), dtype=torch.int32, device=dev)
        sel_count = torch.empty((B,), dtype=torch.int32, device=dev)
        self._call(self.lib.egonn_select_keypoints, self.h, sigma.data_ptr(), keypoints.data_ptr(), descriptors.data_ptr(), n_k,
                   sel_kp.data_ptr(), sel_desc.data_ptr(), sel_rows.data_ptr(), sel_count.data_ptr())
        return sel_kp, sel_desc, sel_rows, sel_count

    # ------------------------------------------------------------------ launch timing
    def profile_enable(self, mode: int, filt: str = ""):
        check(self.lib.egonn_profile_enable(self.h, mode, filt.encode()))

    def profile_fetch(self, cap: int = 4096):
        n = C.c_int()
        names = C.create_string_buffer(cap * 64)
        ms = (C.c_float * cap)()
        by = (C.c_double * cap)()
        fl = (C.c_double * cap)()
        self._call(self.lib.egonn_profile_fetch, self.h, cap, C.byref(n), names, ms, by, fl)
        out = []
        for i in range(n.value):
            nm = names.raw[i * 64:(i + 1) * 64].split(b"\0", 1)[0].decode()
            out.append((nm, float(ms[i]), float(by[i]), float(fl[i])))
        return out


class ModelHandle:
    """egonn_model: weights registered under the reference's state_dict keys."""

    def __init__(self):
        self.lib = load()
        h = _P()
        check(self.lib.egonn_model_create(C.byref(h)))
        self.h = h
        self._keep = {}

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.lib.egonn_model_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def set_tensor(self, key: str, t: torch.Tensor):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous(), key
        shape = (C.c_int64 * max(t.dim(), 1))(*t.shape)
        check(self.lib.egonn_model_set_tensor(self.h, key.encode(), t.data_ptr(), t.dim(), shape))
        self._keep[key] = t

    def finalize(self):
        check(self.lib.egonn_model_finalize(self.h, _stream()))

    def finalize_minkfpn(self, planes: Sequence[int], layers: Sequence[int], num_top_down: int, feature_size: int, block: int,
                         pooling: int):
        """egonn_minkfpn_finalize: the registered tensors as a MinkFPN + pooling model (folds and packs once)"""
        n = len(planes)
        assert len(layers) == n
        check(self.lib.egonn_minkfpn_finalize(self.h, n, (C.c_int * max(n, 1))(*planes), (C.c_int * max(n, 1))(*layers),
                                              int(num_top_down), int(feature_size), int(block), int(pooling), _stream()))


def minkfpn_out_level(n_levels: int, num_top_down: int) -> int:
    lv = C.c_int()
    check(load().egonn_minkfpn_out_level(int(n_levels), int(num_top_down), C.byref(lv)))
    return lv.value
