"""ctypes binding of the gfx950 kernel library (``include/disyolo.h``).

There is no CPU fallback: if ``libdisyolo_hip.so`` is missing or an entry point
returns an error, this module raises.  PyTorch is used only to own device memory
and streams; kernels receive raw device pointers and the current HIP stream.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DISYOLO_LIB", os.path.join(_HERE, "libdisyolo_hip.so"))

GRAD_LD = 32
MAX_BOXES = 256            # DISYOLO_MAX_BOXES: ground-truth boxes per image (yolo_loss, mask_rois, shuffle_perm)
MAX_DET = 256              # DISYOLO_MAX_DET: detections per image (detect, mask_rois, the batched paste)
ROI_MAX = 16
ROI_W = 12
ROI_CAP = 512              # DISYOLO_ROI_CAP: rows of the RoI table the _x forms of mask_rois / psroi_loss take
K_MAPS = (3, 5, 7)          # position-sensitive grids the mask path covers (the reference's list)
MASK_STRIDES = (1, 2, 4)    # GT mask -> score map sampling steps psroi_loss_s covers (score maps at S, S/2, S/4)
# which candidates above the score threshold the detection filter keeps (DISYOLO_NMS_* of disyolo.h; filter_detections,
# yolo/yolo3_net_pos.py:564-592 / 594-605 / nms=False)
NMS_MODES = {"per_class": 0, "agnostic": 1, "none": 2}


def roi_w(k: int) -> int:
    """int32 words per RoI row of a k x k grid (DISYOLO_ROI_W_K): gy0..gyk, gx0..gxk, gt_row, area, valid, 0"""
    return 2 * (k + 1) + 4


def block32_post(k: int) -> int:
    """``post`` code of block32_fused_fwd for the mask head of a k x k grid (1, 2, 3 for k = 3, 5, 7)"""
    return {3: 1, 5: 2, 7: 3}[k]
CONV_LEAKY, CONV_OUT_F32, CONV_STATS, CONV_BN_BWD_STATS, CONV_BN_FUSED, CONV_BN_BWD_FUSED = 1, 2, 4, 8, 16, 32


class DisyoloError(RuntimeError):
    pass


class ConvDesc(C.Structure):
    """mirror of ``disyolo_conv_desc`` (include/disyolo.h)"""
    _fields_ = [
        ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
        ("C0", C.c_int32), ("C1", C.c_int32),
        ("Ho", C.c_int32), ("Wo", C.c_int32), ("Cout", C.c_int32),
        ("ksize", C.c_int32), ("stride", C.c_int32),
        ("pad_t", C.c_int32), ("pad_l", C.c_int32),
        ("in_div", C.c_int32), ("flags", C.c_int32),
        ("alpha", C.c_float), ("tile", C.c_int32),
        ("x0", C.c_void_p), ("x1", C.c_void_p), ("w", C.c_void_p),
        ("scale", C.c_void_p), ("shift", C.c_void_p), ("residual", C.c_void_p),
        ("y", C.c_void_p), ("stats", C.c_void_p),
        ("bn_x", C.c_void_p), ("bn_scale", C.c_void_p), ("bn_shift", C.c_void_p), ("bn_mean", C.c_void_p),
        ("bn_rstd", C.c_void_p), ("bn_partials", C.c_void_p), ("bn_alpha", C.c_float),
        ("bn_decay", C.c_float), ("bn_eps", C.c_float),
        ("y_act", C.c_void_p), ("bn_gamma", C.c_void_p), ("bn_beta", C.c_void_p),
        ("bn_moving_mean", C.c_void_p), ("bn_moving_var", C.c_void_p),
        ("bn_out_scale", C.c_void_p), ("bn_out_shift", C.c_void_p), ("bn_out_mean", C.c_void_p), ("bn_out_rstd", C.c_void_p),
        ("bn_dgamma", C.c_void_p), ("bn_dbeta", C.c_void_p), ("cluster_sync", C.c_void_p),
    ]


_SIGS = {
    "disyolo_version": (C.c_int, []),
    "disyolo_last_error": (C.c_char_p, []),
    "disyolo_conv_desc_size": (C.c_size_t, []),
    "disyolo_find_contours": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int,
                                        C.POINTER(C.c_int), C.POINTER(C.c_int64)]),
    "disyolo_conv2d_stats_rows": (C.c_int, [C.POINTER(ConvDesc)]),
    "disyolo_conv2d_bn_bwd_stats_ok": (C.c_int, [C.POINTER(ConvDesc)]),
    "disyolo_conv2d_bn_fused_ok": (C.c_int, [C.POINTER(ConvDesc)]),
    "disyolo_cluster_sync_words": (C.c_int, [C.c_int]),
    "disyolo_cluster_sync_error": (C.c_int, [C.c_void_p, C.c_int]),
    "disyolo_conv2d_fwd": (C.c_int, [C.POINTER(ConvDesc), C.c_void_p]),
    "disyolo_conv2d_tile": (C.c_int, [C.POINTER(ConvDesc)] + [C.POINTER(C.c_int)] * 4),
    "disyolo_conv_first_fwd": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 4 + [C.c_float, C.c_void_p]),
    "disyolo_conv12_fused_ok": (C.c_int, [C.c_int] * 3),
    "disyolo_conv12_fused_fwd": (C.c_int, [C.c_void_p] * 8 + [C.c_int] * 3 + [C.c_float, C.c_void_p]),
    "disyolo_block32_fused_ok": (C.c_int, [C.c_int] * 6),
    "disyolo_block64_fused_ok": (C.c_int, [C.c_int] * 4),
    "disyolo_pack_quad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "disyolo_dgrad_s2_quad_ok": (C.c_int, [C.c_int] * 5),
    "disyolo_dgrad_s2_quad": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 5 + [C.c_void_p]),
    "disyolo_block64_fused_fwd": (C.c_int, [C.c_void_p] * 8 + [C.c_int] * 4 + [C.c_float, C.c_void_p]),
    "disyolo_block32_fused_fwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 6 + [C.c_int] +
                                  [C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_float, C.c_void_p]),
    "disyolo_conv2d_wgrad_workspace": (C.c_size_t, [C.POINTER(ConvDesc), C.c_int]),
    "disyolo_conv2d_wgrad": (C.c_int, [C.POINTER(ConvDesc), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                       C.c_size_t, C.c_int, C.c_void_p]),
    "disyolo_conv2d_fp8_fwd": (C.c_int, [C.POINTER(ConvDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float,
                                         C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]),
    "disyolo_conv_first_fwd_fp8": (C.c_int, [C.c_void_p] * 5 + [C.c_float] + [C.c_int] * 4 + [C.c_float, C.c_void_p]),
    "disyolo_quant_fp8": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_float, C.c_void_p]),
    "disyolo_dequant_fp8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_void_p]),
    "disyolo_pack_weights_fp8": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int] * 3 + [C.c_float, C.c_void_p]),
    "disyolo_conv2d_wgrad_plan": (C.c_int, [C.POINTER(ConvDesc), C.c_int] + [C.POINTER(C.c_int)] * 4),
    "disyolo_conv_first_wgrad_workspace": (C.c_size_t, [C.c_int] * 4),
    "disyolo_conv_first_wgrad": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 4 + [C.c_void_p, C.c_size_t, C.c_void_p]),
    "disyolo_image_pad8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "disyolo_copy2d_f32": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p]),
    "disyolo_pack_weights": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 4 + [C.c_void_p]),
    "disyolo_pack_table_bytes": (C.c_size_t, [C.c_int]),
    "disyolo_pack_table_build": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int)]),
    "disyolo_pack_all": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "disyolo_bn_finalize": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int64] + [C.c_void_p] * 4 +
                            [C.c_float, C.c_float] + [C.c_void_p] * 5),
    "disyolo_colstats_rows": (C.c_int, [C.c_int64, C.c_int]),
    "disyolo_colstats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]),
    "disyolo_bn_fold": (C.c_int, [C.c_void_p] * 4 + [C.c_float] + [C.c_void_p] * 2 + [C.c_int, C.c_void_p]),
    "disyolo_bn_act_fwd": (C.c_int, [C.c_void_p] * 5 + [C.c_int64, C.c_int, C.c_float, C.c_void_p]),
    "disyolo_bn_act_bwd_workspace": (C.c_size_t, [C.c_int64, C.c_int]),
    "disyolo_bn_act_bwd_partials_workspace": (C.c_size_t, [C.c_int]),
    "disyolo_bn_act_bwd_partials": (C.c_int, [C.c_void_p] * 9 + [C.c_int64, C.c_int, C.c_float, C.c_void_p, C.c_int,
                                              C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "disyolo_bn_partial_sums": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "disyolo_bn_finalize_sums": (C.c_int, [C.c_void_p, C.c_int, C.c_int64] + [C.c_void_p] * 4 + [C.c_float, C.c_float] +
                                 [C.c_void_p] * 5),
    "disyolo_bn_bwd_reduce_rows": (C.c_int, [C.c_int64, C.c_int]),
    "disyolo_bn_bwd_reduce": (C.c_int, [C.c_void_p] * 6 + [C.c_int64, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_size_t,
                                        C.c_void_p]),
    "disyolo_bn_bwd_apply_sums": (C.c_int, [C.c_void_p] * 8 + [C.c_int64] + [C.c_void_p] * 3 + [C.c_int64, C.c_int, C.c_float,
                                            C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "disyolo_bn_act_bwd": (C.c_int, [C.c_void_p] * 9 + [C.c_int64, C.c_int, C.c_float, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t,
                                                       C.c_void_p]),
    "disyolo_bn_frozen_bwd": (C.c_int, [C.c_void_p] * 5 + [C.c_int64, C.c_int, C.c_float, C.c_void_p, C.c_int, C.c_void_p]),
    "disyolo_upsample2x_bwd": (C.c_int, [C.c_void_p] * 2 + [C.c_int] * 7 + [C.c_void_p]),
    "disyolo_colsum_workspace": (C.c_size_t, [C.c_int64, C.c_int]),
    "disyolo_colsum": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                 C.c_void_p]),
    "disyolo_detect_workspace": (C.c_size_t, [C.c_int] * 3),
    "disyolo_detect": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_void_p] * 2 + [C.c_float, C.c_float, C.c_int] +
                       [C.c_void_p] * 3 + [C.c_size_t, C.c_void_p]),
    "disyolo_detect_workspace_hw": (C.c_size_t, [C.c_int] * 4),
    "disyolo_detect_hw": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 4 + [C.c_void_p] * 2 + [C.c_float, C.c_float, C.c_int] +
                          [C.c_void_p] * 3 + [C.c_size_t, C.c_void_p]),
    "disyolo_detect_list_capacity": (C.c_int, []),
    "disyolo_detect_nms_hw": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 4 + [C.c_void_p] * 2 +
                              [C.c_float, C.c_float, C.c_int, C.c_int] + [C.c_void_p] * 3 + [C.c_size_t, C.c_void_p]),
    "disyolo_detect_workspace_x": (C.c_size_t, [C.c_int] * 5),
    "disyolo_detect_x": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 4 + [C.c_void_p] * 2 +
                         [C.c_float, C.c_float, C.c_int, C.c_int] + [C.c_void_p] * 3 + [C.c_size_t, C.c_void_p]),
    "disyolo_yolo_loss_workspace": (C.c_size_t, [C.c_int] * 3),
    "disyolo_yolo_loss_workspace_hw": (C.c_size_t, [C.c_int] * 4),
    "disyolo_yolo_loss_hw": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p, C.c_float] +
                             [C.c_void_p] * 4 + [C.c_size_t, C.c_void_p]),
    "disyolo_yolo_loss": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p, C.c_float] +
                          [C.c_void_p] * 4 + [C.c_size_t, C.c_void_p]),
    "disyolo_yolo_loss_wide": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 5 + [C.c_void_p, C.c_float] +
                               [C.c_void_p] * 4 + [C.c_size_t, C.c_void_p]),
    "disyolo_shuffle_perm": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p]),
    "disyolo_mask_rois": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p] + [C.c_int] * 4 +
                          [C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "disyolo_mask_rois_k": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p] + [C.c_int] * 5 +
                            [C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "disyolo_mask_rois_hw": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p] + [C.c_int] * 6 +
                             [C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "disyolo_psroi_loss_workspace": (C.c_size_t, [C.c_int, C.c_int]),
    "disyolo_psroi_loss_workspace_hw": (C.c_size_t, [C.c_int] * 3),
    "disyolo_psroi_loss_hw": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p] + [C.c_int] * 5 +
                              [C.c_float] + [C.c_void_p] * 3 + [C.c_size_t, C.c_void_p]),
    "disyolo_mask_rois_x": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p] + [C.c_int] * 6 +
                            [C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "disyolo_psroi_loss_workspace_x": (C.c_size_t, [C.c_int] * 4),
    "disyolo_psroi_loss_x": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p] + [C.c_int] * 6 +
                             [C.c_float] + [C.c_void_p] * 3 + [C.c_size_t, C.c_void_p]),
    "disyolo_psroi_assemble_hw": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int] * 5 + [C.c_void_p] * 3),
    "disyolo_psroi_loss": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p] + [C.c_int] * 3 +
                           [C.c_float] + [C.c_void_p] * 3 + [C.c_size_t, C.c_void_p]),
    "disyolo_psroi_loss_s": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p] + [C.c_int] * 4 +
                             [C.c_float] + [C.c_void_p] * 3 + [C.c_size_t, C.c_void_p]),
    "disyolo_psroi_assemble": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] * 3),
    "disyolo_mask_paste": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                     C.c_void_p, C.c_void_p]),
    "disyolo_mask_paste_hw": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                        C.c_void_p, C.c_void_p, C.c_void_p]),
    "disyolo_letterbox": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "disyolo_letterbox_hw": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "disyolo_tile_gather": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                      C.c_int, C.c_void_p]),
    "disyolo_tile_paste_bits": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                          C.c_void_p]),
    "disyolo_tile_seam_counts": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                           C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                           C.c_void_p]),
    "disyolo_tile_compose_blocks": (C.c_int, [C.c_int64]),
    "disyolo_tile_compose": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                       C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                       C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "disyolo_tile_group_counts_blocks": (C.c_int, [C.c_int64]),
    "disyolo_tile_group_counts": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                            C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                            C.c_void_p, C.c_void_p]),
    "disyolo_measure_d2": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "disyolo_measure_thin": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "disyolo_measure_counts": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "disyolo_skeleton_classify": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p]),
    "disyolo_skeleton_label": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p]),
    "disyolo_skeleton_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "disyolo_skeleton_prune": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_int64, C.c_void_p, C.c_void_p]),
    "disyolo_trace_nodes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64] + [C.c_void_p] * 5 + [C.c_int64, C.c_void_p,
                                      C.c_void_p]),
    "disyolo_trace_rank": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64] + [C.c_void_p] * 5 + [C.c_int64, C.c_void_p,
                                     C.c_int64, C.c_int] + [C.c_void_p] * 6),
    "disyolo_trace_edges": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64] +
                            [C.c_void_p] * 4 + [C.c_int64, C.c_void_p]),
    "disyolo_trace_gather": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64] +
                             [C.c_void_p] * 4 + [C.c_int64] + [C.c_void_p] * 4 + [C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                                                                                 C.c_void_p, C.c_void_p]),
    "disyolo_shape_sums": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "disyolo_shape_parts": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p]),
    "disyolo_shape_extents": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int,
                                        C.c_void_p, C.c_void_p]),
    "disyolo_outline_edges": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64] + [C.c_void_p] * 6 +
                              [C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "disyolo_outline_loops": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64] + [C.c_void_p] * 7 +
                              [C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "disyolo_outline_gather": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                         C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]),
    "disyolo_confusion16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "disyolo_confusion_n": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]),
    "disyolo_paste_job_size": (C.c_size_t, []),
    "disyolo_paste_job_plan": (C.c_int, [C.c_void_p, C.c_int]),
    "disyolo_mask_paste_iou_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "disyolo_mask_paste_iou_batch_hw": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "disyolo_paste_job_plan_x": (C.c_int, [C.c_void_p, C.c_int]),
    "disyolo_mask_paste_iou_batch_x": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "disyolo_adam_step": (C.c_int, [C.c_void_p] * 4 + [C.c_int64, C.c_int64] + [C.c_float] * 5 + [C.c_int64, C.c_float,
                                                                                             C.c_void_p]),
    "disyolo_adam_step_dev": (C.c_int, [C.c_void_p] * 4 + [C.c_int64, C.c_int64] + [C.c_float] * 5 + [C.c_void_p, C.c_float,
                                                                                                 C.c_void_p]),
    "disyolo_adam_fused_workspace": (C.c_size_t, [C.c_int64]),
    "disyolo_adam_sweep_parts": (C.c_int, [C.c_int64]),
    "disyolo_adam_sweep": (C.c_int, [C.c_void_p] * 4 + [C.c_int64, C.c_int64, C.c_void_p] + [C.c_float] * 4 +
                           [C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]),
    "disyolo_adam_finish": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
    "disyolo_adam_finish_record": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_float] + [C.c_void_p] * 5 + [C.c_int, C.c_void_p]),
    "disyolo_adam_step_fused": (C.c_int, [C.c_void_p] * 4 + [C.c_int64, C.c_int64, C.c_void_p] + [C.c_float] * 4 +
                                [C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "disyolo_add_bf16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]),
    "disyolo_cmdlist_create": (C.c_void_p, []),
    "disyolo_cmdlist_destroy": (None, [C.c_void_p]),
    "disyolo_cmdlist_begin": (C.c_int, [C.c_void_p]),
    "disyolo_cmdlist_end": (C.c_int, []),
    "disyolo_cmdlist_size": (C.c_int, [C.c_void_p]),
    "disyolo_cmdlist_count": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "disyolo_cmdlist_describe": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int32)]),
    "disyolo_cmdlist_set_lane": (C.c_int, [C.c_int]),
    "disyolo_cmdlist_sync": (C.c_int, [C.c_int, C.c_int]),
    "disyolo_cmdlist_mark": (C.c_int, [C.c_int]),
    "disyolo_cmdlist_wait": (C.c_int, [C.c_int, C.c_int]),
    "disyolo_cmdlist_mark_slot": (C.c_int, [C.c_int, C.c_int]),
    "disyolo_cmdlist_wait_slot": (C.c_int, [C.c_int, C.c_int]),
    "disyolo_cmdlist_run": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "disyolo_cmdlist_run_ex": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]),
    "disyolo_cmdlist_side_stream": (C.c_void_p, [C.c_void_p]),
    "disyolo_cmdlist_lane_stream": (C.c_void_p, [C.c_void_p, C.c_int]),
    "disyolo_lanes_reserve": (C.c_int, [C.c_int]),
    "disyolo_lanes_report": (C.c_int, [C.c_char_p, C.c_int]),
    "disyolo_comm_load": (C.c_int, [C.c_char_p, C.POINTER(C.c_int)]),
    "disyolo_comm_unique_id": (C.c_int, [C.c_void_p]),
    "disyolo_comm_init": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "disyolo_comm_destroy": (C.c_int, [C.c_void_p]),
    "disyolo_comm_allreduce_sum": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]),
    "disyolo_comm_reduce_scatter_sum": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]),
    "disyolo_comm_all_gather": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]),
    "disyolo_cast_f32_bf16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "disyolo_cast_bf16_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "disyolo_polygon_mask": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 3 + [C.c_void_p, C.c_void_p]),
    "disyolo_aug_place": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p]),
    "disyolo_aug_place_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "disyolo_aug_salt_pepper": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "disyolo_aug_change_light": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_void_p]),
    "disyolo_aug_motion_blur3": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "disyolo_aug_place_hw": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p] + [C.c_int] * 7 + [C.c_void_p]),
    "disyolo_aug_place_batch_hw": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "disyolo_aug_salt_pepper_hw": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "disyolo_aug_change_light_hw": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_void_p]),
    "disyolo_aug_motion_blur3_hw": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "disyolo_aug_to_float": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "disyolo_window_job_size": (C.c_size_t, []),
    "disyolo_window_visible": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "disyolo_window_targets": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p] * 6),
    "disyolo_window_place_masks": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "disyolo_crc32c": (C.c_uint32, [C.c_void_p, C.c_size_t, C.c_uint32]),
    "disyolo_l2_workspace": (C.c_size_t, [C.c_int64]),
    "disyolo_l2_loss": (C.c_int, [C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
}

EXPORTS = tuple(_SIGS)
_lib = None


def load() -> C.CDLL:
    """Load the kernel library; raises DisyoloError when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise DisyoloError(
                "%s not found: build it with `make -C dis-yolo_amd/csrc` (or __graft_entry__.build()); "
                "there is no CPU fallback" % LIB_PATH)
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        if lib.disyolo_conv_desc_size() != C.sizeof(ConvDesc):
            raise DisyoloError("%s was built from a different include/disyolo.h (conv descriptor %d bytes, this "
                               "binding %d): rebuild it" % (LIB_PATH, lib.disyolo_conv_desc_size(), C.sizeof(ConvDesc)))
        if lib.disyolo_paste_job_size() != PASTE_JOB.itemsize:
            raise DisyoloError("%s was built from a different include/disyolo.h (paste job %d bytes, this binding %d): "
                               "rebuild it" % (LIB_PATH, lib.disyolo_paste_job_size(), PASTE_JOB.itemsize))
        if lib.disyolo_window_job_size() != WINDOW_JOB.itemsize:
            raise DisyoloError("%s was built from a different include/disyolo.h (window job %d bytes, this binding %d): "
                               "rebuild it" % (LIB_PATH, lib.disyolo_window_job_size(), WINDOW_JOB.itemsize))
        _lib = lib
    return _lib


def _check(rc: int, what: str) -> None:
    if rc != 0:
        raise DisyoloError("%s failed (%d): %s" % (what, rc, load().disyolo_last_error().decode()))


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _need(t: torch.Tensor, dtype, name: str) -> None:
    if t.dtype != dtype or not t.is_cuda or not t.is_contiguous():
        raise DisyoloError("%s must be a contiguous CUDA tensor of %s (got %s on %s)" % (name, dtype, t.dtype, t.device))


def _need_shape(t: torch.Tensor, shape, name: str) -> None:
    if tuple(t.shape) != tuple(shape):
        raise DisyoloError("%s must have shape %s (got %s)" % (name, tuple(shape), tuple(t.shape)))


class Workspace:
    """Grow-only device scratch buffer handed to the kernels that need one.  Once a command
    list has captured its address it is frozen: a later request that does not fit raises
    instead of silently moving the buffer."""

    def __init__(self, device):
        self.device = device
        self.buf = torch.empty(1 << 20, dtype=torch.uint8, device=device)
        self.frozen = False

    def get(self, nbytes: int) -> torch.Tensor:
        if self.buf.numel() < nbytes:
            if self.frozen:
                raise DisyoloError("workspace of %d bytes is frozen by a recorded command list; %d requested"
                                   % (self.buf.numel(), nbytes))
            self.buf = torch.empty(int(nbytes * 1.25) + 256, dtype=torch.uint8, device=self.device)
        return self.buf


class CmdList:
    """Recorded sequence of kernel-library calls replayed by one C call (csrc/runtime.hip)."""

    def __init__(self):
        self.h = load().disyolo_cmdlist_create()
        self.keep = []           # tensors / descriptors referenced by the recorded commands
        self._side = None        # side_stream()'s torch wrapper
        self._lanes = {}

    def __del__(self):
        try:
            if self.h:
                if torch.cuda.is_available() and (self._side is not None or self._lanes):
                    # a side lane may still be running: the caller's stream waits before streams / buffers are released
                    for st in [self._side] + list(self._lanes.values()):
                        if st is not None:
                            torch.cuda.current_stream(st.device).wait_stream(st)
                load().disyolo_cmdlist_destroy(self.h)
        except Exception:
            pass

    def __enter__(self):
        global TIMER
        if TIMER is not None:
            raise DisyoloError("cannot record a command list while the kernel timer is active")
        _check(load().disyolo_cmdlist_begin(self.h), "cmdlist_begin")
        global CURRENT_LANE
        CURRENT_LANE = 0
        return self

    def __exit__(self, *exc):
        _check(load().disyolo_cmdlist_end(), "cmdlist_end")
        global CURRENT_LANE
        CURRENT_LANE = 0
        return False

    def size(self) -> int:
        return load().disyolo_cmdlist_size(self.h)

    def count(self, what: str, lane: int) -> int:
        """packets a replay puts on ``lane``: what = "launches" | "records" | "waits" """
        return load().disyolo_cmdlist_count(self.h, {"launches": 0, "records": 1, "waits": 2}[what], lane)

    def describe(self) -> list:
        """(kind, lane, from, to) of every command, as the list holds them (include/disyolo.h: disyolo_cmdlist_describe)"""
        out = (C.c_int32 * 4)()
        cmds = []
        for i in range(self.size()):
            _check(load().disyolo_cmdlist_describe(self.h, i, out), "cmdlist_describe")
            cmds.append(tuple(out))
        return cmds

    def run(self, first: int = 0, last: Optional[int] = None, fork: bool = True, join: bool = True) -> None:
        last = self.size() if last is None else last
        _check(load().disyolo_cmdlist_run_ex(self.h, first, last, _stream(), (1 if fork else 0) | (2 if join else 0)),
               "cmdlist_run")

    def side_stream(self, device) -> "torch.cuda.Stream":
        """the side lane as a torch stream (to order an RCCL collective, or the caller's stream, after it).  The wrapper
        lives and dies with this list: the HIP stream is destroyed with it"""
        if self._side is None:
            self._side = torch.cuda.ExternalStream(load().disyolo_cmdlist_side_stream(self.h), device=device)
        return self._side

    def lane_stream(self, lane: int, device) -> "torch.cuda.Stream":
        """lane 1..3 of this list as a torch stream (same ownership as side_stream)"""
        if lane == 1:
            return self.side_stream(device)
        if lane not in self._lanes:
            self._lanes[lane] = torch.cuda.ExternalStream(load().disyolo_cmdlist_lane_stream(self.h, lane), device=device)
        return self._lanes[lane]


def same_pads(size: int, k: int, s: int):
    """TF 'SAME' geometry: (out, pad_before)."""
    out = -(-size // s)
    total = max((out - 1) * s + k - size, 0)
    return out, total // 2


def make_conv_desc(x0, w_packed, y, ksize, stride, *, x1=None, scale=None, shift=None, residual=None, stats=None,
                   leaky=False, out_f32=False, alpha=0.1, tile=0, in_div=1, pads=None, out_hw=None,
                   bn_bwd=None, bn_fused=None, bn_bwd_fused=None) -> ConvDesc:
    """``bn_bwd`` = (x, scale, shift, mean, rstd, partials, alpha) of the batch-normalised layer whose output
    gradient ``y`` becomes final with this conv: its batch-norm backward sums are emitted by the epilogue (only the
    3x3 patch kernel can: check ``conv2d_bn_bwd_stats_ok`` on the descriptor without it first).
    ``bn_fused`` = dict(y_act, gamma, beta, mm, mv, scale, shift, mean, rstd, decay, eps, sync): training-mode batch norm
    inside the launch (DISYOLO_CONV_BN_FUSED; ``stats`` must be given, ``y`` receives the raw conv output, ``y_act`` the
    activation; check ``conv2d_bn_fused_ok`` on a descriptor without it first).
    ``bn_bwd_fused`` = dict(dgamma, dbeta, sync) on top of ``bn_bwd``: the target's whole batch-norm backward inside this
    data-gradient conv (``y`` receives dx of the target's conv output)."""
    B, H, W, C0 = x0.shape
    C1 = 0 if x1 is None else x1.shape[3]
    if out_hw is None:
        Ho, pt = same_pads(H, ksize, stride)
        Wo, pl = same_pads(W, ksize, stride)
    else:
        Ho, Wo = out_hw
        pt, pl = pads
    if pads is not None:
        pt, pl = pads
    d = ConvDesc()
    d.B, d.H, d.W, d.C0, d.C1 = B, H, W, C0, C1
    d.Ho, d.Wo, d.Cout = Ho, Wo, y.shape[-1]
    d.ksize, d.stride, d.pad_t, d.pad_l, d.in_div = ksize, stride, pt, pl, in_div
    d.flags = (CONV_LEAKY if leaky else 0) | (CONV_OUT_F32 if out_f32 else 0) | (CONV_STATS if stats is not None else 0)
    d.alpha, d.tile = alpha, tile
    if tile == 0 and TUNED:
        d.tile = TUNED.get(conv_shape_key(d), 0)
    d.x0, d.x1, d.w = _p(x0), _p(x1), _p(w_packed)
    d.scale, d.shift, d.residual = _p(scale), _p(shift), _p(residual)
    d.y, d.stats = _p(y), _p(stats)
    if bn_bwd is not None:
        d.flags |= CONV_BN_BWD_STATS
        d.bn_x, d.bn_scale, d.bn_shift, d.bn_mean, d.bn_rstd, d.bn_partials = (_p(t) for t in bn_bwd[:6])
        d.bn_alpha = bn_bwd[6]
    if bn_fused is not None:
        f = bn_fused
        if stats is None or leaky or scale is not None or shift is not None or residual is not None:
            raise DisyoloError("make_conv_desc(bn_fused=...): needs stats, and no scale / shift / leaky / residual")
        d.flags |= CONV_BN_FUSED
        d.y_act, d.bn_gamma, d.bn_beta = _p(f["y_act"]), _p(f["gamma"]), _p(f["beta"])
        d.bn_moving_mean, d.bn_moving_var = _p(f.get("mm")), _p(f.get("mv"))
        d.bn_out_scale, d.bn_out_shift, d.bn_out_mean, d.bn_out_rstd = _p(f["scale"]), _p(f["shift"]), _p(f["mean"]), _p(f["rstd"])
        d.bn_decay, d.bn_eps = f["decay"], f["eps"]
        d.cluster_sync = _p(f["sync"])
    if bn_bwd_fused is not None:
        f = bn_bwd_fused
        if bn_bwd is None:
            raise DisyoloError("make_conv_desc(bn_bwd_fused=...): needs bn_bwd")
        d.flags |= CONV_BN_BWD_FUSED
        d.bn_dgamma, d.bn_dbeta, d.cluster_sync = _p(f["dgamma"]), _p(f["dbeta"]), _p(f["sync"])
    # the struct only holds raw pointers: keep the tensors alive as long as the descriptor
    d._keepalive = (x0, x1, w_packed, scale, shift, residual, y, stats, bn_bwd, bn_fused, bn_bwd_fused)
    return d


def conv2d_bn_fused_ok(d: ConvDesc) -> bool:
    """can this descriptor (its shape and tile) run batch norm inside the launch -- a kernel with the epilogue and a grid
    that is resident at once on this device?  (make_conv_desc(bn_fused=...) / (bn_bwd_fused=...))"""
    return load().disyolo_conv2d_bn_fused_ok(C.byref(d)) == 1


def cluster_sync_buffer(cout: int, device) -> torch.Tensor:
    """the counters of one layer's in-launch exchange (zeroed once; the launches leave them zero) + its error word"""
    return torch.zeros(load().disyolo_cluster_sync_words(cout), dtype=torch.int32, device=device)


def cluster_sync_error(buf: torch.Tensor, cout: int) -> int:
    return load().disyolo_cluster_sync_error(_p(buf), cout)


def conv2d_bn_bwd_stats_ok(d: ConvDesc) -> bool:
    """does this descriptor run a kernel that can emit the batch-norm backward sums (make_conv_desc(bn_bwd=...))?"""
    return load().disyolo_conv2d_bn_bwd_stats_ok(C.byref(d)) == 1


def conv2d_stats_rows(d: ConvDesc) -> int:
    r = load().disyolo_conv2d_stats_rows(C.byref(d))
    if r < 0:
        raise DisyoloError("conv2d_stats_rows: bad descriptor")
    return r


def conv_shape_key(d: ConvDesc):
    """what the tile choice depends on: the GEMM shape and the gather variant (not the epilogue:
    the batch-norm partial-sum rows are sized from a descriptor without one)"""
    return (d.B, d.H, d.W, d.C0, d.C1, d.Ho, d.Wo, d.Cout, d.ksize, d.stride, d.in_div)


# shape key -> tile code, filled by ConvTuner (YOLONet.autotune); consulted by make_conv_desc
TUNED: dict = {}
TUNE_CANDIDATES = (3, 0x203, 6, 0x206, 2, 0x202, 0x204, 10, 12, 0x20c, 0x10c, 0x108, 0x20d, 16, 17, 18, 19, 20, 21, 24, 25)
# (tiles 26 / 27 / 28 -- two-wave 32x64, 64x32, 32x128 GEMM tiles, round 5 -- cover every shape and won nowhere in the step:
# profiles/r05_two_wave_tiles.txt; pass them explicitly to try them)


class ConvTuner:
    """In-sequence tile autotuner.  Stand-alone timing loops keep a layer's operands hot in L2
    and rank the tiles differently from how they behave inside the step (measured: DESIGN.md),
    so the candidates are timed where they run: while ``active`` every conv2d_fwd launch is
    bracketed with HIP events and uses the candidate of the current pass; the best candidate
    per shape key goes to ``TUNED``."""

    def __init__(self, candidates=TUNE_CANDIDATES):
        self.candidates = tuple(candidates)
        self.current = 0              # tile code of the running pass (0 = launcher heuristic)
        self.events = {}              # (key, cand) -> [(start, end)]
        self.stats_rows = {}          # stats buffer address -> partial-sum rows the last launch into it wrote
        self.covers = {}              # (key, cand) -> does the candidate's kernel cover the shape (else the launcher falls back)

    def launch(self, d: ConvDesc) -> None:
        key = conv_shape_key(d)
        keep = d.tile
        d.tile = self.current
        ck = (key, self.current)
        if ck not in self.covers:
            # a tile that does not cover the shape resolves to the heuristic's pick: timing it would enter the heuristic into
            # the table under a foreign id whenever it wins by noise
            self.covers[ck] = (not self.current) or conv2d_tile(d)[0] == (self.current & 0xff)
        if d.stats:
            # the number of batch-norm partial-sum rows depends on the tile: the finalize that follows must sum
            # exactly the rows THIS candidate writes, or the tuning passes run on garbage statistics
            self.stats_rows[d.stats] = conv2d_stats_rows(d)
        # a candidate tile may have no in-launch batch-norm epilogue, or a grid that is not resident at once: the tuning
        # passes run every conv without it (the caller issues the separate batch-norm launches while a tuner is active)
        keep_flags = d.flags
        d.flags &= ~(CONV_BN_FUSED | CONV_BN_BWD_FUSED)
        s = torch.cuda.Event(enable_timing=True)
        e = torch.cuda.Event(enable_timing=True)
        s.record()
        rc = load().disyolo_conv2d_fwd(C.byref(d), _stream())
        e.record()
        d.tile = keep
        d.flags = keep_flags
        _check(rc, "conv2d_fwd")
        if self.covers[ck]:
            self.events.setdefault(ck, []).append((s, e))

    def table(self):
        """{key: {cand: median ms}}"""
        torch.cuda.synchronize()
        out = {}
        for (key, cand), evs in self.events.items():
            ts = sorted(s.elapsed_time(e) for s, e in evs)
            out.setdefault(key, {})[cand] = ts[len(ts) // 2]
        return out

    def commit(self, min_gain: float = 0.02) -> dict:
        """pick the fastest candidate per key; keep the heuristic unless beaten by min_gain"""
        picks = {}
        for key, row in self.table().items():
            best = min(row, key=row.get)
            base = row.get(0)
            if base is not None and row[best] > base * (1.0 - min_gain):
                best = 0
            picks[key] = best
            if best:
                TUNED[key] = best
            else:
                TUNED.pop(key, None)
        return picks


TUNER: Optional[ConvTuner] = None


class KernelTimer:
    """Brackets selected launches with HIP events on the launch stream (bench.py roofline)."""

    def __init__(self):
        self.records = {}   # name -> [flops_total, [(start, end), ...]]

    def run(self, name: str, flops: float, fn, nbytes: float = 0.0) -> None:
        s = torch.cuda.Event(enable_timing=True)
        e = torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        rec = self.records.setdefault(name, [0.0, [], 0.0])
        rec[0] += flops
        rec[1].append((s, e))
        rec[2] += nbytes

    def summary(self):
        out = {}
        for name, (flops, evs, nbytes) in self.records.items():
            ms = sum(s.elapsed_time(e) for s, e in evs)
            out[name] = {"launches": len(evs), "ms_total": ms, "flops_total": flops, "bytes_total": nbytes}
        return out


TIMER: Optional[KernelTimer] = None


def conv_flops(d: ConvDesc) -> float:
    """algorithmic FLOPs of the convolution this descriptor belongs to: 2*M*Cout*K; for the
    transposed (data-gradient) gather only 1/in_div^2 of the taps are real work"""
    K = d.ksize * d.ksize * (d.C0 + d.C1)
    return 2.0 * d.B * d.Ho * d.Wo * d.Cout * K / float(d.in_div * d.in_div)


def conv_bytes(d: ConvDesc) -> float:
    """algorithmic HBM bytes of one launch: input(s) + packed weights + output (+ the residual it adds), each once"""
    K = d.ksize * d.ksize * (d.C0 + d.C1)
    out_b = d.B * d.Ho * d.Wo * d.Cout * (4 if d.flags & CONV_OUT_F32 else 2)
    return float(d.B * d.H * d.W * d.C0 * 2 + d.B * (d.H // 2) * (d.W // 2) * d.C1 * 2 + d.Cout * K * 2 + out_b
                 + (d.B * d.Ho * d.Wo * d.Cout * 2 if d.residual else 0))


_WAVES = {1: (2, 2), 2: (2, 2), 3: (2, 2), 4: (4, 1), 5: (4, 1), 6: (2, 2), 7: (4, 1), 8: (4, 2), 9: (2, 2),
          10: (2, 2), 11: (2, 2), 12: (4, 2), 13: (2, 2), 14: (2, 2), 15: (4, 2), 26: (1, 2), 27: (2, 1), 28: (1, 2), 29: (4, 2)}


def conv2d_tile(d: ConvDesc):
    """(tile id, BM, BN, BK, stages) of the conv_igemm_kernel instance the launcher will pick"""
    bm, bn, bk, st = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
    tid = load().disyolo_conv2d_tile(C.byref(d), C.byref(bm), C.byref(bn), C.byref(bk), C.byref(st))
    if tid < 0:
        raise DisyoloError("conv2d_tile: bad descriptor")
    return tid, bm.value, bn.value, bk.value, st.value


def conv2d_fwd(d: ConvDesc) -> None:
    if TUNER is not None:
        TUNER.launch(d)
        return
    if TIMER is not None:
        if not hasattr(d, "_tname"):
            tid, bm, bn, bk, st = conv2d_tile(d)
            if tid in (24, 25):
                d._tname = "conv_flat_kernel<%s,2,%d>" % ("2,3,2,1" if tid == 24 else "4,3,1,2", st)
            elif tid == 21:
                d._tname = "conv1x1_stream_kernel<%d>" % (bn // 16)
            elif tid == 20:
                d._tname = "conv_stream_kernel<8,3,4>"
            elif tid >= 16:
                d._tname = "conv_halo_kernel<%d,3,%d>" % (4 if tid == 17 else 8, 2 if tid == 18 else 1 if tid == 19 else 4)
            else:
                # (the last argument: 1 = the instance with the fused batch-norm backward epilogue, round 6)
                d._tname = "conv_igemm_kernel<%d,%d,%d,%d,%d,%d,%d,%d,%d>" % ((bm, bn) + _WAVES.get(tid, (0, 0)) +
                                                                               (bk, st, d.ksize, 2 if 13 <= tid <= 15 else 1,
                                                                                1 if d.flags & CONV_BN_BWD_FUSED else 0))
        TIMER.run(d._tname, conv_flops(d), lambda: _check(load().disyolo_conv2d_fwd(C.byref(d), _stream()),
                                                           "conv2d_fwd"), conv_bytes(d))
        return
    _check(load().disyolo_conv2d_fwd(C.byref(d), _stream()), "conv2d_fwd")


def conv2d_fp8_fwd(d: ConvDesc, w8, escale, eshift, y8, out_scale: float, y16=None, residual8=None,
                   residual_scale: float = 0.0) -> None:
    """fp8 forward conv: d.x0 = e4m3 input; outputs e4m3 (y8, of y / out_scale) and/or bf16 (y16)"""
    if TIMER is not None:
        name = "conv_fp8_kernel<%d,%d,3>" % (128 if d.Cout > 64 else (64 if d.Cout > 32 else 32), 64 if d.C0 % 64 == 0 else 32)
        TIMER.run(name, conv_flops(d), lambda: _check(load().disyolo_conv2d_fp8_fwd(
            C.byref(d), _p(w8), _p(escale), _p(eshift), _p(residual8), residual_scale, _p(y8), out_scale, _p(y16), _stream()),
            "conv2d_fp8_fwd"))
        return
    _check(load().disyolo_conv2d_fp8_fwd(C.byref(d), _p(w8), _p(escale), _p(eshift), _p(residual8), residual_scale, _p(y8),
                                         out_scale, _p(y16), _stream()), "conv2d_fp8_fwd")


def conv_first_fwd_fp8(images, w_hwio, scale, shift, y8, out_scale: float, alpha=0.1) -> None:
    _need(images, torch.float32, "images")
    _need(y8, torch.uint8, "y8")
    B, H, W, _ = images.shape
    _check(load().disyolo_conv_first_fwd_fp8(_p(images), _p(w_hwio), _p(scale), _p(shift), _p(y8), out_scale, B, H, W,
                                             y8.shape[-1], alpha, _stream()), "conv_first_fwd_fp8")


def quant_fp8(x, y8, scale: float) -> None:
    """y8 (uint8 holding OCP e4m3) = e4m3(x / scale); x bf16 or f32"""
    if x.dtype not in (torch.bfloat16, torch.float32) or not x.is_contiguous():
        raise DisyoloError("quant_fp8: x must be contiguous bf16 or f32")
    _check(load().disyolo_quant_fp8(_p(x), int(x.dtype == torch.float32), _p(y8), x.numel(), scale, _stream()), "quant_fp8")


def dequant_fp8(x8, y, scale: float) -> None:
    _need(y, torch.float32, "y")
    _check(load().disyolo_dequant_fp8(_p(x8), _p(y), x8.numel(), scale, _stream()), "dequant_fp8")


def pack_weights_fp8(w_hwio, w8, ksize, cin, cout, scale: float) -> None:
    _check(load().disyolo_pack_weights_fp8(_p(w_hwio), _p(w8), ksize, cin, cout, scale, _stream()), "pack_weights_fp8")


def conv12_fused_ok(B: int, H: int, W: int) -> bool:
    return load().disyolo_conv12_fused_ok(B, H, W) == 1


def conv12_fused_fwd(images, w1_hwio, scale1, shift1, w2_packed, scale2, shift2, y, alpha=0.1) -> None:
    """conv1 + conv2 (both in inference mode) in one launch; conv1's output is not materialised"""
    _need(images, torch.float32, "images")
    _need(y, torch.bfloat16, "y")
    B, H, W, _ = images.shape
    _need_shape(y, (B, H // 2, W // 2, 64), "conv12_fused_fwd: y")
    fn = lambda: _check(load().disyolo_conv12_fused_fwd(_p(images), _p(w1_hwio), _p(scale1), _p(shift1), _p(w2_packed), _p(scale2),
                                                        _p(shift2), _p(y), B, H, W, alpha, _stream()), "conv12_fused_fwd")
    if TIMER is not None:
        flops = 2.0 * B * H * W * 32 * 27 + 2.0 * B * (H // 2) * (W // 2) * 64 * 288
        TIMER.run("conv12_fused_kernel", flops, fn, float(B * H * W * 12 + B * (H // 2) * (W // 2) * 128))
        return
    fn()


def block32_fused_ok(B: int, H: int, W: int, C0: int, C1: int, post: int) -> bool:
    return load().disyolo_block32_fused_ok(B, H, W, C0, C1, post) == 1


def block32_fused_fwd(x0, x1, wA, scaleA, shiftA, wB, scaleB, shiftB, y, post=0, wC=None, biasC=None, alpha=0.1) -> None:
    """[1x1 (C0 + up2(C1)) -> 32] -> [3x3 32 -> 64] with folded batch norms in one launch; post 0: + residual x0 -> bf16 y
    (the first residual block), post 1 / 2 / 3: -> [1x1 64 -> 9 / 25 / 49] + bias -> f32 y (the mask head of a k = 3 / 5 / 7
    grid, block32_post(k)).  The 32- and 64-channel intermediates are not materialised."""
    _need(x0, torch.bfloat16, "x0")
    _need(y, torch.bfloat16 if post == 0 else torch.float32, "y")
    B, H, W, C0 = x0.shape
    C1 = 0 if x1 is None else x1.shape[-1]
    # the C launcher takes B, H, W from x0 and cannot see the other buffers' sizes
    if x1 is not None:
        _need(x1, torch.bfloat16, "x1")
        _need_shape(x1, (B, H // 2, W // 2, C1), "block32_fused_fwd: x1")
    _need_shape(y, (B, H, W, {0: 64, 1: 9, 2: 25, 3: 49}[post]), "block32_fused_fwd: y")
    fn = lambda: _check(load().disyolo_block32_fused_fwd(_p(x0), _p(x1), C0, C1, _p(wA), _p(scaleA), _p(shiftA), _p(wB), _p(scaleB),
                                                         _p(shiftB), post, _p(wC), _p(biasC), _p(y), B, H, W, alpha, _stream()),
                        "block32_fused_fwd")
    if TIMER is not None:
        M = B * H * W
        flops = 2.0 * M * (32 * (C0 + C1) + 64 * 288 + (64 * 9 if post else 0))
        nbytes = M * C0 * 2 + (M // 4) * C1 * 2 + (M * 36 if post else M * 128)
        TIMER.run("block32_kernel<%d,%d>" % (C0 + C1, post), flops, fn, float(nbytes))
        return
    fn()


def dgrad_s2_quad_ok(B: int, Hdy: int, Wdy: int, Cdy: int, C: int) -> bool:
    return load().disyolo_dgrad_s2_quad_ok(B, Hdy, Wdy, Cdy, C) == 1


def pack_quad(w_hwio, wq) -> None:
    """f32 HWIO master [3,3,C,Cdy] of a stride-2 conv -> the bf16 operand [4C, 9*Cdy] of dgrad_s2_quad"""
    _need(w_hwio, torch.float32, "w")
    _need(wq, torch.bfloat16, "wq")
    C_, Cdy = w_hwio.shape[2], w_hwio.shape[3]
    _check(load().disyolo_pack_quad(_p(w_hwio), _p(wq), C_, Cdy, _stream()), "pack_quad")


def dgrad_s2_quad(dy, wq, dx, accumulate: bool = False) -> None:
    """data gradient of a 3x3 stride-2 conv (even input size, C <= 64): dx [B,2H,2W,C] (+)= quad conv of dy [B,H,W,Cdy]"""
    _need(dy, torch.bfloat16, "dy")
    _need(dx, torch.bfloat16, "dx")
    B, H, W, Cdy = dy.shape
    C_ = dx.shape[-1]
    fn = lambda: _check(load().disyolo_dgrad_s2_quad(_p(dy), _p(wq), _p(dx), _p(dx) if accumulate else None, B, H, W, Cdy, C_,
                                                      _stream()), "dgrad_s2_quad")
    if TIMER is not None:
        TIMER.run("conv_igemm_kernel<192,128,4,2,64,2,3,1>", 2.0 * B * H * W * 4 * C_ * 4 * Cdy, fn,
                  float(B * H * W * (Cdy + 4 * C_) * 2))
        return
    fn()


def block64_fused_ok(B: int, H: int, W: int, C0: int) -> bool:
    return load().disyolo_block64_fused_ok(B, H, W, C0) == 1


def block64_fused_fwd(x, wA, scaleA, shiftA, wB, scaleB, shiftB, y, alpha=0.1) -> None:
    """a residual block of the 144^2 maps, [1x1 128 -> 64] -> [3x3 64 -> 128] + x with folded batch norms, in one launch"""
    _need(x, torch.bfloat16, "x")
    _need(y, torch.bfloat16, "y")
    B, H, W, C0 = x.shape
    _need_shape(y, (B, H, W, C0), "block64_fused_fwd: y")
    fn = lambda: _check(load().disyolo_block64_fused_fwd(_p(x), _p(wA), _p(scaleA), _p(shiftA), _p(wB), _p(scaleB), _p(shiftB), _p(y),
                                                         B, H, W, C0, alpha, _stream()), "block64_fused_fwd")
    if TIMER is not None:
        M = B * H * W
        TIMER.run("block64_kernel", 2.0 * M * (64 * 128 + 128 * 576), fn, float(M * 512))
        return
    fn()


def conv_first_fwd(images, w_hwio, scale, shift, y, alpha=0.1) -> None:
    _need(images, torch.float32, "images")
    _need(y, torch.bfloat16, "y")
    B, H, W, _ = images.shape
    _check(load().disyolo_conv_first_fwd(_p(images), _p(w_hwio), _p(scale), _p(shift), _p(y), B, H, W, y.shape[-1],
                                         alpha, _stream()), "conv_first_fwd")


WGRAD_IM2COL, WGRAD_PARTIAL_ONLY, WGRAD_REDUCE_ONLY = 1, 2, 4


def wgrad_stages(n: int) -> int:
    """opts bits for the im2col weight-gradient kernel's pipeline depth (2..4 stages)"""
    if not 2 <= int(n) <= 4:
        raise DisyoloError("wgrad_stages: 2..4 pipeline stages (got %r)" % (n,))
    return (int(n) - 1) << 4


def conv2d_wgrad_workspace(d: ConvDesc, opts: int = 0) -> int:
    return load().disyolo_conv2d_wgrad_workspace(C.byref(d), opts)


def conv2d_wgrad(d: ConvDesc, dy, dy_ld: int, dw, ws: Workspace, opts: int = 0) -> None:
    """dw = weight gradient of the conv ``d`` describes.  ``d.tile`` is not read (it belongs to conv2d_fwd);
    ``opts`` = WGRAD_* tuning / timing switches, 0 in the product path."""
    need = conv2d_wgrad_workspace(d, opts)
    buf = ws.get(need)

    def call(o):
        _check(load().disyolo_conv2d_wgrad(C.byref(d), _p(dy), dy_ld, _p(dw), _p(buf), buf.numel(), o, _stream()),
               "conv2d_wgrad")
    if TIMER is not None and not (opts & (WGRAD_PARTIAL_ONLY | WGRAD_REDUCE_ONLY)):
        # the partial-sum kernel and the slab reduction as two timed launches (same work, same order)
        kind, tn, ring, splits = conv2d_wgrad_plan(d, opts)
        name = ("conv_wgrad3x3_kernel<%d,%d,3,4,0>" % (tn, ring)) if kind == 1 else ("conv_wgrad_kernel<%d,3>" % tn)
        if kind == 1 and d.stride == 2:
            name = "conv_wgrad3x3_kernel<64,8,3,4,1>"
        TIMER.run(name, conv_flops(d), lambda: call(opts | WGRAD_PARTIAL_ONLY))
        if splits > 1:
            TIMER.run("slab_reduce_kernel", 0.0, lambda: call(opts | WGRAD_REDUCE_ONLY))
        return
    call(opts)


def conv2d_wgrad_plan(d: ConvDesc, opts: int = 0):
    """(kind, channel tile, ring slots, pixel splits) of the weight-gradient launch for this descriptor"""
    v = [C.c_int(0) for _ in range(4)]
    _check(load().disyolo_conv2d_wgrad_plan(C.byref(d), opts, *[C.byref(x) for x in v]), "conv2d_wgrad_plan")
    return tuple(x.value for x in v)


def conv_first_wgrad(images, dy, dw, ws: Workspace) -> None:
    B, H, W, _ = images.shape
    cout = dy.shape[-1]
    need = load().disyolo_conv_first_wgrad_workspace(B, H, W, cout)
    buf = ws.get(need)
    _check(load().disyolo_conv_first_wgrad(_p(images), _p(dy), _p(dw), B, H, W, cout, _p(buf), buf.numel(), _stream()),
           "conv_first_wgrad")


def copy2d_f32(src, dst, rows, cols, src_ld, dst_ld) -> None:
    _check(load().disyolo_copy2d_f32(_p(src), _p(dst), rows, cols, src_ld, dst_ld, _stream()), "copy2d_f32")


def pack_weights(w_hwio, w_fwd, w_dgrad, ksize, cin, cout, cout_pad=0) -> None:
    _check(load().disyolo_pack_weights(_p(w_hwio), _p(w_fwd), _p(w_dgrad), ksize, cin, cout, max(cout_pad, cout),
                                       _stream()), "pack_weights")


class PackJob(C.Structure):
    """mirror of ``disyolo_pack_job``"""
    _fields_ = [("w_hwio", C.c_void_p), ("w_fwd", C.c_void_p), ("w_dgrad", C.c_void_p),
                ("ksize", C.c_int32), ("Cin", C.c_int32), ("Cout", C.c_int32), ("cout_pad", C.c_int32)]


class PackTable:
    """Device-resident job table for pack_all: every trainable layer re-packed by one launch."""

    def __init__(self, jobs, device):
        n = len(jobs)
        arr = (PackJob * n)()
        for i, (w, wf, wd, k, cin, cout, pad) in enumerate(jobs):
            arr[i] = PackJob(_p(w), _p(wf), _p(wd), k, cin, cout, pad)
        nbytes = load().disyolo_pack_table_bytes(n)
        host = (C.c_char * nbytes)()
        blocks = C.c_int(0)
        _check(load().disyolo_pack_table_build(arr, n, host, C.byref(blocks)), "pack_table_build")
        self.n, self.blocks = n, blocks.value
        self.dev = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(device)
        self.keep = jobs

    def run(self) -> None:
        _check(load().disyolo_pack_all(_p(self.dev), self.n, self.blocks, _stream()), "pack_all")


def bn_finalize(stats, rows, C_, count, gamma, beta, mm, mv, decay, eps, scale, shift, mean, rstd) -> None:
    _check(load().disyolo_bn_finalize(_p(stats), rows, C_, count, _p(gamma), _p(beta), _p(mm), _p(mv), decay, eps,
                                      _p(scale), _p(shift), _p(mean), _p(rstd), _stream()), "bn_finalize")


def colstats_rows(rows, C_) -> int:
    r = load().disyolo_colstats_rows(rows, C_)
    if r < 0:
        raise DisyoloError("colstats_rows: bad shape")
    return r


def colstats(x, stats, rows, C_) -> None:
    _check(load().disyolo_colstats(_p(x), _p(stats), rows, C_, _stream()), "colstats")


def bn_act_bwd_partials(dy, x, scale, shift, mean, rstd, dx, dgamma, dbeta, rows, C_, partials, part_rows,
                        ws: Workspace, alpha=0.1, shortcut_grad=None, shortcut_accumulate=False) -> None:
    """bn_act_bwd whose column reduction was done by the conv that produced dy (make_conv_desc(bn_bwd=...))"""
    _need(partials, torch.float32, "partials")
    if partials.numel() < part_rows * C_ * 2:
        raise DisyoloError("bn_act_bwd_partials: partials smaller than part_rows x C x 2")
    buf = ws.get(load().disyolo_bn_act_bwd_partials_workspace(C_))
    _check(load().disyolo_bn_act_bwd_partials(_p(dy), _p(x), _p(scale), _p(shift), _p(mean), _p(rstd), _p(dx), _p(dgamma),
                                              _p(dbeta), rows, C_, alpha, _p(partials), part_rows, _p(shortcut_grad),
                                              int(shortcut_accumulate), _p(buf), buf.numel(), _stream()), "bn_act_bwd_partials")


def bn_partial_sums(partials, rows, C_, sums) -> None:
    """SyncBN: conv-epilogue partial rows -> this rank's f64 sums [C,2]"""
    _need(sums, torch.float64, "sums")
    _check(load().disyolo_bn_partial_sums(_p(partials), rows, C_, _p(sums), _stream()), "bn_partial_sums")


def bn_finalize_sums(sums, C_, count, gamma, beta, mm, mv, decay, eps, scale, shift, mean, rstd) -> None:
    _need(sums, torch.float64, "sums")
    _check(load().disyolo_bn_finalize_sums(_p(sums), C_, count, _p(gamma), _p(beta), _p(mm), _p(mv), decay, eps, _p(scale),
                                           _p(shift), _p(mean), _p(rstd), _stream()), "bn_finalize_sums")


def bn_bwd_reduce(dy, x, scale, shift, mean, rstd, rows, C_, sums, ws: Workspace, alpha=0.1) -> None:
    _need(sums, torch.float64, "sums")
    buf = ws.get(load().disyolo_bn_bwd_reduce_rows(rows, C_) * C_ * 2 * 4)
    _check(load().disyolo_bn_bwd_reduce(_p(dy), _p(x), _p(scale), _p(shift), _p(mean), _p(rstd), rows, C_, alpha, _p(sums),
                                        _p(buf), buf.numel(), _stream()), "bn_bwd_reduce")


def bn_bwd_apply_sums(dy, x, scale, shift, mean, rstd, local_sums, global_sums, count, dx, dgamma, dbeta, rows, C_,
                      ws: Workspace, alpha=0.1, shortcut_grad=None, shortcut_accumulate=False) -> None:
    buf = ws.get(2 * C_ * 4)
    _check(load().disyolo_bn_bwd_apply_sums(_p(dy), _p(x), _p(scale), _p(shift), _p(mean), _p(rstd), _p(local_sums),
                                            _p(global_sums), count, _p(dx), _p(dgamma), _p(dbeta), rows, C_, alpha,
                                            _p(shortcut_grad), int(shortcut_accumulate), _p(buf), buf.numel(), _stream()),
           "bn_bwd_apply_sums")


def bn_fold(gamma, beta, mm, mv, eps, scale, shift) -> None:
    _check(load().disyolo_bn_fold(_p(gamma), _p(beta), _p(mm), _p(mv), eps, _p(scale), _p(shift), gamma.numel(),
                                  _stream()), "bn_fold")


def bn_act_fwd(x, scale, shift, residual, y, rows, C_, alpha=0.1) -> None:
    _check(load().disyolo_bn_act_fwd(_p(x), _p(scale), _p(shift), _p(residual), _p(y), rows, C_, alpha, _stream()),
           "bn_act_fwd")


def bn_act_bwd(dy, x, scale, shift, mean, rstd, dx, dgamma, dbeta, rows, C_, ws: Workspace, alpha=0.1,
               shortcut_grad=None, shortcut_accumulate=False) -> None:
    """``shortcut_grad``: the residual shortcut's gradient buffer receives dy (or dy + itself) in the same pass"""
    need = load().disyolo_bn_act_bwd_workspace(rows, C_)
    buf = ws.get(need)
    _check(load().disyolo_bn_act_bwd(_p(dy), _p(x), _p(scale), _p(shift), _p(mean), _p(rstd), _p(dx), _p(dgamma),
                                     _p(dbeta), rows, C_, alpha, _p(shortcut_grad), int(shortcut_accumulate), _p(buf),
                                     buf.numel(), _stream()), "bn_act_bwd")


def bn_frozen_bwd(dy, x, scale, shift, dx, rows, C_, alpha=0.1, shortcut_grad=None, shortcut_accumulate=False) -> None:
    """backward of a locked layer's leaky(x*scale + shift) with the folded moving statistics: dx = scale * dy * leaky'(z);
    ``dx`` may be ``dy``; ``shortcut_grad`` as in bn_act_bwd"""
    _check(load().disyolo_bn_frozen_bwd(_p(dy), _p(x), _p(scale), _p(shift), _p(dx), rows, C_, alpha, _p(shortcut_grad),
                                        int(shortcut_accumulate), _stream()), "bn_frozen_bwd")


def mask_paste(masks, rects, classids, image_h: int, image_w: int, full_masks, merged) -> None:
    """masks f32 [n,Hm,Wm]; rects int32 [n,8]; classids int32 [n]; full_masks uint8 [n,H,W] or None; merged uint8 [H,W]"""
    n = int(rects.shape[0])
    if n:
        _need(masks, torch.float32, "masks")
        _need(rects, torch.int32, "rects")
        _need(classids, torch.int32, "classids")
    mh, mw = (int(masks.shape[-2]), int(masks.shape[-1])) if n else (1, 1)
    _check(load().disyolo_mask_paste_hw(_p(masks) if n else None, n, mh, mw, _p(rects) if n else None,
                                        _p(classids) if n else None, image_h, image_w, _p(full_masks), _p(merged), _stream()),
           "mask_paste")


PASTE_JOB = np.dtype([("masks", np.uint64), ("rects", np.uint64), ("classids", np.uint64), ("gt", np.uint64), ("gt_class", np.uint64),
                      ("merged", np.uint64), ("true_map", np.uint64), ("counts", np.uint64), ("n", np.int32), ("ng", np.int32),
                      ("image_h", np.int32), ("image_w", np.int32), ("block0", np.int32), ("reserved", np.int32)])
assert PASTE_JOB.itemsize == 88      # (disyolo_paste_job, include/disyolo.h)


def paste_job_plan(jobs, wide: bool = False) -> int:
    """jobs: numpy array of PASTE_JOB records (host); checks them and fills ``block0``; returns the launch's block count.
    ``wide``: jobs of up to 256 detections (disyolo_paste_job_plan_x) instead of 64"""
    if jobs.dtype != PASTE_JOB or not jobs.flags["C_CONTIGUOUS"] or jobs.ndim != 1:
        raise DisyoloError("paste_job_plan: jobs must be a contiguous 1-d array of PASTE_JOB records")
    plan = load().disyolo_paste_job_plan_x if wide else load().disyolo_paste_job_plan
    rc = plan(jobs.ctypes.data, int(jobs.shape[0]))
    if rc < 0:
        _check(rc, "paste_job_plan")
    return rc


def mask_paste_iou_batch(jobs, jobs_dev, size, conf=None, wide: bool = False) -> None:
    """jobs: the planned PASTE_JOB records on the host; jobs_dev: a uint8 CUDA tensor that starts with the same bytes (uploaded by
    the caller on this stream); size: the masks' size, an int or (Hm, Wm); conf: int64 [16] CUDA or None.  One launch for all
    jobs (disyolo_mask_paste_iou_batch_hw; ``wide``: disyolo_mask_paste_iou_batch_x, jobs of up to 256 detections)."""
    if jobs.dtype != PASTE_JOB or not jobs.flags["C_CONTIGUOUS"] or jobs.ndim != 1:
        raise DisyoloError("mask_paste_iou_batch: jobs must be a contiguous 1-d array of PASTE_JOB records")
    _need(jobs_dev, torch.uint8, "jobs_dev")
    if jobs_dev.numel() < jobs.nbytes:
        raise DisyoloError("mask_paste_iou_batch: %d jobs do not fit %d bytes" % (jobs.shape[0], jobs_dev.numel()))
    if conf is not None:
        _need(conf, torch.int64, "conf")
        _need_shape(conf, (16,), "conf")
    mh, mw = hw_of(size)
    launch = load().disyolo_mask_paste_iou_batch_x if wide else load().disyolo_mask_paste_iou_batch_hw
    _check(launch(jobs.ctypes.data, _p(jobs_dev), int(jobs.shape[0]), mh, mw, _p(conf), _stream()), "mask_paste_iou_batch")


def letterbox(rgb_u8, out, size):
    """rgb_u8 uint8 CUDA [H,W,3] -> out f32 CUDA [net_h,net_w,3] (``size``: an int, or (net_h, net_w)); returns the clip
    window (numpy f32 [4])"""
    import numpy as np
    _need(rgb_u8, torch.uint8, "rgb")
    _need(out, torch.float32, "out")
    nh, nw = hw_of(size)
    if rgb_u8.dim() != 3 or rgb_u8.shape[2] != 3 or tuple(out.shape) != (nh, nw, 3):
        raise DisyoloError("letterbox: rgb must be [H,W,3] uint8 and out [size,size,3] f32 ([net_h,net_w,3] for a pair)")
    win = (C.c_float * 4)()
    _check(load().disyolo_letterbox_hw(_p(rgb_u8), int(rgb_u8.shape[0]), int(rgb_u8.shape[1]), _p(out), nh, nw, win,
                                       _stream()), "letterbox")
    return np.array(list(win), np.float32)


def _table(host, cols: int, name: str, dev, device):
    """a host int32 table the library checks before it launches, and its device copy (uploaded here when not given)"""
    host = np.ascontiguousarray(host, dtype=np.int32)
    if host.ndim != (1 if cols == 1 else 2) or (cols > 1 and host.shape[1] != cols):
        raise DisyoloError("%s must be an int32 table with %d column(s) (got shape %s)" % (name, cols, host.shape))
    if dev is None:
        dev = torch.from_numpy(host).to(device)
    _need(dev, torch.int32, name)
    _need_shape(dev, host.shape, name)
    return host, dev


def tile_gather(rgb_u8, origins_dev, t0: int, t1: int, out, size) -> None:
    """rgb_u8 uint8 CUDA [h,w,3]; origins_dev int32 CUDA [T,2]; out f32 CUDA [t1-t0,net_h,net_w,3]: tiles t0 .. t1-1 (an index
    >= T is a pad tile) in one launch (disyolo_tile_gather)"""
    _need(rgb_u8, torch.uint8, "rgb")
    _need(origins_dev, torch.int32, "origins")
    _need(out, torch.float32, "out")
    nh, nw = hw_of(size)
    if rgb_u8.dim() != 3 or rgb_u8.shape[2] != 3 or origins_dev.dim() != 2 or origins_dev.shape[1] != 2:
        raise DisyoloError("tile_gather: rgb must be [h,w,3] uint8 and origins [T,2] int32")
    _need_shape(out, (int(t1) - int(t0), nh, nw, 3), "out")
    _check(load().disyolo_tile_gather(_p(rgb_u8), int(rgb_u8.shape[0]), int(rgb_u8.shape[1]), _p(origins_dev),
                                      int(origins_dev.shape[0]), int(t0), int(t1), _p(out), nh, nw, _stream()), "tile_gather")


def tile_paste_bits(masks, rects, size, planes) -> None:
    """masks f32 CUDA [n,Hm,Wm]; rects int32 CUDA [n,8]; planes uint32 bits as int32 CUDA [n,net_h,net_w/32]
    (disyolo_tile_paste_bits); n = 0 launches nothing"""
    nh, nw = hw_of(size)
    n = int(rects.shape[0])
    mh, mw = 1, 1
    if n:
        _need(masks, torch.float32, "masks")
        _need(rects, torch.int32, "rects")
        _need(planes, torch.int32, "planes")
        if masks.dim() != 3 or int(masks.shape[0]) != n:
            raise DisyoloError("tile_paste_bits: masks must be [n,Hm,Wm] with one mask per rect")
        _need_shape(rects, (n, 8), "rects")
        _need_shape(planes, (n, nh, max(nw // 32, 0)), "planes")
        mh, mw = int(masks.shape[1]), int(masks.shape[2])
    _check(load().disyolo_tile_paste_bits(_p(masks) if n else None, n, mh, mw, _p(rects) if n else None, nh, nw,
                                          _p(planes) if n else None, _stream()), "tile_paste_bits")


def tile_seam_counts(pairs, inst_tile, origins, image_hw, planes, size, inst_tile_dev=None, origins_dev=None):
    """pairs [P,2], inst_tile [N], origins [T,2]: host int32 tables (checked before the launch; the device copies of the last
    two may be passed in); planes int32 CUDA [N,net_h,net_w/32] -> counts int32 CUDA [P,3] = |A n R|, |B n R|, |A n B|
    (disyolo_tile_seam_counts)"""
    nh, nw = hw_of(size)
    dev = planes.device
    pairs, pairs_d = _table(np.asarray(pairs, np.int32).reshape(-1, 2), 2, "pairs", None, dev)
    inst_tile, inst_tile_dev = _table(inst_tile, 1, "inst_tile", inst_tile_dev, dev)
    origins, origins_dev = _table(origins, 2, "origins", origins_dev, dev)
    P, N = int(pairs.shape[0]), int(inst_tile.shape[0])
    if P:
        _need(planes, torch.int32, "planes")
        _need_shape(planes, (N, nh, max(nw // 32, 0)), "planes")
    counts = torch.zeros(P, 3, dtype=torch.int32, device=dev)
    _check(load().disyolo_tile_seam_counts(pairs.ctypes.data, _p(pairs_d), P, inst_tile.ctypes.data, _p(inst_tile_dev), N,
                                           origins.ctypes.data, _p(origins_dev), int(origins.shape[0]), int(image_hw[0]),
                                           int(image_hw[1]), _p(planes), nh, nw, _p(counts), _stream()), "tile_seam_counts")
    return counts


COMPOSE_CHUNK = 1024      # pixels of a group's box per block of disyolo_tile_compose (disyolo_tile_compose_blocks)


def tile_compose_plan(boxes, member_start):
    """boxes int32 [G,4] (y1,x1,y2,x2 in the image), member_start [G+1] (CSR) -> (groups int32 [G,8] = m0, m1, the box, block0,
    off16 as disyolo_tile_compose takes them, the arena's size in bytes)"""
    boxes = np.asarray(boxes, np.int64).reshape(-1, 4)
    start = np.asarray(member_start, np.int64).reshape(-1)
    G = int(boxes.shape[0])
    if start.shape[0] != G + 1:
        raise DisyoloError("tile_compose_plan: member_start must have one entry more than there are boxes")
    if load().disyolo_tile_compose_blocks(COMPOSE_CHUNK) != 1 or load().disyolo_tile_compose_blocks(COMPOSE_CHUNK + 1) != 2:
        raise DisyoloError("tile_compose_plan: the library's chunk is not %d pixels: rebuild it" % COMPOSE_CHUNK)
    area = np.maximum(boxes[:, 2] - boxes[:, 0], 0) * np.maximum(boxes[:, 3] - boxes[:, 1], 0)
    blocks = np.concatenate([[0], np.cumsum((area + COMPOSE_CHUNK - 1) // COMPOSE_CHUNK)])
    off16 = np.concatenate([[0], np.cumsum((area + 15) // 16)])
    if blocks[-1] >= 1 << 31 or off16[-1] >= 1 << 31:
        raise DisyoloError("tile_compose_plan: the groups' boxes hold too many pixels for one launch")
    groups = np.zeros((G, 8), np.int32)
    groups[:, 0], groups[:, 1], groups[:, 2:6], groups[:, 6], groups[:, 7] = start[:-1], start[1:], boxes, blocks[:-1], off16[:-1]
    return groups, int(off16[-1]) * 16


def tile_compose(groups, members, inst_tile, origins, planes, size, image_hw, arena, owner, inst_tile_dev=None,
                 origins_dev=None, groups_dev=None) -> None:
    """groups [G,8] (tile_compose_plan), members [M], inst_tile [N], origins [T,2]: host int32 tables (checked before the
    launch; device copies may be passed in); planes int32 CUDA [N,net_h,net_w/32]; arena uint8 CUDA; owner int32 CUDA [h,w]
    (disyolo_tile_compose)"""
    nh, nw = hw_of(size)
    dev = owner.device
    groups, groups_d = _table(np.asarray(groups, np.int32).reshape(-1, 8), 8, "groups", groups_dev, dev)
    members, members_d = _table(members, 1, "members", None, dev)
    inst_tile, inst_tile_dev = _table(inst_tile, 1, "inst_tile", inst_tile_dev, dev)
    origins, origins_dev = _table(origins, 2, "origins", origins_dev, dev)
    G, N = int(groups.shape[0]), int(inst_tile.shape[0])
    _need(owner, torch.int32, "owner")
    _need_shape(owner, (int(image_hw[0]), int(image_hw[1])), "owner")
    if G:
        _need(arena, torch.uint8, "arena")
        _need(planes, torch.int32, "planes")
        _need_shape(planes, (N, nh, max(nw // 32, 0)), "planes")
    _check(load().disyolo_tile_compose(groups.ctypes.data, _p(groups_d), G, members.ctypes.data, _p(members_d),
                                       int(members.shape[0]), inst_tile.ctypes.data, _p(inst_tile_dev), N, origins.ctypes.data,
                                       _p(origins_dev), int(origins.shape[0]), _p(planes) if G else None, nh, nw,
                                       int(image_hw[0]), int(image_hw[1]), _p(arena) if G else None,
                                       int(arena.numel()) if G else 0, _p(owner), _stream()), "tile_compose")


GROUP_COUNTS_CHUNK = 2048      # pixels of a pair's rectangle per block of disyolo_tile_group_counts (..._group_counts_blocks)
GROUP_COUNTS_MAX_BLOCKS = 1024  # ... and the most blocks one pair gets: they stride over the chunks of a larger rectangle


def tile_group_counts_plan(groups, gt, pairs2):
    """groups int32 [G,8] (tile_compose_plan), gt int32 [ng,8] = y1, x1, y2, x2, classid, pitch, off, area, pairs2 int [P,2] =
    (g, j) with j = -1 for the group's own pixel count -> (pairs int32 [P,3] = g, j, block0 as disyolo_tile_group_counts takes
    them, the launch's block count).  A pair's rectangle is the group's box, cut to the instance's box for j >= 0; an empty one
    takes one block."""
    groups = np.asarray(groups, np.int64).reshape(-1, 8)
    gt = np.asarray(gt, np.int64).reshape(-1, 8)
    p2 = np.asarray(pairs2, np.int64).reshape(-1, 2)
    P = int(p2.shape[0])
    lib = load()
    if ([lib.disyolo_tile_group_counts_blocks(a) for a in (GROUP_COUNTS_CHUNK, GROUP_COUNTS_CHUNK + 1, 1 << 40)]
            != [1, 2, GROUP_COUNTS_MAX_BLOCKS]):
        raise DisyoloError("tile_group_counts_plan: the library's chunk is not %d pixels in at most %d blocks: rebuild it" %
                           (GROUP_COUNTS_CHUNK, GROUP_COUNTS_MAX_BLOCKS))
    pairs = np.zeros((P, 3), np.int32)
    if P == 0:
        return pairs, 0
    g, j = p2[:, 0], p2[:, 1]
    if g.min() < 0 or g.max() >= groups.shape[0] or j.min() < -1 or j.max() >= gt.shape[0]:
        raise DisyoloError("tile_group_counts_plan: a pair is out of range (%d groups, %d ground-truth instances)" %
                           (groups.shape[0], gt.shape[0]))
    box = groups[g, 2:6]
    if gt.shape[0]:
        other = gt[np.maximum(j, 0), :4]
        own = (j < 0)[:, None]
        box = np.where(own, box, np.concatenate([np.maximum(box[:, :2], other[:, :2]), np.minimum(box[:, 2:], other[:, 2:])], 1))
    area = np.maximum(box[:, 2] - box[:, 0], 0) * np.maximum(box[:, 3] - box[:, 1], 0)
    blocks = np.concatenate([[0], np.cumsum(np.clip((area + GROUP_COUNTS_CHUNK - 1) // GROUP_COUNTS_CHUNK, 1, GROUP_COUNTS_MAX_BLOCKS))])
    if blocks[-1] >= 1 << 31:
        raise DisyoloError("tile_group_counts_plan: the pairs' rectangles hold too many pixels for one launch")
    pairs[:, 0], pairs[:, 1], pairs[:, 2] = g, j, blocks[:-1]
    return pairs, int(blocks[-1])


def tile_group_counts(groups, arena, gt, gt_bits, pairs, image_hw, groups_dev=None, gt_dev=None, pairs_dev=None,
                      arena_bytes: Optional[int] = None):
    """groups [G,8], gt [ng,8], pairs [P,3] (tile_group_counts_plan): host int32 tables (checked before the launch; their device
    copies may be passed in); arena uint8 CUDA (what tile_compose wrote; ``arena_bytes`` of it, all by default); gt_bits uint32
    bits as int32 CUDA -> counts int32 CUDA [P] (disyolo_tile_group_counts).  P = 0 or G = 0 launches nothing."""
    dev = arena.device
    groups, groups_dev = _table(np.asarray(groups, np.int32).reshape(-1, 8), 8, "groups", groups_dev, dev)
    gt, gt_dev = _table(np.asarray(gt, np.int32).reshape(-1, 8), 8, "gt", gt_dev, dev)
    pairs, pairs_dev = _table(np.asarray(pairs, np.int32).reshape(-1, 3), 3, "pairs", pairs_dev, dev)
    G, ng, P = int(groups.shape[0]), int(gt.shape[0]), int(pairs.shape[0])
    _need(arena, torch.uint8, "arena")
    _need(gt_bits, torch.int32, "gt_bits")
    nbytes = int(arena.numel()) if arena_bytes is None else int(arena_bytes)
    if not 0 <= nbytes <= int(arena.numel()):
        raise DisyoloError("tile_group_counts: arena_bytes = %d, the arena holds %d" % (nbytes, int(arena.numel())))
    counts = torch.zeros(P, dtype=torch.int32, device=dev)
    _check(load().disyolo_tile_group_counts(groups.ctypes.data, _p(groups_dev), G, _p(arena), nbytes, gt.ctypes.data, _p(gt_dev),
                                            ng, _p(gt_bits), int(gt_bits.numel()), pairs.ctypes.data, _p(pairs_dev), P,
                                            int(image_hw[0]), int(image_hw[1]), _p(counts), _stream()), "tile_group_counts")
    return counts


def _arena_tables(groups, buf, groups_dev, arena_bytes, what: str, holder: str = "arena"):
    """the groups table (host copy checked by the library before any launch, device copy uploaded when not given) and the
    elements in use of ``buf``, as every call over the arena takes them.  ``holder`` names buf in the message: "arena", the
    uint8 masks themselves, or "buffer", any per-pixel buffer in the arena's layout"""
    if holder == "arena":
        _need(buf, torch.uint8, "arena")
    groups, groups_dev = _table(np.asarray(groups, np.int32).reshape(-1, 8), 8, "groups", groups_dev, buf.device)
    nbytes = int(buf.numel()) if arena_bytes is None else int(arena_bytes)
    if not 0 <= nbytes <= int(buf.numel()):
        raise DisyoloError("%s: arena_bytes = %d, the %s holds %d" % (what, nbytes, holder, int(buf.numel())))
    return groups, groups_dev, nbytes


def _need_elems(t: torch.Tensor, dtype, n: int, name: str) -> None:
    _need(t, dtype, name)
    if int(t.numel()) < n:
        raise DisyoloError("%s must hold at least %d elements (got %d)" % (name, n, int(t.numel())))


def measure_blocks(groups) -> int:
    """the block count of the plan in groups [G,8] (tile_compose_plan): what measure_counts' partials must hold"""
    groups = np.asarray(groups, np.int64).reshape(-1, 8)
    if groups.shape[0] == 0:
        return 0
    last = groups[-1]
    area = max(int(last[4] - last[2]), 0) * max(int(last[5] - last[3]), 0)
    return int(last[6]) + (area + COMPOSE_CHUNK - 1) // COMPOSE_CHUNK


def measure_d2(groups, arena, colg, d2, groups_dev=None, arena_bytes: Optional[int] = None) -> None:
    """groups [G,8] (tile_compose_plan; host int32, checked before the launch, its device copy may be passed in); arena uint8
    CUDA (what tile_compose wrote; ``arena_bytes`` of it, all by default); colg int16 CUDA scratch and d2 int32 CUDA out, each
    of at least arena_bytes elements in the arena's layout (disyolo_measure_d2).  Elements between crops are left untouched."""
    groups, groups_dev, nbytes = _arena_tables(groups, arena, groups_dev, arena_bytes, "measure_d2")
    _need_elems(colg, torch.int16, nbytes, "colg")
    _need_elems(d2, torch.int32, nbytes, "d2")
    _check(load().disyolo_measure_d2(groups.ctypes.data, _p(groups_dev), int(groups.shape[0]), _p(arena), nbytes, _p(colg), _p(d2),
                                     _stream()), "measure_d2")


def measure_thin(groups, arena, skel, tmp, flags, iters, it0: int, chunk: int, groups_dev=None,
                 arena_bytes: Optional[int] = None) -> None:
    """``chunk`` iterations of Zhang-Suen thinning, numbered from ``it0``, for all groups (disyolo_measure_thin): skel, tmp
    uint8 CUDA of at least arena_bytes elements, flags int32 CUDA [chunk+1,G] (a non-zero word of the last row: that group
    still changed), iters int32 CUDA [G].  No synchronisation here: the caller reads the last flags row."""
    groups, groups_dev, nbytes = _arena_tables(groups, arena, groups_dev, arena_bytes, "measure_thin")
    G = int(groups.shape[0])
    _need_elems(skel, torch.uint8, nbytes, "skel")
    _need_elems(tmp, torch.uint8, nbytes, "tmp")
    _need(flags, torch.int32, "flags")
    _need_shape(flags, (int(chunk) + 1, G), "flags")
    _need(iters, torch.int32, "iters")
    _need_shape(iters, (G,), "iters")
    _check(load().disyolo_measure_thin(groups.ctypes.data, _p(groups_dev), G, _p(arena), nbytes, _p(skel), _p(tmp), _p(flags),
                                       _p(iters), int(it0), int(chunk), _stream()), "measure_thin")


def measure_counts(groups, arena, skel, d2, groups_dev=None, arena_bytes: Optional[int] = None):
    """-> (counts int64 CUDA [G,8] = area, skel_px, n_orth, n_diag, n_end, max_d2, max_d2_skel, 0; sum_sqrt f64 CUDA [G]) of the
    masks in arena, their skeletons in skel and their squared distances in d2 (disyolo_measure_counts)"""
    groups, groups_dev, nbytes = _arena_tables(groups, arena, groups_dev, arena_bytes, "measure_counts")
    G = int(groups.shape[0])
    _need_elems(skel, torch.uint8, nbytes, "skel")
    _need_elems(d2, torch.int32, nbytes, "d2")
    dev = arena.device
    counts = torch.zeros(G, 8, dtype=torch.int64, device=dev)
    sum_sqrt = torch.zeros(G, dtype=torch.float64, device=dev)
    partials = torch.empty(max(measure_blocks(groups), 1), dtype=torch.float64, device=dev)
    _check(load().disyolo_measure_counts(groups.ctypes.data, _p(groups_dev), G, _p(arena), nbytes, _p(skel), _p(d2), _p(counts),
                                         _p(partials), int(partials.numel()), _p(sum_sqrt), _stream()), "measure_counts")
    return counts, sum_sqrt


SKELETON_ROW = 12      # int64 words of a branch row (disyolo_skeleton_rows)


def _need_rows(rows: torch.Tensor) -> None:
    _need(rows, torch.int64, "rows")
    if rows.dim() != 2 or int(rows.shape[1]) != SKELETON_ROW:
        raise DisyoloError("rows must be [capacity, %d] (got %s)" % (SKELETON_ROW, tuple(rows.shape)))


def skeleton_classify(groups, src, skel, links, groups_dev=None, arena_bytes: Optional[int] = None) -> None:
    """src uint8 CUDA (a non-zero byte is a skeleton pixel) -> links uint8 CUDA, the link bits of every pixel; skel uint8 CUDA
    gets the 0 / 1 state of src unless it IS src (disyolo_skeleton_classify).  All in the arena's layout."""
    groups, groups_dev, nbytes = _arena_tables(groups, src, groups_dev, arena_bytes, "skeleton_classify", "buffer")
    _need(src, torch.uint8, "src")
    _need_elems(skel, torch.uint8, nbytes, "skel")
    _need_elems(links, torch.uint8, nbytes, "links")
    _check(load().disyolo_skeleton_classify(groups.ctypes.data, _p(groups_dev), int(groups.shape[0]), nbytes, _p(src), _p(skel),
                                            _p(links), _stream()), "skeleton_classify")


def skeleton_label(groups, skel, links, labels, groups_dev=None, arena_bytes: Optional[int] = None) -> None:
    """labels int32 CUDA: the branch label (its smallest pixel index) on pixels of degree <= 2, -1 on the crop's other pixels
    (disyolo_skeleton_label: init, merge, flatten)"""
    groups, groups_dev, nbytes = _arena_tables(groups, skel, groups_dev, arena_bytes, "skeleton_label", "buffer")
    _need(skel, torch.uint8, "skel")
    _need_elems(links, torch.uint8, nbytes, "links")
    _need_elems(labels, torch.int32, nbytes, "labels")
    _check(load().disyolo_skeleton_label(groups.ctypes.data, _p(groups_dev), int(groups.shape[0]), nbytes, _p(skel), _p(links),
                                         _p(labels), _stream()), "skeleton_label")


def skeleton_rows(groups, links, labels, d2, rowid, rows, M2: int, ctrl, junctions, groups_dev=None,
                  arena_bytes: Optional[int] = None) -> None:
    """the branch rows int64 CUDA [capacity, SKELETON_ROW] in any order, ctrl int32 CUDA [1 + G] (the branch count, which may
    exceed the capacity, and one spur flag per group) and junctions int64 CUDA [G,4] (disyolo_skeleton_rows); rowid int32 CUDA
    per pixel is scratch.  No synchronisation here: the caller reads ctrl."""
    groups, groups_dev, nbytes = _arena_tables(groups, links, groups_dev, arena_bytes, "skeleton_rows", "buffer")
    G = int(groups.shape[0])
    _need(links, torch.uint8, "links")
    _need_elems(labels, torch.int32, nbytes, "labels")
    _need_elems(d2, torch.int32, nbytes, "d2")
    _need_elems(rowid, torch.int32, nbytes, "rowid")
    _need_rows(rows)
    _need_elems(ctrl, torch.int32, G + 1, "ctrl")
    _need(junctions, torch.int64, "junctions")
    _need_shape(junctions, (G, 4), "junctions")
    _check(load().disyolo_skeleton_rows(groups.ctypes.data, _p(groups_dev), G, nbytes, _p(links), _p(labels), _p(d2), _p(rowid),
                                        _p(rows), int(rows.shape[0]), int(M2), _p(ctrl), _p(junctions), _stream()),
           "skeleton_rows")


def skeleton_prune(groups, labels, rowid, rows, skel, groups_dev=None, arena_bytes: Optional[int] = None) -> None:
    """zeroes the bytes of skel whose branch is a spur by its row (disyolo_skeleton_prune)"""
    groups, groups_dev, nbytes = _arena_tables(groups, skel, groups_dev, arena_bytes, "skeleton_prune", "buffer")
    _need(skel, torch.uint8, "skel")
    _need_elems(labels, torch.int32, nbytes, "labels")
    _need_elems(rowid, torch.int32, nbytes, "rowid")
    _need_rows(rows)
    _check(load().disyolo_skeleton_prune(groups.ctypes.data, _p(groups_dev), int(groups.shape[0]), nbytes, _p(labels), _p(rowid),
                                         _p(rows), int(rows.shape[0]), _p(skel), _stream()), "skeleton_prune")


# the traced skeleton graph (csrc/trace.hip): int64 words of a node row and of an edge row, int32 words of a list entry, of a
# branch profile entry, of a trunk profile entry, of the trunk plan's row per branch and per attach pixel; int64 of a trunk row
TRACE_NODE, TRACE_EDGE, TRACE_ENT, TRACE_PROFILE, TRACE_TRUNK_PROFILE, TRACE_SEG, TRACE_ATTACH, TRACE_TRUNK = 8, 12, 12, 4, 5, 4, 6, 8


def _need_table(t: torch.Tensor, dtype, width: int, name: str) -> None:
    _need(t, dtype, name)
    if t.dim() != 2 or int(t.shape[1]) != width:
        raise DisyoloError("%s must be [n, %d] (got %s)" % (name, width, tuple(t.shape)))


def trace_nodes(groups, links, d2, node_labels, noderow, nodes, ctrl, groups_dev=None, arena_bytes: Optional[int] = None) -> None:
    """node_labels int32 CUDA: the node (its smallest pixel index) on pixels of degree >= 3, -1 on the crop's other pixels; nodes
    int64 CUDA [capacity, TRACE_NODE] in any order and ctrl int32 CUDA [1], their number (disyolo_trace_nodes); noderow int32
    CUDA per pixel is scratch.  No synchronisation here."""
    groups, groups_dev, nbytes = _arena_tables(groups, links, groups_dev, arena_bytes, "trace_nodes", "buffer")
    _need(links, torch.uint8, "links")
    _need_elems(d2, torch.int32, nbytes, "d2")
    _need_elems(node_labels, torch.int32, nbytes, "node_labels")
    _need_elems(noderow, torch.int32, nbytes, "noderow")
    _need_table(nodes, torch.int64, TRACE_NODE, "nodes")
    _need_elems(ctrl, torch.int32, 1, "ctrl")
    _check(load().disyolo_trace_nodes(groups.ctypes.data, _p(groups_dev), int(groups.shape[0]), nbytes, _p(links), _p(d2),
                                      _p(node_labels), _p(noderow), _p(nodes), int(nodes.shape[0]), _p(ctrl), _stream()), "trace_nodes")


def trace_rank(groups, links, labels, d2, rowid, rows, ents, rounds: int, nxt, val, count, rank, rank_diag, groups_dev=None,
               arena_bytes: Optional[int] = None) -> None:
    """rank, rank_diag int32 CUDA per pixel: the steps of every branch pixel from its branch's start and the diagonal ones among
    them, -1 elsewhere in the crops; ents int32 CUDA [capacity, TRACE_ENT], the list of the branch pixels in any order, and count
    int32 CUDA [1], its length (disyolo_trace_rank).  nxt int32 and val int64 CUDA [4 capacity] are the two state buffers of the
    ``rounds`` pointer-jumping rounds (2^rounds >= the longest branch's pixels - 1).  labels, rowid, rows: as skeleton_rows left
    them.  No synchronisation here."""
    groups, groups_dev, nbytes = _arena_tables(groups, links, groups_dev, arena_bytes, "trace_rank", "buffer")
    _need(links, torch.uint8, "links")
    for t, name in ((labels, "labels"), (d2, "d2"), (rowid, "rowid"), (rank, "rank"), (rank_diag, "rank_diag")):
        _need_elems(t, torch.int32, nbytes, name)
    _need_rows(rows)
    _need_table(ents, torch.int32, TRACE_ENT, "ents")
    cap = int(ents.shape[0])
    _need_elems(nxt, torch.int32, 4 * cap, "nxt")
    _need_elems(val, torch.int64, 4 * cap, "val")
    _need_elems(count, torch.int32, 1, "count")
    _check(load().disyolo_trace_rank(groups.ctypes.data, _p(groups_dev), int(groups.shape[0]), nbytes, _p(links), _p(labels), _p(d2),
                                     _p(rowid), _p(rows), int(rows.shape[0]), _p(ents), cap, int(rounds), _p(nxt), _p(val),
                                     _p(count), _p(rank), _p(rank_diag), _stream()), "trace_rank")


def trace_edges(groups, ents, count, rank, rank_diag, node_labels, edges, groups_dev=None, arena_bytes: Optional[int] = None) -> None:
    """edges int64 CUDA [rows, TRACE_EDGE]: what the two ends of every branch are, row r for the branch of row r of skeleton_rows
    (disyolo_trace_edges)"""
    groups, groups_dev, nbytes = _arena_tables(groups, rank, groups_dev, arena_bytes, "trace_edges", "buffer")
    _need_table(ents, torch.int32, TRACE_ENT, "ents")
    _need_elems(count, torch.int32, 1, "count")
    _need(rank, torch.int32, "rank")
    _need_elems(rank_diag, torch.int32, nbytes, "rank_diag")
    _need_elems(node_labels, torch.int32, nbytes, "node_labels")
    _need_table(edges, torch.int64, TRACE_EDGE, "edges")
    _check(load().disyolo_trace_edges(groups.ctypes.data, _p(groups_dev), int(groups.shape[0]), nbytes, _p(ents), _p(count),
                                      int(ents.shape[0]), _p(rank), _p(rank_diag), _p(node_labels), _p(edges), int(edges.shape[0]),
                                      _stream()), "trace_edges")


def trace_gather(groups, ents, count, rank, rank_diag, d2, offsets, profile, seg, edges, attach, tprofile, tstart, trunkrows,
                 groups_dev=None, arena_bytes: Optional[int] = None) -> None:
    """profile int32 CUDA [capacity, TRACE_PROFILE]: the ordered pixels of every branch, a branch at offsets[row] (int32 CUDA
    [rows]); tprofile int32 CUDA [n, TRACE_TRUNK_PROFILE]: the trunk profiles by the plan seg int32 CUDA [rows, TRACE_SEG] and
    attach int32 CUDA [m, TRACE_ATTACH]; trunkrows int64 CUDA [G, TRACE_TRUNK] over the entries tstart int32 CUDA [G + 1] bounds
    (disyolo_trace_gather).  No synchronisation here."""
    groups, groups_dev, nbytes = _arena_tables(groups, rank, groups_dev, arena_bytes, "trace_gather", "buffer")
    G = int(groups.shape[0])
    _need_table(ents, torch.int32, TRACE_ENT, "ents")
    _need_elems(count, torch.int32, 1, "count")
    _need(rank, torch.int32, "rank")
    _need_elems(rank_diag, torch.int32, nbytes, "rank_diag")
    _need_elems(d2, torch.int32, nbytes, "d2")
    _need_table(profile, torch.int32, TRACE_PROFILE, "profile")
    _need_shape(profile, (int(ents.shape[0]), TRACE_PROFILE), "profile")
    _need_table(seg, torch.int32, TRACE_SEG, "seg")
    n_rows = int(seg.shape[0])
    _need_elems(offsets, torch.int32, n_rows, "offsets")
    _need_table(edges, torch.int64, TRACE_EDGE, "edges")
    if int(edges.shape[0]) < n_rows:
        raise DisyoloError("edges must hold the %d rows of seg (got %d)" % (n_rows, int(edges.shape[0])))
    _need_table(attach, torch.int32, TRACE_ATTACH, "attach")
    _need_table(tprofile, torch.int32, TRACE_TRUNK_PROFILE, "tprofile")
    _need_elems(tstart, torch.int32, G + 1, "tstart")
    _need(trunkrows, torch.int64, "trunkrows")
    _need_shape(trunkrows, (G, TRACE_TRUNK), "trunkrows")
    _check(load().disyolo_trace_gather(groups.ctypes.data, _p(groups_dev), G, nbytes, _p(ents), _p(count), int(ents.shape[0]), _p(rank),
                                       _p(rank_diag), _p(d2), _p(offsets), n_rows, _p(profile), _p(seg), _p(edges), _p(attach),
                                       int(attach.shape[0]), _p(tprofile), int(tprofile.shape[0]), _p(tstart), _p(trunkrows),
                                       _stream()), "trace_gather")


SHAPE_COLS = 16        # int64 words of a row of disyolo_shape_sums


def shape_sums(groups, arena, sums, groups_dev=None, arena_bytes: Optional[int] = None) -> None:
    """sums int64 CUDA [G, SHAPE_COLS] = n, Sy, Sx, Syy, Sxx, Sxy, ymin, ymax, xmin, xmax, Q1, Q2, Q3, Q4, QD, 0 of the masks in
    arena, initialised by the call (disyolo_shape_sums).  No synchronisation here."""
    groups, groups_dev, nbytes = _arena_tables(groups, arena, groups_dev, arena_bytes, "shape_sums")
    G = int(groups.shape[0])
    _need(sums, torch.int64, "sums")
    _need_shape(sums, (G, SHAPE_COLS), "sums")
    _check(load().disyolo_shape_sums(groups.ctypes.data, _p(groups_dev), G, _p(arena), nbytes, _p(sums), _stream()), "shape_sums")


def shape_parts(groups, arena, labels, px, parts, groups_dev=None, arena_bytes: Optional[int] = None) -> None:
    """labels int32 CUDA: the part (the smallest pixel index of its 8-connected component) on foreground pixels, -1 on the
    crop's other pixels; parts int64 CUDA [G, 2] = n_parts, largest_part_px; px int32 CUDA per pixel is scratch
    (disyolo_shape_parts).  No synchronisation here."""
    groups, groups_dev, nbytes = _arena_tables(groups, arena, groups_dev, arena_bytes, "shape_parts")
    G = int(groups.shape[0])
    _need_elems(labels, torch.int32, nbytes, "labels")
    _need_elems(px, torch.int32, nbytes, "px")
    _need(parts, torch.int64, "parts")
    _need_shape(parts, (G, 2), "parts")
    _check(load().disyolo_shape_parts(groups.ctypes.data, _p(groups_dev), G, _p(arena), nbytes, _p(labels), _p(px), _p(parts),
                                      _stream()), "shape_parts")


def shape_extents(groups, arena, dirs, pminmax, groups_dev=None, dirs_dev=None, arena_bytes: Optional[int] = None) -> None:
    """pminmax int32 CUDA [G, K, 2]: the minimum and maximum of c_k x + s_k y over every mask for the directions dirs int32
    [K, 2] (host, checked before the launch; its device copy may be passed in) (disyolo_shape_extents).  No synchronisation
    here."""
    groups, groups_dev, nbytes = _arena_tables(groups, arena, groups_dev, arena_bytes, "shape_extents")
    G = int(groups.shape[0])
    dirs, dirs_dev = _table(np.asarray(dirs, np.int32).reshape(-1, 2), 2, "dirs", dirs_dev, arena.device)
    K = int(dirs.shape[0])
    _need(pminmax, torch.int32, "pminmax")
    _need_shape(pminmax, (G, K, 2), "pminmax")
    _check(load().disyolo_shape_extents(groups.ctypes.data, _p(groups_dev), G, _p(arena), nbytes, dirs.ctypes.data, _p(dirs_dev), K,
                                        _p(pminmax), _stream()), "shape_extents")


OUTLINE_ROW = 12       # int64 words of a loop's row of disyolo_outline_loops
OUTLINE_PLAN = 8       # int32 words of a loop's plan for disyolo_outline_gather
OUTLINE_WORK = 10      # int64 words of work per list entry
OUTLINE_MAX_LIST = 2 ** 30 - 1


def _outline_list(ekey, nxt, flag, aterm, work) -> int:
    """the per-entry buffers of an edge list -> its capacity"""
    _need(ekey, torch.int32, "ekey")
    cap = int(ekey.numel())
    if nxt is not None:
        _need_elems(nxt, torch.int32, cap, "nxt")
    _need_elems(flag, torch.uint8, cap, "flag")
    if aterm is not None:
        _need_elems(aterm, torch.int32, cap, "aterm")
    if work is not None:
        _need_elems(work, torch.int64, OUTLINE_WORK * cap, "work")
    return cap


def outline_edges(groups, arena, first, sides, ekey, nxt, flag, aterm, work, ctrl, groups_dev=None, arena_bytes: Optional[int] = None) -> None:
    """The boundary edges of every mask, listed: first int32 and sides uint8 CUDA in the arena's layout, ekey, nxt, aterm int32 and
    flag uint8 CUDA per list entry (the capacity is ekey's length), work int64 CUDA of OUTLINE_WORK words per entry, ctrl int32
    CUDA [4], zeroed by the call (disyolo_outline_edges).  No synchronisation here."""
    groups, groups_dev, nbytes = _arena_tables(groups, arena, groups_dev, arena_bytes, "outline_edges")
    _need_elems(first, torch.int32, nbytes, "first")
    _need_elems(sides, torch.uint8, nbytes, "sides")
    cap = _outline_list(ekey, nxt, flag, aterm, work)
    _need_elems(ctrl, torch.int32, 4, "ctrl")
    _check(load().disyolo_outline_edges(groups.ctypes.data, _p(groups_dev), int(groups.shape[0]), _p(arena), nbytes, _p(first), _p(sides),
                                        _p(ekey), _p(nxt), _p(flag), _p(aterm), cap, _p(work), int(work.numel()), _p(ctrl), _stream()),
           "outline_edges")


def outline_loops(groups, arena, part_labels, first, sides, ekey, nxt, flag, aterm, rounds: int, work, eidx, rows, ctrl, groups_dev=None,
                  arena_bytes: Optional[int] = None) -> None:
    """After ``outline_edges`` on the same buffers: rows int64 CUDA [L, OUTLINE_ROW], one per loop in the order of arrival, and
    eidx int32 CUDA [capacity, 3]; part_labels = the labels of ``shape_parts``; 2^rounds must reach the longest loop's edges
    (disyolo_outline_loops).  No synchronisation here."""
    groups, groups_dev, nbytes = _arena_tables(groups, arena, groups_dev, arena_bytes, "outline_loops")
    _need_elems(part_labels, torch.int32, nbytes, "part_labels")
    _need_elems(first, torch.int32, nbytes, "first")
    _need_elems(sides, torch.uint8, nbytes, "sides")
    cap = _outline_list(ekey, nxt, flag, aterm, work)
    _need_elems(eidx, torch.int32, 3 * cap, "eidx")
    _need_table(rows, torch.int64, OUTLINE_ROW, "rows")
    _need_elems(ctrl, torch.int32, 4, "ctrl")
    _check(load().disyolo_outline_loops(groups.ctypes.data, _p(groups_dev), int(groups.shape[0]), _p(arena), nbytes, _p(part_labels),
                                        _p(first), _p(sides), _p(ekey), _p(nxt), _p(flag), _p(aterm), cap, int(rounds), _p(work),
                                        int(work.numel()), _p(eidx), _p(rows), int(rows.shape[0]), _p(ctrl), _stream()), "outline_loops")


def outline_gather(groups, arena, ekey, flag, eidx, ctrl, plan, points, corners, groups_dev=None, arena_bytes: Optional[int] = None) -> None:
    """After ``outline_loops``: plan int32 CUDA [L, OUTLINE_PLAN] per row of its rows; points int32 CUDA [N, 2] and corners int32
    CUDA [C, 2] take the chains and rings in image (x, y) (disyolo_outline_gather).  The arena is not read.  No synchronisation
    here."""
    groups, groups_dev, nbytes = _arena_tables(groups, arena, groups_dev, arena_bytes, "outline_gather")
    cap = _outline_list(ekey, None, flag, None, None)
    _need_elems(eidx, torch.int32, 3 * cap, "eidx")
    _need_elems(ctrl, torch.int32, 4, "ctrl")
    _need_table(plan, torch.int32, OUTLINE_PLAN, "plan")
    _need_table(points, torch.int32, 2, "points")
    _need_table(corners, torch.int32, 2, "corners")
    _check(load().disyolo_outline_gather(groups.ctypes.data, _p(groups_dev), int(groups.shape[0]), nbytes, _p(ekey), _p(flag), _p(eidx),
                                         cap, _p(ctrl), _p(plan), int(plan.shape[0]), _p(points), int(points.shape[0]), _p(corners),
                                         int(corners.shape[0]), _stream()), "outline_gather")


def polygon_mask(px, py, poly_start, poly_is_out, image_h: int, image_w: int, mask) -> None:
    """px/py f32 CUDA [nv]; poly_start int32 CUDA [npoly+1]; poly_is_out int32 CUDA [npoly]; mask uint8 CUDA [H,W]"""
    _need(px, torch.float32, "px")
    _need(py, torch.float32, "py")
    _need(poly_start, torch.int32, "poly_start")
    _need(poly_is_out, torch.int32, "poly_is_out")
    _need(mask, torch.uint8, "mask")
    _check(load().disyolo_polygon_mask(_p(px), _p(py), _p(poly_start), _p(poly_is_out), int(poly_is_out.numel()), image_h,
                                       image_w, _p(mask), _stream()), "polygon_mask")


def aug_place(src, is_mask: bool, dst, size, new_w: int, new_h: int, dx: int, dy: int, flip: int) -> None:
    """``size`` (here and in the four functions below): the frame's size, an int or (net_h, net_w)"""
    _need(src, torch.uint8, "src")
    _need(dst, torch.uint8, "dst")
    nh, nw = hw_of(size)
    if tuple(dst.shape[:2]) != (nh, nw):
        raise DisyoloError("aug_place: dst must be [%d,%d(,3)] (got %s)" % (nh, nw, tuple(dst.shape)))
    _check(load().disyolo_aug_place_hw(_p(src), int(is_mask), int(src.shape[0]), int(src.shape[1]), _p(dst), nh, nw, new_w,
                                       new_h, dx, dy, flip, _stream()), "aug_place")


PLACE_JOB = np.dtype([("src", np.uint64), ("dst", np.uint64), ("is_mask", np.int32), ("image_h", np.int32), ("image_w", np.int32),
                      ("new_w", np.int32), ("new_h", np.int32), ("dx", np.int32), ("dy", np.int32), ("flip", np.int32)])
assert PLACE_JOB.itemsize == 48      # (disyolo_place_job, include/disyolo.h)


def aug_place_batch(jobs_dev, njobs: int, size) -> None:
    """jobs_dev: uint8 CUDA tensor holding njobs PLACE_JOB records (uploaded by the caller on this stream)"""
    _need(jobs_dev, torch.uint8, "jobs")
    if jobs_dev.numel() < njobs * PLACE_JOB.itemsize:
        raise DisyoloError("aug_place_batch: %d jobs do not fit %d bytes" % (njobs, jobs_dev.numel()))
    nh, nw = hw_of(size)
    _check(load().disyolo_aug_place_batch_hw(_p(jobs_dev), njobs, nh, nw, _stream()), "aug_place_batch")


WINDOW_JOB = np.dtype([("src", np.uint64), ("crop_h", np.int32), ("crop_w", np.int32), ("crop_x", np.int32), ("crop_y", np.int32),
                       ("x0", np.int32), ("y0", np.int32), ("image_h", np.int32), ("image_w", np.int32), ("b", np.int32),
                       ("cls", np.int32), ("flip", np.int32), ("reserved", np.int32)])
assert WINDOW_JOB.itemsize == 56     # (disyolo_window_job, include/disyolo.h)


def _window_jobs(jobs_dev, njobs: int, what: str) -> int:
    _need(jobs_dev, torch.uint8, "jobs")
    njobs = int(njobs)
    if njobs < 0 or jobs_dev.numel() < njobs * WINDOW_JOB.itemsize:
        raise DisyoloError("%s: %d jobs do not fit %d bytes" % (what, njobs, jobs_dev.numel()))
    return njobs


def window_visible(jobs_dev, njobs: int, size, vis) -> None:
    """jobs_dev: uint8 CUDA tensor holding njobs WINDOW_JOB records; vis int32 CUDA [>= njobs, 5] <- (count, x1, y1, x2, y2) of
    every job's visible part, in window coordinates (disyolo_window_visible)"""
    njobs = _window_jobs(jobs_dev, njobs, "window_visible")
    _need(vis, torch.int32, "vis")
    if vis.dim() != 2 or vis.shape[1] != 5 or vis.shape[0] < njobs:
        raise DisyoloError("window_visible: vis must be int32 [>= %d, 5] (got %s)" % (njobs, tuple(vis.shape)))
    nh, nw = hw_of(size)
    _check(load().disyolo_window_visible(_p(jobs_dev), njobs, nh, nw, _p(vis), _stream()), "window_visible")


def window_targets(jobs_dev, njobs: int, vis, anchors, size, min_visible: int, true_boxes, yolo3, yolo2, yolo1, rows) -> None:
    """the target arrays of a window batch from ``window_visible``'s table (disyolo_window_targets): true_boxes f32 CUDA
    [B,1,1,1,G,5] (or [B,G,5]), yolo3 / yolo2 / yolo1 f32 CUDA [B, net_h/d, net_w/d, 3, 5+C], all zeroed and filled; rows int32
    CUDA [>= njobs] <- each job's row of true_boxes, or -1; anchors f32 CUDA [9,2]"""
    njobs = _window_jobs(jobs_dev, njobs, "window_targets")
    nh, nw = hw_of(size)
    _need(vis, torch.int32, "vis")
    _need(rows, torch.int32, "rows")
    _need(anchors, torch.float32, "anchors")
    _need_shape(anchors, (9, 2), "anchors")
    for t, name in ((true_boxes, "true_boxes"), (yolo3, "yolo3"), (yolo2, "yolo2"), (yolo1, "yolo1")):
        _need(t, torch.float32, name)
    if vis.dim() != 2 or vis.shape[1] != 5 or vis.shape[0] < njobs or rows.numel() < njobs:
        raise DisyoloError("window_targets: vis must be int32 [>= %d, 5] and rows hold %d entries" % (njobs, njobs))
    if true_boxes.dim() not in (3, 6) or true_boxes.shape[-1] != 5 or true_boxes.numel() != true_boxes.shape[0] * true_boxes.shape[-2] * 5:
        raise DisyoloError("window_targets: true_boxes must be [B,1,1,1,G,5] or [B,G,5] (got %s)" % (tuple(true_boxes.shape),))
    B, G = int(true_boxes.shape[0]), int(true_boxes.shape[-2])
    if yolo3.dim() != 5:
        raise DisyoloError("window_targets: yolo3 must be [B, net_h/8, net_w/8, 3, 5+C] (got %s)" % (tuple(yolo3.shape),))
    nc = int(yolo3.shape[-1]) - 5
    for t, d, name in ((yolo3, 8, "yolo3"), (yolo2, 16, "yolo2"), (yolo1, 32, "yolo1")):
        _need_shape(t, (B, nh // d, nw // d, 3, 5 + nc), name)
    _check(load().disyolo_window_targets(_p(jobs_dev), njobs, _p(vis), _p(anchors), B, G, nc, nh, nw, int(min_visible),
                                         _p(true_boxes), _p(yolo3), _p(yolo2), _p(yolo1), _p(rows), _stream()), "window_targets")


def window_place_masks(jobs_dev, njobs: int, rows, true_masks, size) -> None:
    """true_masks uint8 CUDA [B,G,net_h,net_w] (zeroed by the caller): the visible bytes of every job with rows[job] >= 0 into
    plane [b, rows[job]], flipped (disyolo_window_place_masks)"""
    njobs = _window_jobs(jobs_dev, njobs, "window_place_masks")
    nh, nw = hw_of(size)
    _need(rows, torch.int32, "rows")
    _need(true_masks, torch.uint8, "true_masks")
    if true_masks.dim() != 4 or tuple(true_masks.shape[2:]) != (nh, nw) or rows.numel() < njobs:
        raise DisyoloError("window_place_masks: true_masks must be [B,G,%d,%d] and rows hold %d entries (got %s)"
                           % (nh, nw, njobs, tuple(true_masks.shape)))
    _check(load().disyolo_window_place_masks(_p(jobs_dev), njobs, _p(rows), _p(true_masks), int(true_masks.shape[1]), nh, nw,
                                             _stream()), "window_place_masks")


def aug_salt_pepper(image, size, rows, cols, nsalt: int, npepper: int) -> None:
    nh, nw = hw_of(size)
    _check(load().disyolo_aug_salt_pepper_hw(_p(image), nh, nw, _p(rows), _p(cols), nsalt, npepper, _stream()), "aug_salt_pepper")


def aug_change_light(image, size, coeff: float) -> None:
    nh, nw = hw_of(size)
    _check(load().disyolo_aug_change_light_hw(_p(image), nh, nw, float(coeff), _stream()), "aug_change_light")


def aug_motion_blur3(src, dst, size, angle: int, line_type: int) -> None:
    nh, nw = hw_of(size)
    _check(load().disyolo_aug_motion_blur3_hw(_p(src), _p(dst), nh, nw, angle, line_type, _stream()), "aug_motion_blur3")


def aug_to_float(image, out) -> None:
    _need(out, torch.float32, "out")
    _check(load().disyolo_aug_to_float(_p(image), _p(out), image.numel(), _stream()), "aug_to_float")


def confusion16(true_map, pred_map, conf) -> None:
    """adds the 4x4 confusion counts of two uint8 CUDA class maps to conf (int64 [16], CUDA)"""
    _need(true_map, torch.uint8, "true_map")
    _need(pred_map, torch.uint8, "pred_map")
    _need(conf, torch.int64, "conf")
    if true_map.numel() != pred_map.numel() or conf.numel() != 16:
        raise DisyoloError("confusion16: shape mismatch")
    _check(load().disyolo_confusion16(_p(true_map), _p(pred_map), true_map.numel(), _p(conf), _stream()), "confusion16")


def confusion_n(true_map, pred_map, conf, nlabel: int) -> None:
    """adds the nlabel x nlabel confusion counts of two uint8 CUDA class maps to conf (int64 [nlabel * nlabel], CUDA)"""
    _need(true_map, torch.uint8, "true_map")
    _need(pred_map, torch.uint8, "pred_map")
    _need(conf, torch.int64, "conf")
    if true_map.numel() != pred_map.numel() or conf.numel() != nlabel * nlabel:
        raise DisyoloError("confusion_n: shape mismatch")
    _check(load().disyolo_confusion_n(_p(true_map), _p(pred_map), true_map.numel(), nlabel, _p(conf), _stream()),
           "confusion_n")


def upsample2x_bwd(src, dst, B, Hs, Ws, src_C, c_off, C_, accumulate=False) -> None:
    _check(load().disyolo_upsample2x_bwd(_p(src), _p(dst), B, Hs, Ws, src_C, c_off, C_, int(accumulate), _stream()),
           "upsample2x_bwd")


def colsum(x, out, rows, C_, out_C, ws: Workspace) -> None:
    need = load().disyolo_colsum_workspace(rows, C_)
    buf = ws.get(need)
    _check(load().disyolo_colsum(_p(x), _p(out), rows, C_, out_C, _p(buf), buf.numel(), _stream()), "colsum")


def hw_of(size):
    """(H, W) of a size given as one int (a square) or as a pair"""
    if isinstance(size, (int, np.integer)):
        return int(size), int(size)
    h, w = size
    return int(h), int(w)


def detect_takes_x(num_class: int, max_det: int) -> bool:
    """whether ``detect`` calls disyolo_detect_x: more rows than the entry points of before take -- above 64, or, up to 16
    classes, num_class * max_det above the 512 survivors of their LDS rank merge (which they refuse)"""
    return max_det > 64 or (num_class <= 16 and num_class * max_det > 512)


def detect_workspace(B, S, num_class, max_det: int = 0) -> int:
    """bytes of the filter's workspace; it grows with ``max_det`` above 64 (the kept lists)"""
    H, W = hw_of(S)
    if detect_takes_x(num_class, max_det):
        return load().disyolo_detect_workspace_x(B, H, W, num_class, max_det)
    return load().disyolo_detect_workspace_hw(B, H, W, num_class)


def nms_mode(nms) -> int:
    """the DISYOLO_NMS_* value of a mode name"""
    if not isinstance(nms, str) or nms not in NMS_MODES:
        raise ValueError("nms must be one of %s (got %r)" % (", ".join(repr(m) for m in NMS_MODES), nms))
    return NMS_MODES[nms]


def detect_list_capacity() -> int:
    """candidates above the threshold that the image-wide filter ("agnostic", "none") keeps in registers; a longer list
    runs from the workspace, with the same result"""
    return load().disyolo_detect_list_capacity()


def detect(logits3, logits2, logits1, B, S, num_class, anchors_host, clip_window, obj_thresh, nms_thresh, max_det,
           detections, det_count, ws: Workspace, nms: str = "per_class") -> None:
    """``S``: the net's input size, an int or (H, W).  ``nms``: "per_class" (greedy NMS inside each arg-max class),
    "agnostic" (one greedy NMS over all of an image's candidates) or "none" (the max_det highest scores).
    Sizes that disyolo_detect_nms_hw takes go to it as ever; ``max_det`` of 65..256, and up to 16 classes with
    num_class * max_det > 512, take disyolo_detect_x and its workspace (``detect_takes_x``)"""
    H, W = hw_of(S)
    mode = nms_mode(nms)
    anc = (C.c_float * 18)(*[float(v) for v in anchors_host])
    if detect_takes_x(num_class, max_det):
        need = load().disyolo_detect_workspace_x(B, H, W, num_class, max_det)
        if not need:
            raise DisyoloError("detect: max_det must be in 1..%d (got %d)" % (MAX_DET, max_det))
        buf = ws.get(need)
        _check(load().disyolo_detect_x(_p(logits3), _p(logits2), _p(logits1), B, H, W, num_class, anc, _p(clip_window),
                                       obj_thresh, nms_thresh, max_det, mode, _p(detections), _p(det_count), _p(buf),
                                       buf.numel(), _stream()), "detect")
        return
    need = load().disyolo_detect_workspace_hw(B, H, W, num_class)
    buf = ws.get(need)
    _check(load().disyolo_detect_nms_hw(_p(logits3), _p(logits2), _p(logits1), B, H, W, num_class, anc, _p(clip_window),
                                        obj_thresh, nms_thresh, max_det, mode, _p(detections), _p(det_count), _p(buf),
                                        buf.numel(), _stream()), "detect")


def yolo_loss(logits, labels, true_boxes, max_boxes, B, S, num_class, anchors_host, ignore_thresh, scales, dlogits,
              losses, ws: Workspace) -> None:
    """``S``: the net's input size, an int or (H, W)"""
    H, W = hw_of(S)
    need = load().disyolo_yolo_loss_workspace_hw(B, H, W, num_class)
    buf = ws.get(need)
    anc = (C.c_float * 18)(*[float(v) for v in anchors_host])
    lg = (C.c_void_p * 3)(*[_p(t) for t in logits])
    lb = (C.c_void_p * 3)(*[_p(t) for t in labels])
    dl = (C.c_void_p * 3)(*[_p(t) for t in dlogits])
    sc = (C.c_float * 4)(*[float(v) for v in scales])
    _check(load().disyolo_yolo_loss_hw(lg, lb, _p(true_boxes), max_boxes, B, H, W, num_class, 0, anc, ignore_thresh, sc, dl,
                                       _p(losses), _p(buf), buf.numel(), _stream()), "yolo_loss")


def yolo_loss_wide(logits, labels, true_boxes, max_boxes, B, S, num_class, dlogits_ld, anchors_host, ignore_thresh, scales,
                   dlogits, losses, ws: Workspace) -> None:
    """yolo_loss for rows past 32 channels: dlogits bf16 [B, gh, gw, dlogits_ld] per scale"""
    if not dlogits_ld:
        raise DisyoloError("yolo_loss_wide: dlogits_ld must be a positive multiple of 32")
    H, W = hw_of(S)
    need = load().disyolo_yolo_loss_workspace_hw(B, H, W, num_class)
    buf = ws.get(need)
    anc = (C.c_float * 18)(*[float(v) for v in anchors_host])
    lg = (C.c_void_p * 3)(*[_p(t) for t in logits])
    lb = (C.c_void_p * 3)(*[_p(t) for t in labels])
    dl = (C.c_void_p * 3)(*[_p(t) for t in dlogits])
    sc = (C.c_float * 4)(*[float(v) for v in scales])
    _check(load().disyolo_yolo_loss_hw(lg, lb, _p(true_boxes), max_boxes, B, H, W, num_class, dlogits_ld, anc, ignore_thresh,
                                       sc, dl, _p(losses), _p(buf), buf.numel(), _stream()), "yolo_loss_wide")


def shuffle_perm(perm_det, perm_gt, B, seed, step_counter) -> None:
    _check(load().disyolo_shuffle_perm(_p(perm_det), perm_det.shape[1], _p(perm_gt), perm_gt.shape[1], B, seed,
                                       _p(step_counter), _stream()), "shuffle_perm")


def mask_rois(detections, max_det, true_boxes, G, perm_det, perm_gt, B, map_size, n_det, n_gt, iou_thresh, rois,
              roi_count, k: int = 3) -> None:
    """rois int32 [B, ROI_MAX, roi_w(k)]; ``map_size``: the score map's size, an int or (Hm, Wm)"""
    _need_shape(rois, (B, ROI_MAX, roi_w(k)), "mask_rois: rois")
    Hm, Wm = hw_of(map_size)
    _check(load().disyolo_mask_rois_hw(_p(detections), max_det, _p(true_boxes), G, _p(perm_det), _p(perm_gt), B, Hm, Wm,
                                       k, n_det, n_gt, iou_thresh, _p(rois), _p(roi_count), _stream()), "mask_rois")


def psroi_loss(score, true_masks, G, rois, roi_count, B, map_size, k, mask_scale, dscore, loss, ws: Workspace,
               mask_stride: int = 2) -> None:
    """true_masks uint8 [B, G, mask_stride * Hm, mask_stride * Wm], sampled at [::mask_stride, ::mask_stride];
    ``map_size``: the score map's size, an int or (Hm, Wm)"""
    Hm, Wm = hw_of(map_size)
    need = load().disyolo_psroi_loss_workspace_hw(B, Hm, Wm)
    buf = ws.get(need)
    _check(load().disyolo_psroi_loss_hw(_p(score), _p(true_masks), G, _p(rois), _p(roi_count), B, Hm, Wm, mask_stride, k,
                                        mask_scale, _p(dscore), _p(loss), _p(buf), buf.numel(), _stream()), "psroi_loss")


def mask_rois_x(detections, max_det, true_boxes, G, perm_det, perm_gt, B, map_size, n_det, n_gt, iou_thresh, rois,
                roi_count, k: int = 3) -> None:
    """mask_rois for n_det + n_gt up to ROI_CAP: rois int32 [B, roi_cap, roi_w(k)] with roi_cap >= n_det + n_gt"""
    if rois.dim() != 3 or rois.shape[0] != B or rois.shape[2] != roi_w(k):
        raise DisyoloError("mask_rois_x: rois must be [%d, roi_cap, %d] (got %s)" % (B, roi_w(k), tuple(rois.shape)))
    Hm, Wm = hw_of(map_size)
    _check(load().disyolo_mask_rois_x(_p(detections), max_det, _p(true_boxes), G, _p(perm_det), _p(perm_gt), B, Hm, Wm,
                                      k, n_det, n_gt, iou_thresh, rois.shape[1], _p(rois), _p(roi_count), _stream()),
           "mask_rois_x")


def psroi_loss_workspace_x(B, map_size, roi_cap) -> int:
    Hm, Wm = hw_of(map_size)
    return int(load().disyolo_psroi_loss_workspace_x(B, Hm, Wm, roi_cap))


def psroi_loss_x(score, true_masks, G, rois, roi_count, B, map_size, k, mask_scale, dscore, loss, ws: Workspace,
                 mask_stride: int = 2) -> None:
    """psroi_loss on a table rois int32 [B, roi_cap, roi_w(k)] of up to ROI_CAP rows"""
    Hm, Wm = hw_of(map_size)
    roi_cap = rois.shape[1]
    need = load().disyolo_psroi_loss_workspace_x(B, Hm, Wm, roi_cap)
    buf = ws.get(need)
    _check(load().disyolo_psroi_loss_x(_p(score), _p(true_masks), G, _p(rois), _p(roi_count), roi_cap, B, Hm, Wm,
                                       mask_stride, k, mask_scale, _p(dscore), _p(loss), _p(buf), buf.numel(), _stream()),
           "psroi_loss_x")


def psroi_assemble(score, detections, B, max_det, map_size, k, masks, keep) -> None:
    Hm, Wm = hw_of(map_size)
    _check(load().disyolo_psroi_assemble_hw(_p(score), _p(detections), B, max_det, Hm, Wm, k, _p(masks), _p(keep),
                                            _stream()), "psroi_assemble")


def adam_step(w, grad, m, v, n, n_decay, lr, b1, b2, eps, l2, t, grad_scale=1.0) -> None:
    _check(load().disyolo_adam_step(_p(w), _p(grad), _p(m), _p(v), n, n_decay, lr, b1, b2, eps, l2, t, grad_scale,
                                    _stream()), "adam_step")


CURRENT_LANE = 0     # lane the recording thread's launches go to (mirrors the executor's state)


def set_lane(lane: int) -> None:
    global CURRENT_LANE
    _check(load().disyolo_cmdlist_set_lane(lane), "cmdlist_set_lane")
    CURRENT_LANE = lane


def lane_sync(src: int, dst: int) -> None:
    _check(load().disyolo_cmdlist_sync(src, dst), "cmdlist_sync")


def lane_mark(lane: int) -> int:
    """remember this point of `lane` in the recording (-1 when not recording)"""
    r = load().disyolo_cmdlist_mark(lane)
    if r < -1:
        _check(r, "cmdlist_mark")
    return r


def lane_wait(mark: Optional[int], lane: int) -> None:
    if mark is not None and mark >= 0:
        _check(load().disyolo_cmdlist_wait(mark, lane), "cmdlist_wait")


def lane_mark_slot(lane: int, slot: int) -> None:
    """named mark that outlives a replay (see lane_wait_slot)"""
    _check(load().disyolo_cmdlist_mark_slot(lane, slot), "cmdlist_mark_slot")


def lane_wait_slot(slot: int, lane: int) -> None:
    """`lane` waits for the point `slot` was last marked at: earlier in this replay or in the previous replay of the list"""
    _check(load().disyolo_cmdlist_wait_slot(slot, lane), "cmdlist_wait_slot")


def adam_step_dev(w, grad, m, v, n, n_decay, lr, b1, b2, eps, l2, step_counter, grad_scale=1.0) -> None:
    _check(load().disyolo_adam_step_dev(_p(w), _p(grad), _p(m), _p(v), n, n_decay, lr, b1, b2, eps, l2,
                                        _p(step_counter), grad_scale, _stream()), "adam_step_dev")


def adam_step_fused(w, grad, m, v, n, n_decay, lr_dev, b1, b2, eps, l2, step_counter, grad_scale, reg_loss_out,
                    ws: Workspace) -> None:
    """Adam with lr and t on the device; also writes 0.5*l2*sum(w_decay^2) of the pre-update weights"""
    _need(lr_dev, torch.float32, "lr_dev")
    need = load().disyolo_adam_fused_workspace(n)
    buf = ws.get(need)
    _check(load().disyolo_adam_step_fused(_p(w), _p(grad), _p(m), _p(v), n, n_decay, _p(lr_dev), b1, b2, eps, l2,
                                          _p(step_counter), grad_scale, _p(reg_loss_out), _p(buf), buf.numel(),
                                          _stream()), "adam_step_fused")


def adam_sweep_parts(n: int) -> int:
    return load().disyolo_adam_sweep_parts(n)


def adam_sweep(w, grad, m, v, n, n_decay, lr_dev, b1, b2, eps, l2, step_counter, grad_scale, parts) -> None:
    """Adam over one slice of the variables (t = *step_counter + 1, counter untouched); l2 partials -> parts"""
    _check(load().disyolo_adam_sweep(_p(w), _p(grad), _p(m), _p(v), n, n_decay, _p(lr_dev), b1, b2, eps, l2,
                                     _p(step_counter), grad_scale, _p(parts), _stream()), "adam_sweep")


def adam_finish(step_counter, parts, nparts, l2, reg_loss_out, record=None) -> None:
    """record = (losses8, mask_loss, reg_loss_in or None, ring): also file the step's total loss into the ring"""
    if record is None:
        _check(load().disyolo_adam_finish(_p(step_counter), _p(parts), nparts, l2, _p(reg_loss_out), _stream()),
               "adam_finish")
        return
    losses8, mask_loss, reg_in, ring = record
    _need(ring, torch.float32, "ring")
    _check(load().disyolo_adam_finish_record(_p(step_counter), _p(parts), nparts, l2, _p(reg_loss_out), _p(losses8),
                                             _p(mask_loss), _p(reg_in), _p(ring), ring.numel(), _stream()), "adam_finish_record")


def add_bf16(src, dst, accumulate: bool) -> None:
    _check(load().disyolo_add_bf16(_p(src), _p(dst), src.numel(), int(accumulate), _stream()), "add_bf16")


def l2_loss(w, n, l2, out, ws: Workspace) -> None:
    need = load().disyolo_l2_workspace(n)
    buf = ws.get(need)
    _check(load().disyolo_l2_loss(_p(w), n, l2, _p(out), _p(buf), buf.numel(), _stream()), "l2_loss")


# ---- gradient exchange as commands of the step (csrc/comm.hip) -------------------------------------------------
COMM_LANE = 3        # the list's lane that carries the collectives and the optimizer sweeps behind them
_DT_CODE = {torch.float32: 0, torch.bfloat16: 1, torch.float64: 2}


def reserve_lanes(lanes=(1, COMM_LANE)) -> None:
    """create the side streams of these lanes now (current device).  A data-parallel process calls this BEFORE
    torch.distributed.init_process_group("nccl"): streams created after torch's stream pool exists share hardware
    queues with it, and a lane that shares the caller's stream's queue serialises the step (2.5x, round 5)."""
    mask = 0
    for i in lanes:
        mask |= 1 << int(i)
    _check(load().disyolo_lanes_reserve(mask), "lanes_reserve")


def lanes_report() -> list:
    """how the side lanes that exist on the current device were chosen (csrc/runtime.hip pool_lane): one string per lane"""
    buf = C.create_string_buffer(2048)
    _check(load().disyolo_lanes_report(buf, len(buf)), "lanes_report")
    return [ln for ln in buf.value.decode().splitlines() if ln]


def rccl_path() -> Optional[str]:
    """the RCCL copy this process already maps (torch ships one next to libtorch_hip.so); None = default search"""
    p = os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so")
    return p if os.path.exists(p) else None


def comm_load() -> int:
    """dlopen RCCL inside the kernel library; returns RCCL's version code.  Raises DisyoloError when it cannot."""
    p = rccl_path()
    ver = C.c_int(0)
    _check(load().disyolo_comm_load(p.encode() if p else None, C.byref(ver)), "comm_load")
    return ver.value


class Comm:
    """An RCCL communicator owned by the kernel library, one rank per process.  Created collectively: rank 0 makes the
    128-byte id, ``exchange(id_bytes or None) -> id_bytes`` hands it to every rank (torch.distributed's
    broadcast_object_list in dp.py -- any backend, used once), then every rank joins.  The collectives are recordable:
    inside a CmdList recording they become commands of the current lane."""

    def __init__(self, rank: int, world: int, exchange):
        comm_load()
        ident = None
        if rank == 0:
            buf = C.create_string_buffer(128)
            _check(load().disyolo_comm_unique_id(buf), "comm_unique_id")
            ident = buf.raw
        ident = exchange(ident)
        if not isinstance(ident, (bytes, bytearray)) or len(ident) != 128:
            raise DisyoloError("Comm: the id exchange must return rank 0's 128 bytes on every rank")
        h = C.c_void_p()
        _check(load().disyolo_comm_init(C.create_string_buffer(bytes(ident), 128), rank, world, C.byref(h)), "comm_init")
        self.h, self.rank, self.world = h, rank, world

    def close(self) -> None:
        """destroy the communicator (a collective: every rank must call it); device work that uses it is drained first"""
        if getattr(self, "h", None):
            torch.cuda.synchronize()
            _check(load().disyolo_comm_destroy(self.h), "comm_destroy")
            self.h = None

    def __del__(self):
        # a dropped communicator is released like a closed one (its buffers are device memory); at interpreter exit the
        # runtime may already be gone: never raise from here
        try:
            if getattr(self, "h", None) and torch.cuda.is_available():
                self.close()
        except Exception:
            pass

    def allreduce(self, t: torch.Tensor) -> None:
        """t = sum over the ranks (in place), on the current stream / lane"""
        if t.dtype not in _DT_CODE or not t.is_cuda or not t.is_contiguous():
            raise DisyoloError("Comm.allreduce: contiguous CUDA f32 / bf16 / f64 tensor expected")
        _check(load().disyolo_comm_allreduce_sum(self.h, _p(t), t.numel(), _DT_CODE[t.dtype], _stream()), "comm_allreduce_sum")

    def reduce_scatter(self, full: torch.Tensor) -> torch.Tensor:
        """in place: this rank's shard of ``full`` (numel a multiple of the world size) = its sum over the ranks;
        returns the shard view"""
        n = full.numel() // self.world
        if n * self.world != full.numel() or full.dtype not in _DT_CODE or not full.is_contiguous():
            raise DisyoloError("Comm.reduce_scatter: numel must be a multiple of the world size")
        shard = full.view(-1)[self.rank * n:(self.rank + 1) * n]
        _check(load().disyolo_comm_reduce_scatter_sum(self.h, _p(full), _p(shard), n, _DT_CODE[full.dtype], _stream()),
               "comm_reduce_scatter_sum")
        return shard

    def all_gather(self, full: torch.Tensor) -> None:
        """in place: every rank's shard of ``full`` to every rank"""
        n = full.numel() // self.world
        shard = full.view(-1)[self.rank * n:(self.rank + 1) * n]
        _check(load().disyolo_comm_all_gather(self.h, _p(shard), _p(full), n, _DT_CODE[full.dtype], _stream()), "comm_all_gather")


def cast_f32_bf16(src: torch.Tensor, dst: torch.Tensor) -> None:
    _need(src, torch.float32, "src")
    _need(dst, torch.bfloat16, "dst")
    if dst.numel() < src.numel():
        raise DisyoloError("cast_f32_bf16: destination shorter than the source")
    _check(load().disyolo_cast_f32_bf16(_p(src), _p(dst), src.numel(), _stream()), "cast_f32_bf16")


def cast_bf16_f32(src: torch.Tensor, dst: torch.Tensor) -> None:
    _need(src, torch.bfloat16, "src")
    _need(dst, torch.float32, "dst")
    if src.numel() < dst.numel():
        raise DisyoloError("cast_bf16_f32: source shorter than the destination")
    _check(load().disyolo_cast_bf16_f32(_p(src), _p(dst), dst.numel(), _stream()), "cast_bf16_f32")
