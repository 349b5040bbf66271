"""ctypes binding of libaqengine.so (include/aq_engine.h) + the Python-side engine object.

Mirrors the two operator seams of the reference's ``yolov5/detect.py`` (reference README.md:77)
[UPSTREAM detect.py run()]:

    pred = model(im)                                   -> Engine.forward_raw(tiles_u8)
    pred = non_max_suppression(pred, conf, iou, ...)   -> Engine.nms(pred, ...)
    both, fused, from uint8 tiles                      -> Engine.infer(tiles_u8, ...)

PyTorch is used for device memory and streams only.  There is NO fallback: if the HIP library
cannot be loaded, or no GPU is present, construction raises.
"""
from __future__ import annotations

import ctypes as C
import os
import re
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import spec as _spec
from .checkpoint import Checkpoint, pack_plan_weights

AQ_BF16, AQ_FP32, AQ_BF16_W8, AQ_F16X3 = 0, 1, 2, 3
PRECISIONS = {"bf16": AQ_BF16, "fp32": AQ_FP32, "fp8w": AQ_BF16, "f16x3": AQ_F16X3}
"""Compute precision of the single-op helpers.  fp8w = fp8 (OCP e4m3fn) weights with per-output-channel power-of-two scales, bf16
activations (quant.py): values bf16 holds exactly, so every bf16 kernel runs them as they are."""
ENGINE_PRECISIONS = {"bf16": AQ_BF16, "fp32": AQ_FP32, "fp8w": AQ_BF16_W8, "f16x3": AQ_F16X3, "fp8": AQ_BF16}
"""aq_model_desc.precision.  AQ_BF16_W8 computes as AQ_BF16; kernels with an fp8-weight stream (the planar 3x3) load the e4m3 codes."""
_DTYPE_CODE = {"act": 0, "f32": 1, "u8": 2}

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libaqengine.so")


class aq_tensor_desc(C.Structure):
    _fields_ = [("channels", C.c_int32), ("down", C.c_int32), ("dtype", C.c_int32)]


class aq_slice(C.Structure):
    _fields_ = [("tensor", C.c_int32), ("ch_off", C.c_int32), ("channels", C.c_int32)]


class aq_op_desc(C.Structure):
    _fields_ = [("kind", C.c_int32), ("src", aq_slice), ("dst", aq_slice), ("res", aq_slice),
                ("k", C.c_int32), ("stride", C.c_int32), ("pad", C.c_int32), ("act", C.c_int32),
                ("level", C.c_int32), ("weight", C.POINTER(C.c_float)), ("bias", C.POINTER(C.c_float)),
                ("flops_per_tile", C.c_double)]


class aq_model_desc(C.Structure):
    _fields_ = [("precision", C.c_int32), ("nc", C.c_int32), ("na", C.c_int32), ("nl", C.c_int32),
                ("anchors_px", C.c_float * 2 * 8 * 3), ("stride", C.c_float * 3),
                ("head_tensor", C.c_int32 * 3), ("input_tensor", C.c_int32),
                ("n_tensors", C.c_int32), ("n_ops", C.c_int32),
                ("tensors", C.POINTER(aq_tensor_desc)), ("ops", C.POINTER(aq_op_desc))]


class aq_det(C.Structure):
    _fields_ = [("x1", C.c_float), ("y1", C.c_float), ("x2", C.c_float), ("y2", C.c_float),
                ("conf", C.c_float), ("cls", C.c_float)]


# every symbol include/aq_engine.h declares (tests check the library exports all of them)
EXPORTS = (
    "aq_last_error", "aq_version", "aq_engine_create", "aq_engine_destroy", "aq_engine_workspace_bytes", "aq_size_guard",
    "aq_engine_infer", "aq_engine_run_ops", "aq_engine_candidates", "aq_engine_forward_raw", "aq_engine_tensor_ptr", "aq_engine_profile",
    "aq_engine_op_times", "aq_engine_num_ops", "aq_engine_set_conv_config", "aq_engine_autotune", "aq_engine_set_tuned_table",
    "aq_engine_get_conv_config", "aq_conv_num_configs", "aq_debug_conv_stamp", "aq_debug_mfma_peak",
    "aq_conv_config_tiles", "aq_pack_conv_weights", "aq_pack_conv_weights_x3", "aq_conv2d", "aq_pack_stem_weights", "aq_stem_conv", "aq_pack_bottleneck_weights", "aq_bottleneck", "aq_bottleneck_asm_form", "aq_bottleneck_c3tail_supported", "aq_pack_bottleneck_c3tail_weights", "aq_bottleneck_c3tail", "aq_pack_downblock_weights", "aq_downblock", "aq_stemdown_supported", "aq_stemdown", "aq_conv1x1_direct_supported", "aq_pack_conv1x1_direct", "aq_conv1x1_direct", "aq_conv1x1_asm_supported", "aq_pack_conv1x1_asm", "aq_conv1x1_asm", "aq_nms_opts", "aq_engine_set_nms_options",
    "aq_conv3x3s2_direct_supported", "aq_pack_conv3x3s2_direct", "aq_conv3x3s2_direct",
    "aq_conv3x3_pl_supported", "aq_conv3x3_pl_asm_family", "aq_pack_conv3x3_pl", "aq_conv3x3_pl", "aq_conv3x3_pl_s2_supported", "aq_pack_conv3x3_pl_s2", "aq_conv3x3_pl_s2", "aq_jpeg_scratch_bytes", "aq_jpeg_idct_rgb", "aq_jpeg_idct_rgb_checked", "aq_f32_to_e4m3", "aq_conv1x1_direct_f8out", "aq_absmax_bf16", "aq_engine_calibrate_amax", "aq_engine_set_fp8_scales", "aq_engine_last_launch", "aq_conv3x3_pl_f8_supported", "aq_pack_conv3x3_pl_f8", "aq_conv3x3_pl_f8", "aq_conv3x3_pl_w8_supported", "aq_pack_conv3x3_pl_w8", "aq_conv3x3_pl_w8", "aq_head_decode_supported", "aq_pack_head_weights", "aq_head_decode", "aq_head_counts_gather", "aq_preprocess_s2d", "aq_sppf_pool",
    "aq_upsample2x", "aq_letterbox_u8", "aq_letterbox_tiles_u8", "aq_format_label_rows", "aq_detect_decode", "aq_nms_scratch_bytes", "aq_nms", "aq_jpeg_huffman_decode", "aq_write_label_files",
    "aq_crop_jpeg_coefs", "aq_crop_jpeg_bytes", "aq_write_crop_files",
    "aq_annotate_u8", "aq_image_jpeg_coefs", "aq_image_jpeg_bytes", "aq_write_image_files",
    "aq_image_jpeg_coefs_q", "aq_image_jpeg_bytes_q", "aq_write_image_files_q", "aq_val_mosaic_u8",
    "aq_blank_stats_scratch_bytes", "aq_blank_stats_u8",
    "aq_blank_geom_scratch_bytes", "aq_blank_components_u8", "aq_blank_ring_edges_u8",
    "aq_facility_scratch_bytes", "aq_facility_dbscan_f64",
    "aq_land_scratch_bytes", "aq_land_filter_f64",
    "aq_land_images_scratch_bytes", "aq_land_images_f64",
    "aq_eval_scratch_bytes", "aq_eval_member_conf_f64", "aq_box_match_f64",
    "aq_eval_subsets_scratch_bytes", "aq_eval_member_conf_subsets_f64", "aq_box_match_subsets_scratch_bytes", "aq_box_match_subsets_f64",
    "aq_model_error_match_f64", "aq_model_error_moments_f64",
    "aq_tonnage_simulate_f64", "aq_tonnage_reduce_f64", "aq_tonnage_ndtri_f64", "aq_tonnage_uniform_f64",
    "aq_bernoulli_counts_i32",
    "aq_depth_ranges_f64", "aq_depth_stats_f64",
    "aq_dedup_fill_u32", "aq_dedup_sets_u32", "aq_dedup_select_f64",
    "aq_coverage_first_i32",
    "aq_overlap_partners_f64", "aq_overlap_clip_f64",
    "aq_facility_bounds_f64", "aq_box_join_count_i32", "aq_box_join_list_i32",
    "aq_val_expand_scratch_bytes", "aq_val_expand_rows_f32", "aq_val_match", "aq_val_score_chunk", "aq_val_scores_scratch_bytes", "aq_val_scores_f64",
    "aq_val_confusion_scratch_bytes", "aq_val_confusion",
    "aq_augment_geometry", "aq_augment_taps", "aq_stem_conv_scaled", "aq_preprocess_s2d_scaled", "aq_head_decode_aug", "aq_detect_decode_aug",
    "aq_engine_workspace_bytes_augment", "aq_engine_infer_augment", "aq_engine_forward_raw_augment", "aq_engine_last_launch_augment",
)

_lib = None


def load_library(path: str = LIB_PATH) -> C.CDLL:
    """dlopen libaqengine.so and set argument types.  Raises if it is missing (no fallback path)."""
    global _lib
    if _lib is not None:
        return _lib
    if path == LIB_PATH and os.environ.get("AQ_ENGINE_LIB"):
        path = os.environ["AQ_ENGINE_LIB"]             # A/B runs of two builds of the library in one session (tools/build_variant.py)
    if not os.path.exists(path):
        raise RuntimeError(f"{path} not found: build it with `python -m aquaculture_amd.build` "
                           "(there is no CPU/PyTorch fallback for the detect path)")
    lib = C.CDLL(path)
    vp, i32, f32, sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t
    lib.aq_last_error.restype = C.c_char_p
    lib.aq_engine_create.argtypes = [C.POINTER(aq_model_desc), i32, C.POINTER(vp)]
    lib.aq_engine_destroy.argtypes = [vp]
    lib.aq_engine_destroy.restype = None
    lib.aq_engine_workspace_bytes.argtypes = [vp, i32, i32, i32, C.POINTER(sz)]
    lib.aq_size_guard.argtypes = [i32, C.POINTER(C.c_longlong), i32]
    lib.aq_engine_infer.argtypes = [vp, vp, i32, i32, i32, vp, sz, vp, vp, f32, f32, i32, vp]
    lib.aq_engine_run_ops.argtypes = [vp, vp, i32, i32, i32, vp, sz, i32, i32, f32, f32, i32, vp, vp, vp]
    lib.aq_engine_candidates.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(i32)]
    lib.aq_engine_forward_raw.argtypes = [vp, vp, i32, i32, i32, vp, sz, vp, vp]
    lib.aq_engine_tensor_ptr.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    lib.aq_engine_profile.argtypes = [vp, i32, i32]
    lib.aq_engine_op_times.argtypes = [vp, C.POINTER(f32), i32, C.POINTER(i32)]
    lib.aq_engine_num_ops.argtypes = [vp]
    lib.aq_engine_set_conv_config.argtypes = [vp, i32, i32]
    lib.aq_engine_autotune.argtypes = [vp, vp, i32, i32, i32, vp, sz, i32, vp]
    lib.aq_engine_get_conv_config.argtypes = [vp, i32]
    lib.aq_engine_last_launch.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(i32)]
    lib.aq_jpeg_huffman_decode.argtypes = [vp, vp, i32, vp, vp, vp, vp]
    lib.aq_write_label_files.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), C.POINTER(f32), C.POINTER(C.c_longlong), i32, i32, i32]
    lib.aq_write_label_files.restype = C.c_long
    lib.aq_crop_jpeg_coefs.argtypes = [vp, C.c_longlong, vp, i32, i32, vp, vp]
    lib.aq_crop_jpeg_bytes.argtypes = [vp, i32, i32, vp, sz]
    lib.aq_crop_jpeg_bytes.restype = C.c_long
    lib.aq_write_crop_files.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), vp, vp, i32, i32, i32]
    lib.aq_write_crop_files.restype = C.c_long
    lib.aq_annotate_u8.argtypes = [vp, C.c_longlong, vp, C.c_longlong, vp, vp, i32, vp, i32, vp, i32, vp, i32, vp, C.c_longlong, vp]
    lib.aq_image_jpeg_coefs.argtypes = [vp, C.c_longlong, vp, vp, i32, i32, vp, vp]
    lib.aq_image_jpeg_bytes.argtypes = [vp, i32, i32, vp, sz]
    lib.aq_image_jpeg_bytes.restype = C.c_long
    lib.aq_write_image_files.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), vp, vp, i32, i32, i32]
    lib.aq_write_image_files.restype = C.c_long
    lib.aq_image_jpeg_coefs_q.argtypes = [vp, C.c_longlong, vp, vp, i32, i32, i32, vp, vp]
    lib.aq_image_jpeg_bytes_q.argtypes = [vp, i32, i32, i32, vp, sz]
    lib.aq_image_jpeg_bytes_q.restype = C.c_long
    lib.aq_write_image_files_q.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), vp, vp, i32, i32, i32, i32]
    lib.aq_write_image_files_q.restype = C.c_long
    lib.aq_val_mosaic_u8.argtypes = [vp, C.c_longlong, i32, i32, i32, i32, i32, i32, vp, C.c_longlong, i32, i32, vp, vp, vp, vp, vp]
    lib.aq_blank_stats_scratch_bytes.argtypes = [vp, i32]
    lib.aq_blank_stats_scratch_bytes.restype = sz
    lib.aq_blank_stats_u8.argtypes = [vp, C.c_longlong, vp, vp, i32, vp, sz, vp, vp]
    lib.aq_blank_geom_scratch_bytes.argtypes = [vp, i32]
    lib.aq_blank_geom_scratch_bytes.restype = sz
    lib.aq_blank_components_u8.argtypes = [vp, C.c_longlong, vp, vp, i32, vp, vp, sz, vp, vp, vp]
    lib.aq_blank_ring_edges_u8.argtypes = [vp, vp, i32, vp, sz, vp, vp, vp, vp, C.c_longlong, vp]
    lib.aq_facility_scratch_bytes.argtypes = [C.c_longlong]
    lib.aq_facility_scratch_bytes.restype = sz
    lib.aq_facility_dbscan_f64.argtypes = [vp, vp, vp, vp, C.c_longlong, C.c_double, i32, vp, sz, vp, vp, vp]
    lib.aq_land_scratch_bytes.argtypes = [C.c_longlong]
    lib.aq_land_scratch_bytes.restype = sz
    lib.aq_land_filter_f64.argtypes = [vp, C.c_longlong, vp, C.c_longlong, vp, i32, C.c_double, C.c_double, vp, C.c_longlong, vp, sz, vp, vp]
    lib.aq_land_images_scratch_bytes.argtypes = [C.c_longlong]
    lib.aq_land_images_scratch_bytes.restype = sz
    lib.aq_land_images_f64.argtypes = [vp, C.c_longlong, vp, C.c_longlong, vp, i32, C.c_double, C.c_double, vp, C.c_longlong, C.c_double, vp, sz, vp, vp, vp]
    lib.aq_eval_scratch_bytes.argtypes = [C.c_longlong, i32]
    lib.aq_eval_scratch_bytes.restype = sz
    lib.aq_eval_member_conf_f64.argtypes = [vp, vp, vp, vp, vp, C.c_longlong, C.c_double, i32, vp, sz, vp, vp]
    lib.aq_box_match_f64.argtypes = [vp, vp, C.c_longlong, vp, C.c_longlong, vp, i32, vp, i32, vp, vp, vp]
    lib.aq_eval_subsets_scratch_bytes.argtypes = [C.c_longlong, i32, i32]
    lib.aq_eval_subsets_scratch_bytes.restype = sz
    lib.aq_eval_member_conf_subsets_f64.argtypes = [vp, vp, vp, vp, vp, vp, C.c_longlong, C.c_double, i32, i32, vp, sz, vp, vp]
    lib.aq_box_match_subsets_scratch_bytes.argtypes = [C.c_longlong, C.c_longlong, i32, i32]
    lib.aq_box_match_subsets_scratch_bytes.restype = sz
    lib.aq_box_match_subsets_f64.argtypes = [vp, vp, vp, C.c_longlong, vp, vp, C.c_longlong, vp, i32, vp, i32, i32, vp, vp, vp]
    lib.aq_model_error_match_f64.argtypes = [vp, vp, vp, C.c_longlong, vp, vp, vp, C.c_longlong, vp, i32, vp, vp, vp, vp]
    lib.aq_model_error_moments_f64.argtypes = [vp, vp, vp, C.c_longlong, C.c_longlong, vp, vp, vp, vp]
    lib.aq_tonnage_simulate_f64.argtypes = [C.c_ulonglong, C.c_longlong, C.c_longlong, vp, vp, C.c_longlong, vp, vp, vp, C.c_longlong, vp, vp, vp, vp, i32,
                                            C.c_double, C.c_double, vp, vp, vp]
    lib.aq_tonnage_reduce_f64.argtypes = [vp, C.c_longlong, C.c_longlong, vp, i32, vp, vp, vp]
    lib.aq_tonnage_ndtri_f64.argtypes = [vp, C.c_longlong, vp, vp]
    lib.aq_tonnage_uniform_f64.argtypes = [C.c_ulonglong, vp, C.c_longlong, vp, vp]
    lib.aq_bernoulli_counts_i32.argtypes = [C.c_ulonglong, C.c_longlong, C.c_longlong, C.c_longlong, vp, vp, i32, vp, vp]
    lib.aq_depth_ranges_f64.argtypes = [vp, C.c_longlong, vp, C.c_longlong, C.c_double, C.c_double, C.c_double, C.c_double, i32, i32, vp, vp, vp]
    lib.aq_depth_stats_f64.argtypes = [vp, C.c_longlong, vp, C.c_longlong, vp, vp, vp, vp, vp, i32, i32, C.c_double, vp, C.c_longlong, vp, vp, vp]
    lib.aq_engine_set_tuned_table.argtypes = [vp, i32, i32, i32, C.POINTER(i32), i32]
    lib.aq_engine_calibrate_amax.argtypes = [vp, vp, i32, i32, i32, vp, sz, C.POINTER(f32), i32, vp]
    lib.aq_engine_set_fp8_scales.argtypes = [vp, C.POINTER(f32), i32]
    lib.aq_conv1x1_direct_f8out.argtypes = [vp, i32, i32, vp, i32, i32, i32, i32, vp, vp, C.c_longlong, i32, f32, vp]
    lib.aq_absmax_bf16.argtypes = [vp, i32, i32, i32, C.c_longlong, vp, vp]
    lib.aq_debug_conv_stamp.argtypes = [vp, sz]
    lib.aq_debug_mfma_peak.argtypes = [i32, i32, vp, vp]
    lib.aq_conv_config_tiles.argtypes = [i32, C.POINTER(i32), C.POINTER(i32)]
    lib.aq_pack_conv_weights.argtypes = [C.POINTER(f32), i32, i32, i32, i32, vp, C.POINTER(sz), vp]
    lib.aq_pack_conv_weights_x3.argtypes = [C.POINTER(f32), C.POINTER(f32), i32, i32, i32, vp, C.POINTER(sz), vp, C.POINTER(sz), vp]
    lib.aq_conv2d.argtypes = [vp, i32, i32, i32, vp, i32, i32, i32, vp, i32, i32, vp, vp,
                              i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp]
    lib.aq_pack_stem_weights.argtypes = [C.POINTER(f32), i32, i32, vp, C.POINTER(sz), vp]
    lib.aq_stem_conv.argtypes = [vp, vp, i32, i32, i32, vp, vp, i32, i32, i32, i32, i32, vp]
    lib.aq_pack_bottleneck_weights.argtypes = [C.POINTER(f32), C.POINTER(f32), i32, vp, C.POINTER(sz), vp]
    lib.aq_bottleneck.argtypes = [vp, i32, i32, vp, i32, i32, i32, vp, vp, i32, i32, i32, i32, vp]
    lib.aq_bottleneck_asm_form.argtypes = [i32] * 6
    lib.aq_bottleneck_c3tail_supported.argtypes = [i32, i32, i32, i32, i32, i32]
    lib.aq_pack_bottleneck_c3tail_weights.argtypes = [C.POINTER(f32), C.POINTER(f32), C.POINTER(f32), vp, C.POINTER(sz), vp]
    lib.aq_bottleneck_c3tail.argtypes = [vp, i32, i32, vp, i32, i32, vp, i32, i32, vp, vp, i32, i32, i32, i32, vp]
    lib.aq_pack_downblock_weights.argtypes = [C.POINTER(f32), C.POINTER(f32), vp, C.POINTER(sz), vp]
    lib.aq_downblock.argtypes = [vp, i32, i32, vp, i32, i32, vp, vp, i32, i32, i32, vp]
    lib.aq_conv1x1_direct_supported.argtypes = [i32, i32]
    lib.aq_pack_conv1x1_direct.argtypes = [C.POINTER(f32), i32, i32, vp, C.POINTER(sz), vp]
    lib.aq_conv1x1_direct.argtypes = [vp, i32, i32, vp, i32, i32, i32, i32, vp, vp, C.c_longlong, i32, vp]
    lib.aq_nms_opts.argtypes = [vp, i32, i32, i32, i32, f32, f32, i32, vp, vp, i32, vp, vp, vp, i32, C.c_ulonglong, C.c_ulonglong, vp]
    lib.aq_engine_set_nms_options.argtypes = [vp, i32, C.c_ulonglong, C.c_ulonglong]
    lib.aq_conv1x1_asm_supported.argtypes = [i32, i32]
    lib.aq_pack_conv1x1_asm.argtypes = [C.POINTER(f32), i32, i32, vp, C.POINTER(sz), vp]
    lib.aq_conv1x1_asm.argtypes = [vp, i32, i32, vp, i32, i32, i32, i32, vp, vp, C.c_longlong, i32, vp]
    lib.aq_conv3x3s2_direct_supported.argtypes = [i32, i32]
    lib.aq_pack_conv3x3s2_direct.argtypes = [C.POINTER(f32), i32, i32, vp, C.POINTER(sz), vp]
    lib.aq_conv3x3s2_direct.argtypes = [vp, i32, i32, vp, i32, i32, i32, i32, vp, vp, i32, i32, i32, i32, vp]
    lib.aq_conv3x3_pl_supported.argtypes = [i32, i32]
    lib.aq_conv3x3_pl_asm_family.argtypes = [i32]
    lib.aq_pack_conv3x3_pl.argtypes = [C.POINTER(f32), i32, i32, vp, C.POINTER(sz), vp]
    lib.aq_conv3x3_pl.argtypes = [vp, C.c_longlong, C.c_longlong, i32, vp, i32, i32, i32, vp, i32, i32, vp, vp, i32, i32, i32, i32, vp]
    lib.aq_conv3x3_pl_w8.argtypes = lib.aq_conv3x3_pl.argtypes
    lib.aq_pack_conv3x3_pl_w8.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_float), i32, i32, vp, C.POINTER(C.c_size_t), vp, vp]
    lib.aq_conv3x3_pl_w8_supported.argtypes = [i32] * 5
    lib.aq_jpeg_scratch_bytes.argtypes = [i32, i32, i32]
    lib.aq_jpeg_scratch_bytes.restype = sz
    lib.aq_jpeg_idct_rgb.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp, vp]
    lib.aq_jpeg_idct_rgb_checked.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp, vp, vp]
    lib.aq_f32_to_e4m3.argtypes = [f32]
    lib.aq_f32_to_e4m3.restype = C.c_ubyte
    lib.aq_conv3x3_pl_f8_supported.argtypes = [i32] * 5
    lib.aq_pack_conv3x3_pl_f8.argtypes = [C.POINTER(f32), C.POINTER(f32), i32, i32, f32, vp, C.POINTER(sz), vp, vp]
    lib.aq_conv3x3_pl_f8.argtypes = [vp, i32, i32, i32, vp, i32, i32, i32, vp, i32, i32, vp, vp, i32, i32, i32, i32, vp]
    lib.aq_conv3x3_pl_s2_supported.argtypes = [i32] * 5
    lib.aq_pack_conv3x3_pl_s2.argtypes = [C.POINTER(f32), i32, i32, vp, C.POINTER(sz), vp]
    lib.aq_conv3x3_pl_s2.argtypes = [vp, i32, i32, i32, vp, i32, i32, i32, vp, vp, i32, i32, i32, i32, vp]
    lib.aq_preprocess_s2d.argtypes = [vp, vp, i32, i32, i32, i32, vp]
    lib.aq_sppf_pool.argtypes = [vp, i32, i32, i32, i32, i32, i32, i32, vp]
    lib.aq_upsample2x.argtypes = [vp, i32, i32, vp, i32, i32, i32, i32, i32, i32, i32, vp]
    lib.aq_letterbox_u8.argtypes = [vp, i32, i32, i32, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp]
    lib.aq_letterbox_tiles_u8.argtypes = [vp, C.c_longlong, C.c_longlong, vp, vp, i32, i32, i32, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp]
    lib.aq_format_label_rows.argtypes = [C.POINTER(f32), i32, i32, C.c_char_p, sz]
    lib.aq_format_label_rows.restype = C.c_long
    lib.aq_detect_decode.argtypes = [C.POINTER(vp), i32, i32, i32, i32, i32, i32, C.POINTER(f32), C.POINTER(f32),
                                     vp, f32, vp, vp, vp, i32, vp]
    lib.aq_nms_scratch_bytes.argtypes = [i32, i32]
    lib.aq_nms_scratch_bytes.restype = sz
    lib.aq_nms.argtypes = [vp, i32, i32, i32, i32, f32, f32, i32, vp, vp, i32, vp, vp, vp, vp]
    lib.aq_dedup_fill_u32.argtypes = [vp, C.c_longlong, vp, vp, vp, vp, C.c_longlong, vp, C.c_longlong, vp]
    lib.aq_dedup_sets_u32.argtypes = [vp, vp, C.c_longlong, vp, C.c_longlong, vp, C.c_longlong, vp, vp]
    lib.aq_dedup_select_f64.argtypes = [vp, vp, vp, vp, C.c_longlong, vp, vp, vp, C.c_longlong, vp, vp, vp, vp, vp]
    lib.aq_coverage_first_i32.argtypes = [vp, vp, vp, C.c_longlong, vp, C.c_longlong, vp, C.c_longlong, vp, vp, vp, vp, C.c_longlong, C.c_longlong,
                                          vp, vp, C.c_longlong, vp, sz, vp, vp]
    lib.aq_overlap_partners_f64.argtypes = [vp, C.c_longlong, vp, C.c_longlong, vp, C.c_longlong, C.c_double, C.c_double, vp, vp, C.c_longlong, vp]
    lib.aq_overlap_clip_f64.argtypes = [vp, C.c_longlong, vp, vp, C.c_longlong, vp, vp, C.c_longlong, vp, vp, vp, vp, vp]
    lib.aq_facility_bounds_f64.argtypes = [vp, vp, C.c_longlong, vp, vp, C.c_longlong, vp, vp]
    lib.aq_box_join_count_i32.argtypes = [vp, vp, C.c_longlong, vp, vp, vp, vp, C.c_longlong, C.c_longlong, vp, vp, vp]
    lib.aq_box_join_list_i32.argtypes = [vp, vp, C.c_longlong, vp, vp, vp, vp, C.c_longlong, C.c_longlong, vp, vp, vp, C.c_longlong, vp]
    lib.aq_val_expand_scratch_bytes.argtypes = [i32, i32, i32]
    lib.aq_val_expand_scratch_bytes.restype = sz
    lib.aq_val_expand_rows_f32.argtypes = [vp, i32, i32, i32, f32, i32, vp, sz, vp, vp, vp]
    lib.aq_val_match.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp, C.c_longlong, vp, vp, vp, vp, vp, vp, C.c_longlong, vp, vp]
    lib.aq_val_confusion_scratch_bytes.argtypes = [i32, i32, C.c_longlong]
    lib.aq_val_confusion_scratch_bytes.restype = sz
    lib.aq_val_confusion.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp, vp, C.c_longlong, vp, i32, f32, f32, vp, sz, vp, vp, vp, vp]
    lib.aq_val_score_chunk.argtypes = []
    lib.aq_val_scores_scratch_bytes.argtypes = [C.c_longlong, C.c_longlong]
    lib.aq_val_scores_scratch_bytes.restype = sz
    lib.aq_val_scores_f64.argtypes = [vp, vp, C.c_longlong, vp, vp, vp, vp, vp, i32, vp, i32, vp, i32, vp, sz, vp, vp, vp, vp, vp]
    lib.aq_augment_geometry.argtypes = [i32, i32, i32, vp, C.POINTER(i32)]
    lib.aq_augment_taps.argtypes = [i32, i32, i32, vp]
    lib.aq_stem_conv_scaled.argtypes = [vp, i32, i32, vp, vp, i32, i32, vp, i32, i32, i32, vp, vp, i32, i32, i32, i32, i32, vp]
    lib.aq_preprocess_s2d_scaled.argtypes = [vp, i32, i32, vp, vp, i32, i32, vp, i32, i32, i32, i32, vp]
    lib.aq_head_decode_aug.argtypes = [vp, i32, i32, i32, vp, i32, i32, i32, i32, f32, C.POINTER(f32), i32, i32, f32, f32, f32, vp, vp, vp, i32, i32, vp]
    lib.aq_detect_decode_aug.argtypes = [C.POINTER(vp), i32, i32, i32, i32, i32, i32, C.POINTER(f32), C.POINTER(f32), i32, i32, i32, f32, f32,
                                         vp, f32, vp, vp, vp, i32, vp]
    lib.aq_engine_workspace_bytes_augment.argtypes = [vp, i32, i32, i32, C.POINTER(sz)]
    lib.aq_engine_infer_augment.argtypes = lib.aq_engine_infer.argtypes
    lib.aq_engine_forward_raw_augment.argtypes = lib.aq_engine_forward_raw.argtypes
    lib.aq_engine_last_launch_augment.argtypes = [vp, i32, i32, C.POINTER(i32), C.POINTER(i32)]
    _lib = lib
    return lib


def _check(rc: int) -> None:
    if rc != 0:
        raise RuntimeError(f"libaqengine error {rc}: {load_library().aq_last_error().decode()}")


def _stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


def _require_gpu() -> None:
    if not torch.cuda.is_available():
        raise RuntimeError("aquaculture_amd needs a ROCm GPU (MI355X/gfx950); there is no CPU fallback")


def _act_dtype(precision: int) -> torch.dtype:
    return torch.float32 if precision in (AQ_FP32, AQ_F16X3) else torch.bfloat16


class Engine:
    """YOLOv5 tile engine on one GPU.  Owns the C engine (packed weights) and a workspace tensor."""

    def __init__(self, ck: Checkpoint, precision: str = "bf16", device: int = 0, fused_stem: bool = True,
                 fused_bottleneck: Optional[bool] = None, fp8_calibration=None):
        """``fused_bottleneck``: None = on for bf16 engines (the fused kernel is bf16 only), off for fp32 parity engines.
        ``precision="fp8"`` (BASELINE.json configs[3]): a bf16 engine whose wide Bottleneck 3x3 layers run on the fp8 MFMA with e4m3 on
        both operands; the per-tensor activation scales are calibrated on ``fp8_calibration`` (uint8 tiles [B,H,W,3], numpy or CUDA tensor;
        default: synthetic tiles 0-7 at 640 px) -- call ``calibrate_fp8`` again to re-calibrate on other tiles."""
        _require_gpu()
        self.lib = load_library()
        self.ck = ck
        self.precision = ENGINE_PRECISIONS[precision]
        self.precision_name = precision
        self.device = torch.device("cuda", device)
        if fused_bottleneck is None:
            fused_bottleneck = precision in ("bf16", "fp8w", "fp8")
        if fused_bottleneck and precision in ("fp32", "f16x3"):
            raise ValueError("the fused Bottleneck kernel is bf16 only")
        self.plan = _spec.build_plan(ck.variant, ck.nc, ck.na, fused_stem=fused_stem, fused_bottleneck=fused_bottleneck)
        self.no = ck.nc + 5
        packed = pack_plan_weights(ck, self.plan, "fp8" if precision == "fp8w" else "native")
        self._keep = packed   # host arrays must outlive aq_engine_create only, kept for debugging
        tens = (aq_tensor_desc * len(self.plan.tensors))()
        for i, t in enumerate(self.plan.tensors):
            tens[i] = aq_tensor_desc(t.channels, t.down, _DTYPE_CODE[t.dtype])
        ops = (aq_op_desc * len(self.plan.ops))()
        self.plan.flops(640, 640)
        ci = 0
        for i, o in enumerate(self.plan.ops):
            d = aq_op_desc()
            d.kind = o.kind
            for name in ("src", "dst", "res"):
                s = getattr(o, name)
                setattr(d, name, aq_slice(s.tensor, s.ch_off, s.channels) if s is not None else aq_slice(-1, 0, 0))
            d.k, d.stride, d.pad, d.act, d.level = o.k, o.stride, o.pad, o.act, o.level
            d.flops_per_tile = o.flops_per_tile
            if o.kind in (_spec.OP_CONV, _spec.OP_STEM, _spec.OP_BOTTLENECK, _spec.OP_DOWNBLOCK):
                pw = packed[ci]
                ci += 1
                d.weight = pw.weight.ctypes.data_as(C.POINTER(C.c_float))
                d.bias = pw.bias.ctypes.data_as(C.POINTER(C.c_float))
            ops[i] = d
        desc = aq_model_desc()
        desc.precision, desc.nc, desc.na, desc.nl = self.precision, ck.nc, ck.na, 3
        ag = ck.anchor_grid_px().numpy()
        for l in range(3):
            desc.stride[l] = ck.stride[l]
            desc.head_tensor[l] = self.plan.head_tensors[l]
            for a in range(ck.na):
                desc.anchors_px[l][a][0] = float(ag[l, a, 0])
                desc.anchors_px[l][a][1] = float(ag[l, a, 1])
        desc.input_tensor = self.plan.input_tensor
        desc.n_tensors, desc.n_ops = len(self.plan.tensors), len(self.plan.ops)
        desc.tensors, desc.ops = tens, ops
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            _check(self.lib.aq_engine_create(C.byref(desc), device, C.byref(h)))
        self.handle = h
        self._ws: Optional[torch.Tensor] = None
        self._slots: Dict[int, torch.Tensor] = {}     # one workspace per in-flight batch (stream slot)
        self.fp8_scales: Dict[str, float] = {}        # fp8 engines: consumer op name -> e4m3 scale of its input tensor
        if precision == "fp8" and not (isinstance(fp8_calibration, str) and fp8_calibration == "defer"):
            # "defer": the caller calibrates on its own imagery (calibrate_fp8) or installs recorded scales (set_fp8_scales) before the first
            # batch -- yolov5/detect.py does, on tiles sampled from the sweep; until then every pair runs in bf16 (scale 0)
            if fp8_calibration is None:
                from . import tiles as _tiles
                fp8_calibration = _tiles.synthetic_batch(list(range(8)), 640)
            self.calibrate_fp8(fp8_calibration)

    def fp8_pairs(self) -> List[Tuple[int, int]]:
        """(producer op, consumer op) pairs the fp8 path covers: a Bottleneck's cv1 (1x1, direct kernel) feeding its cv2 (3x3 / stride 1,
        planar kernel) with 192 or 384 channels -- yolov5m: the 14 wide Bottleneck layers."""
        pairs = []
        ops = self.plan.ops
        for i, o in enumerate(ops):
            if (i and o.kind == _spec.OP_CONV and o.k == 3 and o.stride == 1 and o.name.endswith(".cv2") and ops[i - 1].name == o.name[:-1] + "1"
                    and ops[i - 1].kind == _spec.OP_CONV and ops[i - 1].k == 1 and o.src.channels == o.dst.channels and o.src.channels in (192, 384)
                    and (ops[i - 1].dst.tensor, ops[i - 1].dst.ch_off) == (o.src.tensor, o.src.ch_off)
                    and self.lib.aq_conv3x3_pl_f8_supported(o.src.channels, o.dst.channels, 1, 8, 8)):
                pairs.append((i - 1, i))
        return pairs

    def calibrate_fp8(self, tiles, margin: float = 1.0) -> Dict[str, float]:
        """One bf16 pass over ``tiles`` (uint8 [B,H,W,3]) records max |t| of every Bottleneck cv1 output; scale = margin x max / 448 (e4m3's
        largest value; the producer saturates beyond it).  Installs the scales (aq_engine_set_fp8_scales) and returns them by consumer name."""
        if not isinstance(tiles, torch.Tensor):
            tiles = torch.from_numpy(np.ascontiguousarray(tiles))
        tiles = tiles.to(self.device).contiguous()
        B, H, W = self._check_tiles(tiles)
        n = len(self.plan.ops)
        zero = (C.c_float * n)()
        _check(self.lib.aq_engine_set_fp8_scales(self.handle, zero, n))         # calibrate on the bf16 path
        ws = self.workspace(B, H, W)
        amax = (C.c_float * n)()
        _check(self.lib.aq_engine_calibrate_amax(self.handle, tiles.data_ptr(), B, H, W, ws.data_ptr(), ws.numel(), amax, n, _stream_ptr()))
        scales = (C.c_float * n)()
        self.fp8_scales = {}
        for prod, cons in self.fp8_pairs():
            a = float(amax[prod])
            if a > 0.0 and np.isfinite(a):
                scales[cons] = margin * a / 448.0
                self.fp8_scales[self.plan.ops[cons].name] = float(scales[cons])
        _check(self.lib.aq_engine_set_fp8_scales(self.handle, scales, n))
        return dict(self.fp8_scales)

    def set_fp8_scales(self, by_name: Dict[str, float]) -> None:
        """Installs e4m3 activation scales recorded elsewhere (consumer op name -> scale, as calibrate_fp8 returns them): the other ranks of a
        sweep take rank 0's, a resumed sweep takes the interrupted run's, so that every tile is quantised with the same scales."""
        n = len(self.plan.ops)
        scales = (C.c_float * n)()
        names = {self.plan.ops[cons].name: cons for _, cons in self.fp8_pairs()}
        unknown = sorted(set(by_name) - set(names))
        if unknown:
            raise ValueError(f"fp8 scales for ops this engine does not run in fp8: {unknown}")
        for name, v in by_name.items():
            if not (np.isfinite(v) and v > 0.0):
                raise ValueError(f"fp8 scale of {name} must be positive and finite, got {v}")
            scales[names[name]] = float(v)
        _check(self.lib.aq_engine_set_fp8_scales(self.handle, scales, n))
        self.fp8_scales = {k: float(v) for k, v in by_name.items()}

    def close(self) -> None:
        if getattr(self, "handle", None):
            self.lib.aq_engine_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- workspace ----
    def workspace(self, B: int, H: int, W: int, slot: int = 0, augment: bool = False) -> torch.Tensor:
        """Workspace of in-flight batch ``slot``: batches issued on different streams must not share one."""
        n = self.workspace_bytes(B, H, W, augment)
        ws = self._slots.get(slot)
        if ws is None or ws.numel() < n:
            self._slots.pop(slot, None)
            ws = self._slots[slot] = torch.empty(n, dtype=torch.uint8, device=self.device)
        self._ws = ws
        return ws

    def workspace_bytes(self, B: int, H: int, W: int, augment: bool = False, save_img: Optional[Tuple[int, int]] = None,
                        blank_key: Optional[Tuple[int, int]] = None) -> int:
        """Workspace bytes for batches up to ``B`` of H x W tiles, allocating nothing.  A batch some op of the plan cannot run raises
        RuntimeError naming the op (plan index and name) and the largest batch that fits.  save_img = (h0, w0): plus what writing annotated
        images of that original size takes per pipeline slot (image_save_bytes).  blank_key = (h0, w0): plus what --blank-key holds per
        pipeline slot for images of that original size (blank_key_bytes)."""
        if blank_key is not None:
            return self.workspace_bytes(B, H, W, augment, save_img) + blank_key_bytes(B, *blank_key)
        if save_img is not None:
            return self.workspace_bytes(B, H, W, augment) + image_save_bytes(B, *save_img)
        n = C.c_size_t()
        try:
            _check((self.lib.aq_engine_workspace_bytes_augment if augment else self.lib.aq_engine_workspace_bytes)(self.handle, B, H, W, C.byref(n)))
        except RuntimeError as err:
            m = re.search(r"plan op (\d+)", str(err))
            if m is None:
                raise
            i = int(m.group(1))
            raise RuntimeError(str(err).replace(m.group(0), f"{m.group(0)} ({self.plan.ops[i].name})", 1)) from None
        return n.value

    def num_candidates(self, H: int, W: int, augment: bool = False) -> int:
        """Rows per image of the prediction: one pass, or the three clipped passes of --augment (augment.geometry)."""
        if augment:
            from . import augment as _aug
            return _aug.geometry(H, W, self.ck.na)[1]
        return _spec.num_candidates(H, W, self.ck.na)

    @staticmethod
    def _check_tiles(tiles: torch.Tensor) -> Tuple[int, int, int]:
        if tiles.dtype != torch.uint8 or tiles.dim() != 4 or tiles.shape[3] != 3 or not tiles.is_cuda or not tiles.is_contiguous():
            raise ValueError("tiles must be a contiguous CUDA uint8 tensor [B, H, W, 3] (RGB)")
        return int(tiles.shape[0]), int(tiles.shape[1]), int(tiles.shape[2])

    # ---- S1 + S2 ----
    def infer(self, tiles: torch.Tensor, conf_thres: float = 0.25, iou_thres: float = 0.45, max_det: int = 1000,
              out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, slot: int = 0, augment: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
        """uint8 [B,H,W,3] -> (dets float32 [B,max_det,6] = x1,y1,x2,y2,conf,cls ; counts int32 [B]).
        Work is enqueued on torch's current stream; ``slot`` selects the workspace (use one slot per stream when
        several batches are in flight).  ``augment``: upstream's test-time augmentation (three passes, one NMS; augment.py)."""
        B, H, W = self._check_tiles(tiles)
        ws = self.workspace(B, H, W, slot, augment)
        if out is None:
            dets = torch.empty((B, max_det, 6), dtype=torch.float32, device=self.device)
            counts = torch.empty((B,), dtype=torch.int32, device=self.device)
        else:
            dets, counts = out
        fn = self.lib.aq_engine_infer_augment if augment else self.lib.aq_engine_infer
        _check(fn(self.handle, tiles.data_ptr(), B, H, W, ws.data_ptr(), ws.numel(),
                  dets.data_ptr(), counts.data_ptr(), conf_thres, iou_thres, max_det, _stream_ptr()))
        return dets, counts

    def run_ops(self, tiles: torch.Tensor, first: int, last: int, conf_thres: float = 0.25, iou_thres: float = 0.45, max_det: int = 1000,
                out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, slot: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
        """Plan ops [first, last) of ``infer`` on the same arguments (tests only: layer-by-layer checks of the path ``infer`` takes).
        Stepping through the plan in order on one workspace slot and stream launches exactly what one ``infer`` call launches; ``out``
        holds the detections and counts once the last op (NMS) has run.  Between calls, ``tensor`` views the ops' inputs and outputs."""
        B, H, W = self._check_tiles(tiles)
        ws = self.workspace(B, H, W, slot)
        if out is None:
            dets = torch.empty((B, max_det, 6), dtype=torch.float32, device=self.device)
            counts = torch.empty((B,), dtype=torch.int32, device=self.device)
        else:
            dets, counts = out
        _check(self.lib.aq_engine_run_ops(self.handle, tiles.data_ptr(), B, H, W, ws.data_ptr(), ws.numel(), first, last,
                                          conf_thres, iou_thres, max_det, dets.data_ptr(), counts.data_ptr(), _stream_ptr()))
        return dets, counts

    # ---- S1 ----
    def forward_raw(self, tiles: torch.Tensor, augment: bool = False) -> torch.Tensor:
        """uint8 [B,H,W,3] -> pred float32 [B, N, 5+nc] (what Detect.forward returns at inference).  ``augment``: what
        ``model(im, augment=True)`` returns -- the three passes de-scaled, clipped and concatenated, [B, N_aug, 5+nc]."""
        B, H, W = self._check_tiles(tiles)
        ws = self.workspace(B, H, W, augment=augment)
        pred = torch.empty((B, self.num_candidates(H, W, augment), self.no), dtype=torch.float32, device=self.device)
        fn = self.lib.aq_engine_forward_raw_augment if augment else self.lib.aq_engine_forward_raw
        _check(fn(self.handle, tiles.data_ptr(), B, H, W, ws.data_ptr(), ws.numel(), pred.data_ptr(), _stream_ptr()))
        return pred

    # ---- S2 ----
    def nms(self, pred: torch.Tensor, conf_thres=0.25, iou_thres=0.45, max_det=1000) -> Tuple[torch.Tensor, torch.Tensor]:
        return nms(pred, self.ck.nc, conf_thres, iou_thres, max_det)

    def set_nms_options(self, agnostic: bool = False, classes: Optional[Sequence[int]] = None) -> None:
        """detect.py's --agnostic-nms / --classes for the NMS step of infer() [UPSTREAM non_max_suppression(classes, agnostic)]."""
        lo, hi = class_mask(classes, self.ck.nc)
        _check(self.lib.aq_engine_set_nms_options(self.handle, int(bool(agnostic)), lo, hi))

    # ---- test / tuning hooks ----
    def tensor(self, tensor_id: int, B: int) -> torch.Tensor:
        """View of plan tensor ``tensor_id`` ([B,h,w,C]) inside the workspace after a call (tests only)."""
        p, c, h, w, eb = C.c_void_p(), C.c_int(), C.c_int(), C.c_int(), C.c_int()
        _check(self.lib.aq_engine_tensor_ptr(self.handle, tensor_id, C.byref(p), C.byref(c), C.byref(h), C.byref(w), C.byref(eb)))
        off = p.value - self._ws.data_ptr()
        nbytes = B * h.value * w.value * c.value * eb.value
        dt = {1: torch.uint8, 2: torch.bfloat16, 4: torch.float32}[eb.value]
        return self._ws[off:off + nbytes].view(dt).view(B, h.value, w.value, c.value)

    def candidates(self, B: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """Views of the candidate list the NMS step reads, inside the workspace after a call (tests only): (cand int32 [B, N] candidate
        indices, rows float32 [B, N, 5 + nc] decoded rows in the same order, counts int32 [B]); entries past counts[b] are unspecified."""
        c, r, n, cap = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int()
        _check(self.lib.aq_engine_candidates(self.handle, C.byref(c), C.byref(r), C.byref(n), C.byref(cap)))
        base, N = self._ws.data_ptr(), cap.value

        def view(p, nbytes, dt, shape):
            return self._ws[p - base:p - base + nbytes].view(dt).view(*shape)
        return (view(c.value, B * N * 4, torch.int32, (B, N)), view(r.value, B * N * self.no * 4, torch.float32, (B, N, self.no)),
                view(n.value, B * 4, torch.int32, (B,)))

    def tensor_by_name(self, name: str, B: int) -> torch.Tensor:
        ids = [i for i, t in enumerate(self.plan.tensors) if t.name == name]
        return self.tensor(ids[0], B)

    def set_conv_config(self, op: int, cfg: int) -> None:
        _check(self.lib.aq_engine_set_conv_config(self.handle, op, cfg))

    def set_tuned_table(self, B: int, H: int, W: int, cfgs) -> None:
        """Install an autotune result (from a cache file or another rank) for batches of exactly this geometry."""
        arr = (C.c_int * len(cfgs))(*[int(c) for c in cfgs])
        _check(self.lib.aq_engine_set_tuned_table(self.handle, B, H, W, arr, len(cfgs)))

    def tune_key(self, B: int, H: int, W: int) -> str:
        """Key of a tuned table: model, precision, geometry, library version + candidate count + plan shape (new kernels invalidate old
        tables), and the environment switches that remove kernels from the candidate set (such a run has a table of its own)."""
        key = (f"{self.ck.variant}:nc{self.ck.nc}:p{self.precision_name}:{B}x{H}x{W}:n{self.lib.aq_conv_num_configs()}"
               f":v{self.lib.aq_version()}:ops{len(self.plan.ops)}")
        off = ",".join(sorted(f"{k}={v}" for k, v in os.environ.items() if k.startswith("AQ_DISABLE_") or k in ("AQ_PL_W8", "AQ_PL_ASM", "AQ_PL_NB", "AQ_C1_ASM", "AQ_C1_ASM_NB")))
        return key + (":" + off if off else "")

    def autotune(self, tiles: torch.Tensor, reps: int = 3, cache: Optional[str] = None, shipped: bool = True, augment: bool = False):
        """Pick the fastest tile configuration per conv op for this batch geometry (synchronises).
        ``cache``: optional JSON file; a stored table for the same model/precision/geometry is applied
        instead of re-timing (used to keep tuning launches out of rocprof traces).
        ``shipped``: on a cache miss look in the table that ships in-tree (aquaculture_amd/data/tuned_tables.json: the geometries of
        BASELINE.json's configs, timed on MI355X with this library version) before timing anything -- two runs of the same build then
        launch the same kernels and write the same bf16 label bytes (the timing sweep's picks between near-equal shapes flip from run to
        run); ``shipped=False`` (bench.py --retune, AQ_RETUNE=1) times regardless.
        ``augment``: tune (or install from the caches) the tables of all three geometries an augmented call runs at -- each pass uses the
        table of its own network input; returns [((B, Hp, Wp), cfgs)] per pass.  The scaled passes are timed on the tiles' top-left Hp x Wp
        corner (the kernels' speed does not depend on the pixel values)."""
        import json
        B, H, W = self._check_tiles(tiles)
        if augment:
            from . import augment as _aug
            out = []
            for ps in reversed(_aug.geometry(H, W, self.ck.na)[0]):     # (the plain geometry last: get_conv_config reports its table)
                t = tiles if (ps.hp, ps.wp) == (H, W) else tiles[:, :ps.hp, :ps.wp].contiguous()
                out.append(((B, ps.hp, ps.wp), self.autotune(t, reps, cache, shipped)))
            return out[::-1]
        key = self.tune_key(B, H, W)
        table = {}
        if cache and os.path.exists(cache):
            try:
                with open(cache) as f:
                    table = json.load(f)
            except (OSError, ValueError):      # unreadable or half-written by another rank: tune again
                table = {}
            if key in table and len(table[key]) == len(self.plan.ops):
                try:
                    self.set_tuned_table(B, H, W, table[key])
                    return list(table[key])
                except RuntimeError:           # an entry this build / environment has no kernel for: tune again, replace the entry
                    pass
        if shipped and os.environ.get("AQ_RETUNE") != "1":
            try:
                with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "tuned_tables.json")) as f:
                    ship = json.load(f)
                if key in ship and len(ship[key]) == len(self.plan.ops):
                    self.set_tuned_table(B, H, W, ship[key])
                    self.tuned_from = "shipped table"
                    return list(ship[key])
            except (OSError, ValueError, RuntimeError):
                pass
        self.tuned_from = "timed in this run"
        ws = self.workspace(B, H, W)
        _check(self.lib.aq_engine_autotune(self.handle, tiles.data_ptr(), B, H, W, ws.data_ptr(), ws.numel(), reps, _stream_ptr()))
        cfgs = [self.lib.aq_engine_get_conv_config(self.handle, i) for i in range(len(self.plan.ops))]
        if cache:
            table[key] = cfgs
            os.makedirs(os.path.dirname(os.path.abspath(cache)), exist_ok=True)
            tmp = f"{cache}.{os.getpid()}.tmp"     # ranks of one job may share the file: replace it atomically
            with open(tmp, "w") as f:
                json.dump(table, f)
            os.replace(tmp, cache)
        return cfgs

    FAMILIES = {0: "none", 1: "igemm_or_halo", 2: "pl3x3", 3: "pl3x3_w8", 4: "pl3x3s2", 5: "pl3x3_f8", 6: "direct1x1", 7: "direct1x1_f8out",
                8: "direct3x3s2", 9: "bottleneck", 10: "downblock", 11: "stem", 12: "head_decode", 13: "asm1x1"}

    def last_launches(self, augment_pass: Optional[int] = None) -> List[Tuple[str, int]]:
        """(kernel family, tile-configuration id) of every op's most recent launch (aq_engine_last_launch) -- what actually ran, as opposed
        to what the tuned table asked for.  ``augment_pass`` (0..2): the records of that pass of the last augmented call."""
        out = []
        fam, cfg = C.c_int(), C.c_int()
        for i in range(len(self.plan.ops)):
            if augment_pass is None:
                _check(self.lib.aq_engine_last_launch(self.handle, i, C.byref(fam), C.byref(cfg)))
            else:
                _check(self.lib.aq_engine_last_launch_augment(self.handle, augment_pass, i, C.byref(fam), C.byref(cfg)))
            out.append((self.FAMILIES.get(fam.value, str(fam.value)), cfg.value))
        return out

    def profile(self, enable: bool, ring: int = 32) -> None:
        _check(self.lib.aq_engine_profile(self.handle, int(enable), ring))

    def op_times_ms(self) -> Tuple[np.ndarray, int]:
        n = len(self.plan.ops)
        buf = (C.c_float * n)()
        calls = C.c_int()
        _check(self.lib.aq_engine_op_times(self.handle, buf, n, C.byref(calls)))
        return np.array(buf[:], dtype=np.float64), calls.value


# --------------------------------------------------------------------------------------
# individual kernels (used by the parity tests; same C entry points the engine uses)
# --------------------------------------------------------------------------------------
def class_mask(classes: Optional[Sequence[int]], nc: int) -> Tuple[int, int]:
    """--classes as the two 64-bit words aq_nms_opts takes (None = every class)."""
    if classes is None:
        return (1 << 64) - 1, (1 << 64) - 1
    m = 0
    for c in classes:
        if not 0 <= int(c) < min(nc, 128):
            raise ValueError(f"--classes {c}: the model has classes 0 .. {nc - 1}")
        m |= 1 << int(c)
    return m & ((1 << 64) - 1), m >> 64


def nms(pred: torch.Tensor, nc: int, conf_thres=0.25, iou_thres=0.45, max_det=1000, agnostic: bool = False,
        classes: Optional[Sequence[int]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """non_max_suppression(pred, conf, iou, classes, agnostic, multi_label=False, max_det) on device."""
    _require_gpu()
    lib = load_library()
    if pred.dtype != torch.float32 or pred.dim() != 3 or not pred.is_cuda or not pred.is_contiguous():
        raise ValueError("pred must be a contiguous CUDA float32 tensor [B, N, 5+nc]")
    B, N, no = pred.shape
    if no != nc + 5:
        raise ValueError(f"pred last dim {no} != nc + 5 = {nc + 5}")
    scratch = torch.empty(lib.aq_nms_scratch_bytes(B, N), dtype=torch.uint8, device=pred.device)
    dets = torch.empty((B, max_det, 6), dtype=torch.float32, device=pred.device)
    counts = torch.empty((B,), dtype=torch.int32, device=pred.device)
    lo, hi = class_mask(classes, nc)
    _check(lib.aq_nms_opts(pred.data_ptr(), N, B, N, nc, conf_thres, iou_thres, max_det, None, None, 0,
                           scratch.data_ptr(), dets.data_ptr(), counts.data_ptr(), int(bool(agnostic)), lo, hi, _stream_ptr()))
    return dets, counts


_zero_pages: Dict[int, torch.Tensor] = {}


def _zero_page(device) -> torch.Tensor:
    key = device.index or 0
    if key not in _zero_pages:
        _zero_pages[key] = torch.zeros(4096, dtype=torch.uint8, device=device)
    return _zero_pages[key]


def pack_conv_weights(w_oihw: torch.Tensor, precision: str, device) -> torch.Tensor:
    """fp32 (Cout,Cin,k,k) -> packed device buffer the conv kernels read."""
    lib = load_library()
    prec = PRECISIONS[precision]
    w = np.ascontiguousarray(w_oihw.permute(0, 2, 3, 1).float().cpu().numpy())
    cout, k, _, cin = w.shape
    n = C.c_size_t()
    wp = w.ctypes.data_as(C.POINTER(C.c_float))
    _check(lib.aq_pack_conv_weights(wp, cout, k, cin, prec, None, C.byref(n), None))
    buf = torch.empty(n.value, dtype=torch.uint8, device=device)
    _check(lib.aq_pack_conv_weights(wp, cout, k, cin, prec, buf.data_ptr(), C.byref(n), _stream_ptr()))
    return buf


def conv2d_nhwc(x: torch.Tensor, w_oihw: torch.Tensor, bias: torch.Tensor, stride=1, pad=None, act=True,
                residual: Optional[torch.Tensor] = None, precision="bf16", out_f32=False,
                cfg: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = (residual +) SiLU(conv(x, w) + b) on NHWC tensors through aq_conv2d (tests).  ``x``, ``residual`` and ``out`` may be channel
    slices (starting on a multiple of 8 channels) of wider dense NHWC tensors."""
    _require_gpu()
    lib = load_library()
    prec = PRECISIONS[precision]

    def pixel_stride(t, h, w):
        assert t.is_cuda and t.stride(3) == 1 and t.stride(1) == w * t.stride(2) and t.stride(0) == h * w * t.stride(2), \
            "a channel slice of a dense NHWC tensor is needed"
        return t.stride(2)

    assert x.dtype == _act_dtype(prec)
    B, H, W, cin = x.shape
    in_ld = pixel_stride(x, H, W)
    cout, _, k, _ = w_oihw.shape
    pad = k // 2 if pad is None else pad
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    if prec == AQ_F16X3:          # split mode: the packer writes the weights' fp16 halves and the bias / scale buffer the kernel reads
        wk = np.ascontiguousarray(w_oihw.permute(0, 2, 3, 1).float().cpu().numpy())
        bh = np.ascontiguousarray(bias.float().cpu().numpy())
        n, nb = C.c_size_t(), C.c_size_t()
        wp_, bp_ = wk.ctypes.data_as(C.POINTER(C.c_float)), bh.ctypes.data_as(C.POINTER(C.c_float))
        _check(lib.aq_pack_conv_weights_x3(wp_, bp_, cout, k, cin, None, C.byref(n), None, C.byref(nb), None))
        wbuf = torch.empty(n.value, dtype=torch.uint8, device=x.device)
        bbuf = torch.empty(nb.value, dtype=torch.float32, device=x.device)
        _check(lib.aq_pack_conv_weights_x3(wp_, bp_, cout, k, cin, wbuf.data_ptr(), C.byref(n), bbuf.data_ptr(), C.byref(nb), _stream_ptr()))
    else:
        wbuf = pack_conv_weights(w_oihw, precision, x.device)
        bbuf = torch.zeros(cout + 512, dtype=torch.float32, device=x.device)
        bbuf[:cout] = bias.float().to(x.device)
    odt = torch.float32 if (out_f32 or prec in (AQ_FP32, AQ_F16X3)) else torch.bfloat16
    if out is None:
        out = torch.empty((B, Ho, Wo, cout), dtype=odt, device=x.device)
    assert out.dtype == odt and tuple(out.shape) == (B, Ho, Wo, cout)
    out_ld = pixel_stride(out, Ho, Wo)
    res_ptr, res_ld = None, cout
    if residual is not None:
        assert residual.dtype == x.dtype and tuple(residual.shape) == (B, Ho, Wo, cout)
        res_ptr, res_ld = residual.data_ptr(), pixel_stride(residual, Ho, Wo)
    old = os.environ.get("AQ_CONV_CFG")
    if cfg is not None:
        os.environ["AQ_CONV_CFG"] = str(cfg)
    try:
        _check(lib.aq_conv2d(x.data_ptr(), in_ld, 0, cin, out.data_ptr(), out_ld, 0, cout, res_ptr, res_ld, 0,
                             wbuf.data_ptr(), bbuf.data_ptr(), B, H, W, k, stride, pad, int(act), prec, int(out_f32),
                             _zero_page(x.device).data_ptr(), _stream_ptr()))
    finally:
        if cfg is not None:
            if old is None:
                os.environ.pop("AQ_CONV_CFG", None)
            else:
                os.environ["AQ_CONV_CFG"] = old
    torch.cuda.current_stream().synchronize()   # wbuf/bbuf are freed on return
    return out


_lb_tables: Dict[Tuple, Tuple[torch.Tensor, torch.Tensor, Tuple[int, int, int, int, int, int]]] = {}


def letterbox_device(tiles0: torch.Tensor, new_shape=(640, 640), stride: int = 32, auto: bool = True) -> torch.Tensor:
    """uint8 CUDA [B,H0,W0,3] original tiles -> letterboxed uint8 [B,H,W,3] on the device (aq_letterbox_u8).
    Geometry and coefficient tables come from dataloader.letterbox_geometry / resize tables (host, cached per shape)."""
    from . import dataloader
    _require_gpu()
    lib = load_library()
    assert tiles0.is_cuda and tiles0.dtype == torch.uint8 and tiles0.dim() == 4 and tiles0.shape[3] == 3 and tiles0.is_contiguous()
    B, H0, W0, _ = tiles0.shape
    key = (H0, W0, tuple(new_shape), stride, auto, tiles0.device.index)
    if key not in _lb_tables:
        (nw, nh), (top, bottom, left, right) = dataloader.letterbox_geometry((H0, W0), new_shape, auto, True, stride)
        xt = np.stack(dataloader._axis_coeffs(W0, nw), 1).astype(np.int32)
        yt = np.stack(dataloader._axis_coeffs(H0, nh), 1).astype(np.int32)
        _lb_tables[key] = (torch.from_numpy(xt).to(tiles0.device), torch.from_numpy(yt).to(tiles0.device),
                           (nw, nh, top, left, nh + top + bottom, nw + left + right))
    xt, yt, (nw, nh, top, left, H, W) = _lb_tables[key]
    out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=tiles0.device)
    _check(lib.aq_letterbox_u8(tiles0.data_ptr(), B, H0, W0, out.data_ptr(), H, W, nw, nh, top, left,
                               xt.data_ptr(), yt.data_ptr(), _stream_ptr()))
    return out


def _letterbox_tables(H0: int, W0: int, new_shape, stride: int, auto: bool, device):
    from . import dataloader
    key = (H0, W0, tuple(new_shape), stride, auto, device.index)
    if key not in _lb_tables:
        (nw, nh), (top, bottom, left, right) = dataloader.letterbox_geometry((H0, W0), new_shape, auto, True, stride)
        xt = np.stack(dataloader._axis_coeffs(W0, nw), 1).astype(np.int32)
        yt = np.stack(dataloader._axis_coeffs(H0, nh), 1).astype(np.int32)
        _lb_tables[key] = (torch.from_numpy(xt).to(device), torch.from_numpy(yt).to(device),
                           (nw, nh, top, left, nh + top + bottom, nw + left + right))
    return _lb_tables[key]


def letterbox_scene_tiles(scene: torch.Tensor, origins, tile_hw, new_shape=(640, 640), stride: int = 32, auto: bool = True) -> torch.Tensor:
    """uint8 CUDA scene raster [Hs,Ws,3] + tile origins [(x0, y0), ...] of equal size tile_hw=(H0,W0) -> letterboxed uint8 [B,H,W,3]
    (aq_letterbox_tiles_u8): crop (reference src/load_data/tile_tifs.py:33-47) and letterbox in one pass, no tile copies."""
    _require_gpu()
    lib = load_library()
    assert scene.is_cuda and scene.dtype == torch.uint8 and scene.dim() == 3 and scene.shape[2] == 3 and scene.is_contiguous()
    Hs, Ws, _ = scene.shape
    H0, W0 = tile_hw
    row_b = Ws * 3
    offs = np.asarray([y0 * row_b + x0 * 3 for x0, y0 in origins], dtype=np.int64)
    B = int(offs.shape[0])
    xt, yt, (nw, nh, top, left, H, W) = _letterbox_tables(H0, W0, new_shape, stride, auto, scene.device)
    offs_dev = torch.from_numpy(offs).to(scene.device)
    out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=scene.device)
    _check(lib.aq_letterbox_tiles_u8(scene.data_ptr(), Hs * row_b, row_b, offs_dev.data_ptr(), offs.ctypes.data, B, H0, W0, out.data_ptr(),
                                     H, W, nw, nh, top, left, xt.data_ptr(), yt.data_ptr(), _stream_ptr()))
    return out


def format_label_rows(rows: np.ndarray, save_conf: bool = True) -> bytes:
    """rows float32 [n,6] (cls xc yc w h conf) -> label-file bytes via the C formatter (releases the GIL)."""
    lib = load_library()
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    n = rows.shape[0]
    if n == 0:
        return b""
    buf = C.create_string_buffer(n * 6 * 16)
    k = lib.aq_format_label_rows(rows.ctypes.data_as(C.POINTER(C.c_float)), n, int(save_conf), buf, len(buf))
    if k < 0:
        buf = C.create_string_buffer(-k + 1)
        k = lib.aq_format_label_rows(rows.ctypes.data_as(C.POINTER(C.c_float)), n, int(save_conf), buf, len(buf))
    return buf.raw[:k]


def write_label_files(labels_dir: str, stems, rows: np.ndarray, offsets: np.ndarray, save_conf: bool = True, fsync: bool = False) -> int:
    """One C call per batch (aq_write_label_files; releases the GIL for formatting and file system calls): tile t's rows are
    rows[offsets[t]:offsets[t + 1]] (float32 [N, 6], file order); returns the number of label files written (tiles without rows get none)."""
    lib = load_library()
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    n = len(stems)
    assert offsets.shape[0] == n + 1 and (rows.shape[0] == 0 or rows.shape[1] == 6)
    arr = (C.c_char_p * n)(*[os.fsencode(s_) for s_ in stems])
    k = lib.aq_write_label_files(os.fsencode(labels_dir), arr, rows.ctypes.data_as(C.POINTER(C.c_float)), offsets.ctypes.data_as(C.POINTER(C.c_longlong)), n,
                                 int(save_conf), int(fsync))
    if k < 0:
        raise OSError(f"could not write the label file of {stems[-1 - k]} in {labels_dir}")
    return int(k)


# aq_crop (include/aq_engine.h): one crop of a uint8 RGB device image -- pixel (x, y) at base + y * pitch + 3 x, window [x1, x2) x [y1, y2),
# first block position in the coefficient arena
CROP_DTYPE = np.dtype([("base", "<i8"), ("pitch", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("x2", "<i4"), ("y2", "<i4"), ("block", "<i4")])
CROP_ARENA_BLOCKS = 1 << 16        # block positions (384 bytes each) per encode piece: 25 MB of device arena and as much pinned


def crop_blocks(table: np.ndarray) -> np.ndarray:
    """Block positions (8 x 8 pixels, three components) of each crop of a CROP_DTYPE table."""
    return ((table["x2"].astype(np.int64) - table["x1"] + 7) // 8) * ((table["y2"].astype(np.int64) - table["y1"] + 7) // 8)


def crop_table(bases, pitch, rects) -> np.ndarray:
    """CROP_DTYPE table of n crops: bases int64 [n] (byte offset of each crop's image), pitch (row bytes; scalar or [n]), rects int [n, 4]
    (x1, y1, x2, y2); the crops' block positions follow each other from 0."""
    rects = np.asarray(rects, dtype=np.int64).reshape(-1, 4)
    t = np.zeros(rects.shape[0], CROP_DTYPE)
    t["base"], t["pitch"] = bases, pitch
    t["x1"], t["y1"], t["x2"], t["y2"] = rects.T
    nb = crop_blocks(t)
    if nb.sum() >= 1 << 31:
        raise ValueError("crop table: more than 2^31 block positions in one call")
    t["block"][1:] = np.cumsum(nb)[:-1]
    return t


def encode_crops(images_dev: torch.Tensor, table: np.ndarray, arena_blocks: int = CROP_ARENA_BLOCKS, arena: Optional[torch.Tensor] = None,
                 arena_host: Optional[torch.Tensor] = None) -> Tuple[np.ndarray, np.ndarray]:
    """The device half of --save-crop (aq_crop_jpeg_coefs) on the current stream: images_dev = the uint8 CUDA buffer the table's byte offsets
    point into, table = crop_table(...).  The crops go through an arena of `arena_blocks` block positions in pieces (a crop never straddles
    two); after each piece only its used part comes back through the pinned arena.  `arena` (int16 CUDA) / `arena_host` (int16 pinned),
    at least arena_blocks x 192 values each, are reused when given.  Returns (coefficients int16 [positions, 192] in host memory, table)."""
    _require_gpu()
    lib = load_library()
    assert images_dev.is_cuda and images_dev.dtype == torch.uint8 and images_dev.is_contiguous()
    table = np.ascontiguousarray(table, dtype=CROP_DTYPE)
    n = table.shape[0]
    nb = crop_blocks(table)
    if n == 0:
        return np.zeros((0, 192), np.int16), table
    ends = table["block"].astype(np.int64) + nb
    if table["block"][0] != 0 or np.any(table["block"][1:] != ends[:-1]):
        raise ValueError("crop table: block positions must follow each other from 0 (crop_table)")
    w, h = table["x2"] - table["x1"], table["y2"] - table["y1"]
    last = table["base"] + (table["y2"].astype(np.int64) - 1) * table["pitch"] + 3 * table["x2"].astype(np.int64)
    bad = (w <= 0) | (h <= 0) | (w > 65535) | (h > 65535) | (table["x1"] < 0) | (table["y1"] < 0) | (table["base"] < 0) | \
          (table["pitch"] < 3 * table["x2"].astype(np.int64)) | (last > images_dev.numel())
    if bad.any():
        i = int(np.nonzero(bad)[0][0])
        raise ValueError(f"crop {i} {table[i]} is empty or leaves its image ({images_dev.numel()} bytes)")
    if int(nb.max()) > arena_blocks:
        raise ValueError(f"a crop of {int(nb.max())} block positions does not fit an arena of {arena_blocks}")
    if arena is None or arena.numel() < arena_blocks * 192:
        arena = torch.empty(arena_blocks * 192, dtype=torch.int16, device=images_dev.device)
    if arena_host is None or arena_host.numel() < arena_blocks * 192:
        arena_host = torch.empty(arena_blocks * 192, dtype=torch.int16, pin_memory=True)
    table_dev = torch.from_numpy(table.view(np.uint8)).to(images_dev.device, non_blocking=False)
    out = np.empty((int(ends[-1]), 192), np.int16)
    stream = torch.cuda.current_stream()
    c0 = 0
    while c0 < n:
        p0 = int(table["block"][c0])
        c1 = int(np.searchsorted(ends, p0 + arena_blocks, side="right"))
        used = int(ends[c1 - 1]) - p0
        _check(lib.aq_crop_jpeg_coefs(images_dev.data_ptr(), images_dev.numel(), table_dev.data_ptr() + c0 * CROP_DTYPE.itemsize, c1 - c0, used,
                                      arena.data_ptr(), stream.cuda_stream))
        arena_host[:used * 192].copy_(arena[:used * 192], non_blocking=True)
        stream.synchronize()
        out[p0:p0 + used] = arena_host[:used * 192].numpy().reshape(used, 192)
        c0 = c1
    return out, table


def crop_jpeg_bytes(coef: np.ndarray, w: int, h: int) -> bytes:
    """The JPEG file of one w x h crop from its coefficient positions (aq_crop_jpeg_bytes; int16 [ceil(w/8) ceil(h/8), 192])."""
    lib = load_library()
    nblk = ((w + 7) // 8) * ((h + 7) // 8)
    coef = np.ascontiguousarray(coef.reshape(-1)[:nblk * 192], dtype=np.int16)
    assert coef.size == nblk * 192
    buf = C.create_string_buffer(1024 + nblk * 192)
    k = lib.aq_crop_jpeg_bytes(coef.ctypes.data, int(w), int(h), buf, len(buf))
    if k < 0:
        buf = C.create_string_buffer(-k)
        k = lib.aq_crop_jpeg_bytes(coef.ctypes.data, int(w), int(h), buf, len(buf))
    if k <= 0:
        raise ValueError(f"crop_jpeg_bytes: bad crop size {w} x {h}")
    return buf.raw[:k]


def write_crop_files(root_dir: str, rel_paths, coef: np.ndarray, table: np.ndarray, threads: int = 4, fsync: bool = False) -> int:
    """One C call per batch (aq_write_crop_files; no interpreter lock held): crop i of `table`, coefficients from position table[i]["block"] of
    `coef` (encode_crops), -> <root_dir>/<rel_paths[i]> on `threads` threads, directories created on the way.  Returns the number of files."""
    lib = load_library()
    table = np.ascontiguousarray(table, dtype=CROP_DTYPE)
    coef = np.ascontiguousarray(coef, dtype=np.int16)
    n = table.shape[0]
    assert len(rel_paths) == n and (n == 0 or coef.shape[0] >= int((table["block"].astype(np.int64) + crop_blocks(table)).max()))
    if n == 0:
        return 0
    arr = (C.c_char_p * n)(*[os.fsencode(p_) for p_ in rel_paths])
    k = lib.aq_write_crop_files(os.fsencode(root_dir), arr, coef.ctypes.data, table.ctypes.data, n, int(threads), int(fsync))
    if k < 0:
        raise OSError(f"could not write the crop {rel_paths[-1 - k]} in {root_dir}")
    return int(k)


# ---- annotated images: aq_annotate_u8 (boxes and labels) and the whole-frame 4:2:0 encoder ----

# aq_frame / aq_canvas / aq_prim (include/aq_engine.h)
FRAME_DTYPE = np.dtype([("base", "<i8"), ("pitch", "<i4"), ("w", "<i4"), ("h", "<i4"), ("mcu", "<i4")])
CANVAS_DTYPE = np.dtype([("src", "<i8"), ("dst", "<i8"), ("src_pitch", "<i4"), ("dst_pitch", "<i4"), ("w", "<i4"), ("h", "<i4"), ("cell", "<i4"), ("unit", "<i4")])
PRIM_DTYPE = np.dtype([("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("rgb", "<u4"), ("mask_w", "<i4"), ("mask", "<i8")])
FRAME_ARENA_MCUS = 1 << 15         # 16 x 16 MCUs (768 bytes each) per encode piece: 25 MB of device arena and as much pinned (eight 1024-px frames)


def frame_mcus(table: np.ndarray) -> np.ndarray:
    """MCUs (16 x 16 pixels: four Y blocks, Cb, Cr) of each frame of a FRAME_DTYPE table."""
    return ((table["w"].astype(np.int64) + 15) // 16) * ((table["h"].astype(np.int64) + 15) // 16)


def frame_table(bases, pitch, sizes) -> np.ndarray:
    """FRAME_DTYPE table of n frames: bases int64 [n] (byte offset of each image), pitch (row bytes; scalar or [n]), sizes int [n, 2] (h, w);
    the frames' MCUs follow each other from 0."""
    sizes = np.asarray(sizes, dtype=np.int64).reshape(-1, 2)
    t = np.zeros(sizes.shape[0], FRAME_DTYPE)
    t["base"], t["pitch"] = bases, pitch
    t["h"], t["w"] = sizes.T
    nm = frame_mcus(t)
    if nm.sum() >= 1 << 31:
        raise ValueError("frame table: more than 2^31 MCUs in one call")
    t["mcu"][1:] = np.cumsum(nm)[:-1]
    return t


def image_save_bytes(B: int, h0: int, w0: int, arena_mcus: int = FRAME_ARENA_MCUS) -> int:
    """Device bytes one pipeline slot holds for writing the annotated images of batches of B images of h0 x w0: the annotated copies and the
    coefficient arena (as much again is pinned on the host)."""
    per = ((h0 + 15) // 16) * ((w0 + 15) // 16)
    return B * h0 * w0 * 3 + max(arena_mcus, per) * 768


def encode_frames(images_dev: torch.Tensor, table: np.ndarray, arena_mcus: int = FRAME_ARENA_MCUS, arena: Optional[torch.Tensor] = None,
                  arena_host: Optional[torch.Tensor] = None, quality: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
    """The device half of the whole-frame 4:2:0 encoder (aq_image_jpeg_coefs) on the current stream, shaped like encode_crops: the frames go
    through an arena of `arena_mcus` MCUs in pieces (a frame never straddles two), each piece comes back through the pinned arena.  Returns
    (coefficients int16 [MCUs, 384] in host memory, table).  quality: None = the entry point of the annotated images (95), or libjpeg's
    1 .. 100 through aq_image_jpeg_coefs_q."""
    _require_gpu()
    lib = load_library()
    assert images_dev.is_cuda and images_dev.dtype == torch.uint8 and images_dev.is_contiguous()
    table = np.ascontiguousarray(table, dtype=FRAME_DTYPE)
    n = table.shape[0]
    if n == 0:
        return np.zeros((0, 384), np.int16), table
    nm = frame_mcus(table)
    ends = table["mcu"].astype(np.int64) + nm
    if table["mcu"][0] != 0 or np.any(table["mcu"][1:] != ends[:-1]):
        raise ValueError("frame table: MCUs must follow each other from 0 (frame_table)")
    w, h = table["w"].astype(np.int64), table["h"].astype(np.int64)
    last = table["base"] + (h - 1) * table["pitch"] + 3 * w
    bad = (w <= 0) | (h <= 0) | (w > 65535) | (h > 65535) | (table["base"] < 0) | (table["pitch"] < 3 * w) | (last > images_dev.numel())
    if bad.any():
        i = int(np.nonzero(bad)[0][0])
        raise ValueError(f"frame {i} {table[i]} is empty or leaves its buffer ({images_dev.numel()} bytes)")
    if int(nm.max()) > arena_mcus:
        raise ValueError(f"a frame of {int(nm.max())} MCUs does not fit an arena of {arena_mcus}")
    if arena is None or arena.numel() < arena_mcus * 384:
        arena = torch.empty(arena_mcus * 384, dtype=torch.int16, device=images_dev.device)
    if arena_host is None or arena_host.numel() < arena_mcus * 384:
        arena_host = torch.empty(arena_mcus * 384, dtype=torch.int16, pin_memory=True)
    table_dev = torch.from_numpy(table.view(np.uint8)).to(images_dev.device, non_blocking=False)
    out = np.empty((int(ends[-1]), 384), np.int16)
    stream = torch.cuda.current_stream()
    c0 = 0
    while c0 < n:
        p0 = int(table["mcu"][c0])
        c1 = int(np.searchsorted(ends, p0 + arena_mcus, side="right"))
        used = int(ends[c1 - 1]) - p0
        if quality is None:
            _check(lib.aq_image_jpeg_coefs(images_dev.data_ptr(), images_dev.numel(), table_dev.data_ptr() + c0 * FRAME_DTYPE.itemsize,
                                           table.ctypes.data + c0 * FRAME_DTYPE.itemsize, c1 - c0, used, arena.data_ptr(), stream.cuda_stream))
        else:
            _check(lib.aq_image_jpeg_coefs_q(images_dev.data_ptr(), images_dev.numel(), table_dev.data_ptr() + c0 * FRAME_DTYPE.itemsize,
                                             table.ctypes.data + c0 * FRAME_DTYPE.itemsize, c1 - c0, used, int(quality), arena.data_ptr(),
                                             stream.cuda_stream))
        arena_host[:used * 384].copy_(arena[:used * 384], non_blocking=True)
        stream.synchronize()
        out[p0:p0 + used] = arena_host[:used * 384].numpy().reshape(used, 384)
        c0 = c1
    return out, table


def image_jpeg_bytes(coef: np.ndarray, w: int, h: int, quality: Optional[int] = None) -> bytes:
    """The 4:2:0 JPEG file of one w x h frame from its MCUs (aq_image_jpeg_bytes; int16 [ceil(w/16) ceil(h/16), 384]); quality: the one
    encode_frames made the coefficients with (None: aq_image_jpeg_bytes, 95; else aq_image_jpeg_bytes_q)."""
    lib = load_library()
    if quality is not None:
        def call(*a):
            return lib.aq_image_jpeg_bytes_q(a[0], a[1], a[2], int(quality), a[3], a[4])
    else:
        call = lib.aq_image_jpeg_bytes
    n = ((w + 15) // 16) * ((h + 15) // 16)
    coef = np.ascontiguousarray(coef.reshape(-1)[:n * 384], dtype=np.int16)
    assert coef.size == n * 384
    buf = C.create_string_buffer(1024 + n * 384)
    k = call(coef.ctypes.data, int(w), int(h), buf, len(buf))
    if k < 0:
        buf = C.create_string_buffer(-k)
        k = call(coef.ctypes.data, int(w), int(h), buf, len(buf))
    if k <= 0:
        raise ValueError(f"image_jpeg_bytes: bad frame size {w} x {h}" + (f" or quality {quality}" if quality is not None else ""))
    return buf.raw[:k]


def write_image_files(root_dir: str, rel_paths, coef: np.ndarray, table: np.ndarray, threads: int = 4, fsync: bool = False,
                      quality: Optional[int] = None) -> int:
    """One C call per batch (aq_write_image_files; no interpreter lock held): frame i of `table`, coefficients from MCU table[i]["mcu"] of
    `coef` (encode_frames), -> <root_dir>/<rel_paths[i]> on `threads` threads.  Returns the number of files."""
    lib = load_library()
    table = np.ascontiguousarray(table, dtype=FRAME_DTYPE)
    coef = np.ascontiguousarray(coef, dtype=np.int16)
    n = table.shape[0]
    assert len(rel_paths) == n and (n == 0 or coef.size >= 384 * int((table["mcu"].astype(np.int64) + frame_mcus(table)).max()))
    if n == 0:
        return 0
    arr = (C.c_char_p * n)(*[os.fsencode(p_) for p_ in rel_paths])
    if quality is None:
        k = lib.aq_write_image_files(os.fsencode(root_dir), arr, coef.ctypes.data, table.ctypes.data, n, int(threads), int(fsync))
    else:
        k = lib.aq_write_image_files_q(os.fsencode(root_dir), arr, coef.ctypes.data, table.ctypes.data, n, int(quality), int(threads), int(fsync))
    if k < 0:
        raise OSError(f"could not write the image {rel_paths[-1 - k]} in {root_dir}")
    return int(k)


def canvas_table(src_bases, src_pitch, sizes) -> Tuple[np.ndarray, int]:
    """CANVAS_DTYPE table of n images: src_bases int64 [n] / src_pitch (scalar or [n]) address the sources, sizes int [n, 2] (h, w); the
    annotated copies lie back to back without row padding (each starting on a 4-byte boundary).  -> (table, bytes of the destination)."""
    sizes = np.asarray(sizes, dtype=np.int64).reshape(-1, 2)
    t = np.zeros(sizes.shape[0], CANVAS_DTYPE)
    t["src"], t["src_pitch"] = src_bases, src_pitch
    t["h"], t["w"] = sizes.T
    t["dst_pitch"] = 3 * sizes[:, 1]
    nbytes = (sizes[:, 0] * sizes[:, 1] * 3 + 3) // 4 * 4
    cw, ch = (sizes[:, 1] + 15) // 16, (sizes[:, 0] + 15) // 16
    t["dst"][1:] = np.cumsum(nbytes)[:-1]
    t["cell"][1:] = np.cumsum(cw * ch)[:-1]
    t["unit"][1:] = np.cumsum((cw + 3) // 4 * ch)[:-1]
    return t, int(nbytes.sum())


def annotate_images(src_dev: torch.Tensor, canvases: np.ndarray, prims: np.ndarray, cell_start: np.ndarray, cell_prims: np.ndarray,
                    atlas_dev: Optional[torch.Tensor], dst_bytes: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """aq_annotate_u8 on the current stream: the images `canvases` (canvas_table) addresses in src_dev, each with the primitives of
    `prims` (PRIM_DTYPE, postprocess.annotation_prims) binned per cell (postprocess.bin_prims) drawn on its copy.  Returns the destination
    buffer (uint8 CUDA, `out` when it is large enough); src_dev is only read."""
    _require_gpu()
    lib = load_library()
    assert src_dev.is_cuda and src_dev.dtype == torch.uint8 and src_dev.is_contiguous()
    canvases = np.ascontiguousarray(canvases, dtype=CANVAS_DTYPE)
    prims = np.ascontiguousarray(prims, dtype=PRIM_DTYPE)
    cell_start = np.ascontiguousarray(cell_start, dtype=np.int32)
    cell_prims = np.ascontiguousarray(cell_prims, dtype=np.int32)
    w, h = canvases["w"].astype(np.int64), canvases["h"].astype(np.int64)
    bad = (w <= 0) | (h <= 0) | (canvases["src"] < 0) | (canvases["src_pitch"] < 3 * w) | \
          (canvases["src"] + (h - 1) * canvases["src_pitch"] + 3 * w > src_dev.numel())
    if canvases.shape[0] == 0 or bad.any():
        raise ValueError(f"image {int(np.nonzero(bad)[0][0]) if bad.any() else 0} is empty or leaves the source buffer ({src_dev.numel()} bytes)")
    n_cells = int((((w + 15) // 16) * ((h + 15) // 16)).sum())
    atlas_bytes = int(atlas_dev.numel()) if atlas_dev is not None else 0
    m = prims["mask_w"] > 0
    if cell_start.shape[0] != n_cells + 1 or cell_start[0] != 0 or cell_start[-1] != cell_prims.shape[0] or np.any(np.diff(cell_start) < 0) or \
            (cell_prims.size and (cell_prims.min() < 0 or cell_prims.max() >= prims.shape[0])):
        raise ValueError("annotate: the cell table does not fit the images and primitives (postprocess.bin_prims)")
    if np.any(prims["mask"][m] < 0) or np.any(prims["mask"][m] + (prims["y1"][m].astype(np.int64) - prims["y0"][m]) * prims["mask_w"][m]
                                              + (prims["x1"][m] - prims["x0"][m]) >= atlas_bytes):
        raise ValueError("annotate: a label mask leaves the atlas")
    if out is None or out.numel() < dst_bytes:
        out = torch.empty(max(dst_bytes, 4), dtype=torch.uint8, device=src_dev.device)
    # one upload for the four tables (8-byte aligned parts)
    parts = [canvases.view(np.uint8), prims.view(np.uint8), cell_start.view(np.uint8), cell_prims.view(np.uint8)]
    offs, total = [], 0
    for a in parts:
        offs.append(total)
        total += (a.size + 7) // 8 * 8
    host = np.zeros(max(total, 8), np.uint8)
    for a, o in zip(parts, offs):
        host[o:o + a.size] = a
    tab = torch.from_numpy(host).to(src_dev.device)
    base = tab.data_ptr()
    _check(lib.aq_annotate_u8(src_dev.data_ptr(), src_dev.numel(), out.data_ptr(), out.numel(), base + offs[0], canvases.ctypes.data, canvases.shape[0],
                              base + offs[1] if prims.shape[0] else None, prims.shape[0], base + offs[2], n_cells,
                              base + offs[3] if prims.shape[0] else None, cell_prims.shape[0],
                              atlas_dev.data_ptr() if atlas_bytes else None, atlas_bytes, _stream_ptr()))
    tab.record_stream(torch.cuda.current_stream())
    return out


# ---- val.py --plots: aq_val_mosaic_u8 (the mosaic of a batch's first images; geometry and tables in val_plots.py) ----

def val_mosaic(batch: torch.Tensor, n: int, ns: int, h: int, w: int, xtab: np.ndarray, ytab: np.ndarray, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """aq_val_mosaic_u8 on the current stream: the first n images of `batch` (uint8 CUDA [B, H, W, 3], contiguous; a view inside a larger
    allocation is fine) in ns x ns cells of h x w pixels -> uint8 CUDA [ns h, ns w, 3] (`out` when given).  xtab int32 [ns w, 4], ytab int32
    [ns h, 4]: (i0, i1, w0, w1) per output column / row (val_plots.mosaic_tables)."""
    _require_gpu()
    lib = load_library()
    assert batch.is_cuda and batch.dtype == torch.uint8 and batch.dim() == 4 and batch.shape[3] == 3 and batch.is_contiguous()
    B, H, W, _ = batch.shape
    xtab = np.ascontiguousarray(xtab, dtype=np.int32).reshape(-1, 4)
    ytab = np.ascontiguousarray(ytab, dtype=np.int32).reshape(-1, 4)
    out_h, out_w = int(ytab.shape[0]), int(xtab.shape[0])
    if out is None:
        out = torch.empty((out_h, out_w, 3), dtype=torch.uint8, device=batch.device)
    assert out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous()
    tab = torch.from_numpy(np.concatenate([xtab, ytab])).to(batch.device)         # one upload; int4 entries, 16-byte aligned
    _check(lib.aq_val_mosaic_u8(batch.data_ptr(), batch.numel(), int(n), int(ns), H, W, int(h), int(w),
                                out.data_ptr(), out.numel(), out_h, out_w, tab.data_ptr(), xtab.ctypes.data,
                                tab.data_ptr() + 16 * out_w, ytab.ctypes.data, _stream_ptr()))
    tab.record_stream(torch.cuda.current_stream())
    return out


# ---- --blank-key: aq_blank_stats_u8 (grey extrema, blank rows and columns, non-blank pixels of every source image) ----

BLANK_FIELDS = ("l_min", "l_max", "blank_rows", "blank_cols", "nonblank_px", "x0", "y0", "x1", "y1")      # aq_blank_stat


def blank_frame_table(bases, pitch, sizes) -> np.ndarray:
    """FRAME_DTYPE table of n images for blank_stats: bases int64 [n] (byte offset of each image), pitch (row bytes; scalar or [n]), sizes int
    [n, 2] (h, w); `mcu` = the image's first word among the scratch's column sums (the images' columns follow each other from 0)."""
    sizes = np.asarray(sizes, dtype=np.int64).reshape(-1, 2)
    t = np.zeros(sizes.shape[0], FRAME_DTYPE)
    t["base"], t["pitch"] = bases, pitch
    t["h"], t["w"] = sizes.T
    if sizes[:, 1].sum() >= 1 << 31:
        raise ValueError("blank frame table: more than 2^31 columns in one call")
    t["mcu"][1:] = np.cumsum(sizes[:, 1])[:-1]
    return t


def blank_key_bytes(B: int, h0: int, w0: int) -> int:
    """Device bytes one pipeline slot holds for --blank-key with batches of B images of h0 x w0: the kernel's scratch (8 words per image and
    one per column), the frame table and the records."""
    return B * (8 + w0) * 4 + B * FRAME_DTYPE.itemsize + B * 4 * len(BLANK_FIELDS)


def blank_stats(images_dev: torch.Tensor, frames: np.ndarray, stream: Optional[torch.cuda.Stream] = None, scratch: Optional[torch.Tensor] = None,
                out: Optional[torch.Tensor] = None, frames_dev: Optional[torch.Tensor] = None) -> torch.Tensor:
    """aq_blank_stats_u8 on `stream` (default: the current one): the statistics of the images `frames` (blank_frame_table) addresses in the
    uint8 CUDA buffer images_dev -> int32 CUDA [n, 9] (BLANK_FIELDS), exactly blank.stats_numpy of each image.  `scratch` (uint8 CUDA),
    `out` (int32 CUDA [>= n, 9]) and `frames_dev` (the table in device memory, uint8) are used when given and large enough: the call
    itself allocates nothing then.  A frame that leaves the buffer raises before anything is launched."""
    _require_gpu()
    lib = load_library()
    assert images_dev.is_cuda and images_dev.dtype == torch.uint8 and images_dev.is_contiguous()
    frames = np.ascontiguousarray(frames, dtype=FRAME_DTYPE)
    n = frames.shape[0]
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        if out is None or out.shape[0] < n:
            out = torch.empty((n, len(BLANK_FIELDS)), dtype=torch.int32, device=images_dev.device)
        if n == 0:
            _check(lib.aq_blank_stats_u8(images_dev.data_ptr(), images_dev.numel(), None, None, 0, None, 0, None, _stream_ptr()))
            return out[:0]
        need = int(lib.aq_blank_stats_scratch_bytes(frames.ctypes.data, n))
        if scratch is None or scratch.numel() < need:
            scratch = torch.empty(max(need, 4), dtype=torch.uint8, device=images_dev.device)
        if frames_dev is None:
            frames_dev = torch.from_numpy(frames.view(np.uint8)).to(images_dev.device)
        assert frames_dev.numel() >= frames.nbytes
        _check(lib.aq_blank_stats_u8(images_dev.data_ptr(), images_dev.numel(), frames_dev.data_ptr(), frames.ctypes.data, n, scratch.data_ptr(),
                                     scratch.numel(), out.data_ptr(), _stream_ptr()))
        for t_ in (scratch, frames_dev, out):
            t_.record_stream(torch.cuda.current_stream())
    return out[:n]


# ---- --blank-geom: aq_blank_components_u8 / aq_blank_ring_edges_u8 (components of the non-blank mask, the largest one, its outer edges) ----

GEOM_FIELDS = ("examined", "n_components", "label", "px", "area_px", "x0", "y0", "x1", "y1", "n_edges", "edge_px", "reserved")      # aq_blank_geom
GEOM_GROUP_SLOTS = 16 << 20        # scratch slots (9 bytes each: 151 MB) blank_geom_groups gives one call: sixteen 1024-px tiles


def blank_geom_slots(sizes) -> np.ndarray:
    """Scratch slots of images of the sizes int [n, 2] (h, w): (w + 1) h + 2, rounded up to a multiple of 4."""
    sizes = np.asarray(sizes, dtype=np.int64).reshape(-1, 2)
    return ((sizes[:, 1] + 1) * sizes[:, 0] + 2 + 3) // 4 * 4


def blank_geom_frame_table(bases, pitch, sizes) -> np.ndarray:
    """FRAME_DTYPE table of n images for blank_components (arguments as blank_frame_table's); `mcu` = the image's first scratch slot."""
    sizes = np.asarray(sizes, dtype=np.int64).reshape(-1, 2)
    t = np.zeros(sizes.shape[0], FRAME_DTYPE)
    t["base"], t["pitch"] = bases, pitch
    t["h"], t["w"] = sizes.T
    slots = blank_geom_slots(sizes)
    if slots.sum() >= 1 << 31:
        raise ValueError("blank geom frame table: more than 2^31 scratch slots in one call")
    t["mcu"][1:] = np.cumsum(slots)[:-1]
    return t


def blank_geom_groups(sizes, limit: int = GEOM_GROUP_SLOTS) -> List[List[int]]:
    """Images of the sizes int [n, 2] (h, w) in groups, in order, whose scratch slots stay within `limit` (an image larger than that is a
    group of its own): what bounds the scratch of --blank-geom to 9 bytes x limit whatever the batch."""
    groups, room = [], 0
    for k, s in enumerate(blank_geom_slots(sizes).tolist()):
        if not groups or room < s:
            groups.append([])
            room = limit
        groups[-1].append(k)
        room -= s
    return groups


def blank_components(images_dev: torch.Tensor, frames: np.ndarray, stats_dev: Optional[torch.Tensor] = None, stream: Optional[torch.cuda.Stream] = None,
                     scratch: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, frames_dev: Optional[torch.Tensor] = None,
                     labels: bool = False):
    """aq_blank_components_u8 on `stream` (default: the current one): per image `frames` (blank_geom_frame_table) addresses in the uint8 CUDA
    buffer images_dev its aq_blank_geom record -> int32 CUDA [n, 12] (GEOM_FIELDS), exactly blank_geom.components_numpy's.  stats_dev = the
    images' blank_stats records (int32 CUDA [n, 9]): only partly blank images with a non-blank pixel are examined then.  labels=True:
    -> (records, int32 CUDA [2 x slots]: per image its two label maps from 2 mcu).  Returns (records, scratch, frames_dev[, labels]): the
    scratch and the device table are what blank_ring_edges reads.  A frame that leaves the buffer raises before anything is launched."""
    _require_gpu()
    lib = load_library()
    assert images_dev.is_cuda and images_dev.dtype == torch.uint8 and images_dev.is_contiguous()
    frames = np.ascontiguousarray(frames, dtype=FRAME_DTYPE)
    n = frames.shape[0]
    dev = images_dev.device
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        if out is None or out.shape[0] < n:
            out = torch.empty((n, len(GEOM_FIELDS)), dtype=torch.int32, device=dev)
        if n == 0:
            _check(lib.aq_blank_components_u8(images_dev.data_ptr(), images_dev.numel(), None, None, 0, None, None, 0, None, None, _stream_ptr()))
            return (out[:0], scratch, frames_dev) + ((torch.empty(0, dtype=torch.int32, device=dev),) if labels else ())
        need = int(lib.aq_blank_geom_scratch_bytes(frames.ctypes.data, n))
        if scratch is None or scratch.numel() < need:
            scratch = torch.empty(max(need, 8), dtype=torch.uint8, device=dev)
        if frames_dev is None:
            frames_dev = torch.from_numpy(frames.view(np.uint8)).to(dev)
        assert frames_dev.numel() >= frames.nbytes
        if stats_dev is not None:
            assert stats_dev.is_cuda and stats_dev.dtype == torch.int32 and stats_dev.is_contiguous() and tuple(stats_dev.shape) == (n, len(BLANK_FIELDS))
        maps = None
        if labels:
            maps = torch.full((2 * int(blank_geom_slots(np.stack([frames["h"], frames["w"]], 1)).sum()),), -3, dtype=torch.int32, device=dev)
        _check(lib.aq_blank_components_u8(images_dev.data_ptr(), images_dev.numel(), frames_dev.data_ptr(), frames.ctypes.data, n,
                                          stats_dev.data_ptr() if stats_dev is not None else None, scratch.data_ptr(), scratch.numel(),
                                          out.data_ptr(), maps.data_ptr() if labels else None, _stream_ptr()))
        for t_ in (scratch, frames_dev, out) + ((stats_dev,) if stats_dev is not None else ()) + ((maps,) if labels else ()):
            t_.record_stream(torch.cuda.current_stream())
    return (out[:n], scratch, frames_dev) + ((maps,) if labels else ())


def blank_ring_edges(frames: np.ndarray, records: np.ndarray, records_dev: torch.Tensor, scratch: torch.Tensor, frames_dev: torch.Tensor,
                     stream: Optional[torch.cuda.Stream] = None) -> List[np.ndarray]:
    """aq_blank_ring_edges_u8 after blank_components on the same table: records = its records on the host (they size the slices),
    records_dev / scratch / frames_dev = what it returned.  -> per image int32 [edge_px, 2] (pixel index, side mask), sorted by pixel
    index, so that the result does not depend on the order the kernel wrote them in.  Synchronises the stream."""
    _require_gpu()
    lib = load_library()
    frames = np.ascontiguousarray(frames, dtype=FRAME_DTYPE)
    n = frames.shape[0]
    records = np.asarray(records).reshape(n, len(GEOM_FIELDS))
    at = np.zeros(n + 1, np.int64)
    at[1:] = np.cumsum(records[:, GEOM_FIELDS.index("edge_px")].astype(np.int64))
    total = int(at[-1])
    if n == 0 or total == 0:
        return [np.zeros((0, 2), np.int32) for _ in range(n)]
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        at_dev = torch.from_numpy(at).to(scratch.device)
        edges = torch.full((total, 2), -1, dtype=torch.int32, device=scratch.device)
        _check(lib.aq_blank_ring_edges_u8(frames_dev.data_ptr(), frames.ctypes.data, n, scratch.data_ptr(), scratch.numel(), records_dev.data_ptr(),
                                          at_dev.data_ptr(), at.ctypes.data, edges.data_ptr(), total, _stream_ptr()))
        for t_ in (scratch, frames_dev, records_dev, at_dev, edges):
            t_.record_stream(torch.cuda.current_stream())
        host = edges.cpu().numpy()                          # (waits for the stream)
    out = []
    for k in range(n):
        e = host[at[k]:at[k + 1]]
        out.append(e[np.argsort(e[:, 0], kind="stable")])
    return out


# ---- --facilities: aq_facility_dbscan_f64 (DBSCAN of the detections' centroids, as sklearn labels them) ----

FACILITY_CELL_BITS = 21                    # AQ_FACILITY_CELL_BITS: key = group << 42 | cell_y << 21 | cell_x
FACILITY_CELL_FACTOR = 1.0 + 2.0 ** -20    # cell edge = eps x this


def facility_sort_keys(xy: torch.Tensor, group: torch.Tensor, eps: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """The sort aq_facility_dbscan_f64 takes: xy float64 [n, 2] and group int32 [n] (dense ids) on one device -> (keys int64 [n] ascending,
    perm int32 [n]: the original index of every sorted position).  key = group << 42 | cell_y << 21 | cell_x with
    cell = floor((v - min v) / h) + 1 per axis, h = eps (1 + 2^-20).

    Two points within eps never lie two cells apart.  With t = (v - min v) / h exact, |v_a - v_b| <= eps (1 + 2^-51) for every pair the
    kernel's rounded test dx dx + dy dy <= eps eps can accept (the differences, the products, the sum and eps eps are each rounded once, by at
    most 2^-53 of the value; along one axis that is at most six roundings of a squared length, under 2^-51 of the length), so
    t_a - t_b <= (1 + 2^-51) / (1 + 2^-20) < 1 - 2^-21.  The computed t carries two roundings (the subtraction and the division): a relative
    error below 2^-52, and t < 2^21 (checked), so an absolute error below 2^-31 each.  The computed difference is therefore below
    1 - 2^-21 + 2^-30 < 1, and floor values of two numbers less than 1 apart differ by at most 1.  (torch.floor of a finite double is
    exact.)  A coordinate that is not finite, a grid of more than 2^21 - 2 cells along an axis or a group outside [0, 2^21) raises."""
    assert xy.dtype == torch.float64 and xy.ndim == 2 and xy.shape[1] == 2 and group.dtype == torch.int32 and group.shape == (xy.shape[0],)
    if not eps > 0:
        raise ValueError(f"facilities: eps = {eps} (it has to be positive)")
    h = float(eps) * FACILITY_CELL_FACTOR
    top = (1 << FACILITY_CELL_BITS) - 2
    cell = torch.floor((xy - xy.min(dim=0).values) / h) + 1.0
    lo, hi = cell.aminmax()
    g_lo, g_hi = group.aminmax()
    lo, hi, g_lo, g_hi = (float(v) for v in torch.stack([lo, hi, g_lo.double(), g_hi.double()]).tolist())
    if not (lo >= 1.0 and hi <= top):                       # (NaN fails too)
        raise ValueError(f"facilities: the points span more than {top} cells of {h:g} m along an axis, or a coordinate is not finite")
    if g_lo < 0 or g_hi >= 1 << FACILITY_CELL_BITS:
        raise ValueError(f"facilities: group ids have to lie in [0, 2^{FACILITY_CELL_BITS})")
    cell = cell.to(torch.int64)
    key = (group.to(torch.int64) << (2 * FACILITY_CELL_BITS)) | (cell[:, 1] << FACILITY_CELL_BITS) | cell[:, 0]
    keys, perm = torch.sort(key)
    return keys, perm.to(torch.int32)


class _Phases:
    """HIP events around the phases of a wrapper's call on the current stream: mark() before each phase, done(key, ...) after the last one
    writes the phases' milliseconds into `times` under those keys (the call then waits for them).  With times = None nothing is recorded."""

    def __init__(self, times: Optional[dict]):
        self.times, self.events = times, []

    def mark(self) -> None:
        if self.times is not None:
            self.events.append(torch.cuda.Event(enable_timing=True))
            self.events[-1].record()

    def done(self, *keys: str) -> None:
        if self.times is not None:
            self.mark()
            self.events[-1].synchronize()
            for key, a, b in zip(keys, self.events, self.events[1:]):
                self.times[key] = a.elapsed_time(b)


def facility_dbscan(xy: torch.Tensor, group: torch.Tensor, eps: float, min_samples: int, stream: Optional[torch.cuda.Stream] = None,
                    scratch: Optional[torch.Tensor] = None, times: Optional[dict] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """aq_facility_dbscan_f64 on `stream` (default: the current one): xy float64 CUDA [n, 2] (metres), group int32 CUDA [n] (dense ids; points
    of different groups never interact) -> (core uint8 CUDA [n], root int32 CUDA [n]) in the caller's order: root = the smallest original
    index among the core points of the point's cluster, -1 for noise (facilities.dbscan_numpy gives the same).  The sort is torch's
    (facility_sort_keys), the neighbour search, the union-find and the border pass are the kernels'.  times = a dict that receives
    "sort_ms" and "kernel_ms" (HIP events; the call then waits for them)."""
    _require_gpu()
    lib = load_library()
    assert xy.is_cuda and group.is_cuda and xy.dtype == torch.float64 and group.dtype == torch.int32
    xy, group = xy.contiguous(), group.contiguous()
    n = xy.shape[0]
    if not eps > 0 or int(min_samples) < 1:                 # the library refuses these too; here before the sort
        raise ValueError(f"facilities: eps = {eps}, min_samples = {min_samples} (eps > 0 and min_samples >= 1)")
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        core = torch.empty(n, dtype=torch.uint8, device=xy.device)
        root = torch.empty(n, dtype=torch.int32, device=xy.device)
        if n == 0:
            _check(lib.aq_facility_dbscan_f64(None, None, None, None, 0, float(eps), int(min_samples), None, 0, None, None, _stream_ptr()))
            return core, root
        ph = _Phases(times)
        ph.mark()
        keys, perm = facility_sort_keys(xy, group, eps)
        need = int(lib.aq_facility_scratch_bytes(n))
        if scratch is None or scratch.numel() < need:
            scratch = torch.empty(need, dtype=torch.uint8, device=xy.device)
        ph.mark()
        _check(lib.aq_facility_dbscan_f64(keys.data_ptr(), perm.data_ptr(), xy.data_ptr(), group.data_ptr(), n, float(eps), int(min_samples),
                                          scratch.data_ptr(), scratch.numel(), core.data_ptr(), root.data_ptr(), _stream_ptr()))
        ph.done("sort_ms", "kernel_ms")
        for t_ in (keys, perm, xy, group, scratch, core, root):
            t_.record_stream(torch.cuda.current_stream())
    return core, root


# ---- --evaluate: aq_eval_member_conf_f64 and aq_box_match_f64 (the precision / recall grid without a DBSCAN run per grid point) ----

EVAL_MAX_K = 16


def eval_member_conf(xy: torch.Tensor, group: torch.Tensor, conf: torch.Tensor, eps: float, K: int, times: Optional[dict] = None) -> torch.Tensor:
    """aq_eval_member_conf_f64 on the current stream: xy float64 CUDA [n, 2] (metres), group int32 CUDA [n] (dense ids), conf float64 CUDA [n]
    -> M float64 CUDA [n, K] in the caller's order: M[i, m - 1] = the largest confidence threshold at which DBSCAN(eps, min_samples = m) over
    the points of at least that confidence makes point i a member of a cluster (-inf: none); evaluate.member_conf_numpy gives the same
    bytes.  The sort is torch's (facility_sort_keys).  times = a dict that receives "sort_ms" and "kernel_ms" (HIP events; the call then
    waits for them)."""
    return _eval_member_conf(xy, group, conf, eps, K, times)


def _eval_member_conf(xy, group, conf, eps, K, times, mask=None, S=None):
    """The body of eval_member_conf (S = None) and of eval_member_conf_subsets (mask and S given): the same checks, sort, scratch and call,
    with the mask words and S passed on to the subsets entry."""
    _require_gpu()
    lib = load_library()
    assert xy.is_cuda and group.is_cuda and conf.is_cuda and xy.dtype == torch.float64 and group.dtype == torch.int32 and conf.dtype == torch.float64
    xy, group, conf = xy.contiguous(), group.contiguous(), conf.contiguous()
    n = xy.shape[0]
    assert xy.shape == (n, 2) and group.shape == (n,) and conf.shape == (n,)
    if S is None:                                           # the library refuses these too; here before the sort
        if not eps > 0 or not 1 <= int(K) <= EVAL_MAX_K:
            raise ValueError(f"evaluate: eps = {eps}, K = {K} (eps > 0 and 1 <= K <= {EVAL_MAX_K})")
        fn, scratch_bytes, sizes, arrays = lib.aq_eval_member_conf_f64, lib.aq_eval_scratch_bytes, (int(K),), (xy, group, conf)
    else:
        if not eps > 0 or not 1 <= int(K) <= EVAL_MAX_K or not 1 <= int(S) <= EVAL_MAX_S:
            raise ValueError(f"evaluate subsets: eps = {eps}, K = {K}, S = {S} (eps > 0, 1 <= K <= {EVAL_MAX_K} and 1 <= S <= {EVAL_MAX_S})")
        fn, scratch_bytes, sizes = lib.aq_eval_member_conf_subsets_f64, lib.aq_eval_subsets_scratch_bytes, (int(K), int(S))
        arrays = (xy, group, conf, _subset_words(mask, n, "mask"))
    M = torch.empty(sizes[1:] + (n, int(K)), dtype=torch.float64, device=xy.device)
    if n == 0:                                              # null pointers: the library still validates eps, K and S
        _check(fn(None, None, *(None for _ in arrays), 0, float(eps), *sizes, None, 0, None, _stream_ptr()))
        return M
    need = int(scratch_bytes(n, *sizes))
    if S is not None and need == 0:
        raise ValueError(f"evaluate subsets: {n} points x {K} sizes x {S} subsets is more than one call takes")
    ph = _Phases(times)
    ph.mark()
    arrays = facility_sort_keys(xy, group, eps) + arrays
    scratch = torch.empty(need, dtype=torch.uint8, device=xy.device)
    ph.mark()
    _check(fn(*(t_.data_ptr() for t_ in arrays), n, float(eps), *sizes, scratch.data_ptr(), scratch.numel(), M.data_ptr(), _stream_ptr()))
    ph.done("sort_ms", "kernel_ms")
    for t_ in arrays + (scratch, M):
        t_.record_stream(torch.cuda.current_stream())
    return M


def box_match_sort(kbox: torch.Tensor, kgroup: torch.Tensor, G: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The key order aq_box_match_f64 takes: kbox float64 [N, 4], kgroup int32 [N] with ids in [0, G) -> (order int64 [N]: by (group, x0),
    stable; group_start int32 [G + 1])."""
    by_x = torch.sort(kbox[:, 0], stable=True).indices
    order = by_x[torch.sort(kgroup[by_x], stable=True).indices]
    start = torch.searchsorted(kgroup[order].to(torch.int64), torch.arange(G + 1, device=kbox.device))
    return order, start.to(torch.int32)


def _join_inputs(what: str, qbox, qgroup, kbox, kgroup, G, S=None):
    """What the three box joins check before anything else, under the caller's message prefix: dtypes and shapes, S when there are subsets,
    the keys' group ids -> (the library, qbox and qgroup contiguous, Q, N, G)."""
    _require_gpu()
    lib = load_library()
    assert qbox.is_cuda and qbox.dtype == torch.float64 and kbox.dtype == torch.float64 and qgroup.dtype == torch.int32 and kgroup.dtype == torch.int32
    qbox, qgroup = qbox.contiguous(), qgroup.contiguous()
    Q, N, G = qbox.shape[0], kbox.shape[0], int(G)
    assert qbox.shape == (Q, 4) and kbox.shape == (N, 4) and qgroup.shape == (Q,) and kgroup.shape == (N,)
    if S is not None and not 1 <= S <= EVAL_MAX_S:
        raise ValueError(f"{what}: S = {S} subsets (1 to {EVAL_MAX_S})")
    if G < 0 or (N and not (0 <= int(kgroup.min()) and int(kgroup.max()) < G)):
        raise ValueError(f"{what}: the keys' group ids have to lie in [0, {G})")
    return lib, qbox, qgroup, Q, N, G


def box_match(qbox: torch.Tensor, qgroup: torch.Tensor, kbox: torch.Tensor, kgroup: torch.Tensor, G: int, payload: Optional[torch.Tensor] = None,
              times: Optional[dict] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """aq_box_match_f64 on the current stream: qbox float64 CUDA [Q, 4] (x0, y0, x1, y1), qgroup int32 CUDA [Q], kbox float64 CUDA [N, 4],
    kgroup int32 CUDA [N] with ids in [0, G), in any order (box_match_sort sorts them), payload float64 CUDA [N, K] or None ->
    (hit uint8 CUDA [Q]: the query's closed box meets the closed box of a key of its group; out float64 CUDA [Q, K]: the elementwise
    maximum of the payload over those keys, -inf without one -- None without a payload).  evaluate.box_match_numpy gives the same bytes.
    times = a dict that receives "sort_ms" and "kernel_ms"."""
    lib, qbox, qgroup, Q, N, G = _join_inputs("box match", qbox, qgroup, kbox, kgroup, G)
    K = 0
    if payload is not None:
        assert payload.is_cuda and payload.dtype == torch.float64 and payload.ndim == 2 and payload.shape[0] == N
        K = payload.shape[1]
        if not 1 <= K <= EVAL_MAX_K:
            raise ValueError(f"box match: {K} payload columns (1 to {EVAL_MAX_K})")
    hit = torch.empty(Q, dtype=torch.uint8, device=qbox.device)
    out = torch.empty((Q, K), dtype=torch.float64, device=qbox.device) if payload is not None else None
    if Q == 0:
        return hit, out
    ph = _Phases(times)
    ph.mark()
    order, start = box_match_sort(kbox, kgroup, G)
    kb = kbox[order].contiguous()
    pl = payload[order].contiguous() if payload is not None else None
    ph.mark()
    _check(lib.aq_box_match_f64(qbox.data_ptr(), qgroup.data_ptr(), Q, kb.data_ptr() if N else None, N, start.data_ptr(), G,
                                pl.data_ptr() if pl is not None and N else None, K, hit.data_ptr(), out.data_ptr() if out is not None else None,
                                _stream_ptr()))
    ph.done("sort_ms", "kernel_ms")
    for t_ in (qbox, qgroup, kb, start, hit) + ((pl, out) if pl is not None else ()):
        t_.record_stream(torch.cuda.current_stream())
    return hit, out


# ---- --evaluate-kfold: aq_eval_member_conf_subsets_f64 and aq_box_match_subsets_f64 (the same two steps for up to 32 subsets of the points) ----

EVAL_MAX_S = 32


def _subset_words(mask: torch.Tensor, n: int, what: str) -> torch.Tensor:
    """A mask of subset bits as the int32 words the library reads as uint32 (torch has no arithmetic on uint32): int32, or int64 in [0, 2^32)."""
    assert mask.is_cuda and mask.shape == (n,) and mask.dtype in (torch.int32, torch.int64), f"{what}: int32 or int64 CUDA [{n}]"
    if mask.dtype == torch.int64:
        mask = torch.where(mask >= (1 << 31), mask - (1 << 32), mask).to(torch.int32)     # bit 31 is the sign bit of the word
    return mask.contiguous()


def eval_member_conf_subsets(xy: torch.Tensor, group: torch.Tensor, conf: torch.Tensor, mask: torch.Tensor, eps: float, K: int, S: int,
                             times: Optional[dict] = None) -> torch.Tensor:
    """aq_eval_member_conf_subsets_f64 on the current stream: the arguments of eval_member_conf plus mask (int32 CUDA [n], read as uint32, or
    int64 in [0, 2^32): bit s set = the point is in subset s) and S in 1 .. 32 -> M float64 CUDA [S, n, K]: M[s, i] = eval_member_conf's row of
    point i among the points of subset s alone, -inf for a point outside s; evaluate.member_conf_subsets_numpy gives the same bytes.  One sort
    (facility_sort_keys), one gather and one set of key runs for all subsets.  times = a dict that receives "sort_ms" and "kernel_ms"."""
    return _eval_member_conf(xy, group, conf, eps, K, times, mask, S)


def box_match_subsets(qbox: torch.Tensor, qgroup: torch.Tensor, qmask: torch.Tensor, kbox: torch.Tensor, kgroup: torch.Tensor, kmask: torch.Tensor,
                      G: int, S: int, payload: Optional[torch.Tensor] = None, times: Optional[dict] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """aq_box_match_subsets_f64 on the current stream: the arguments of box_match plus qmask [Q] and kmask [N] (subset words as in
    eval_member_conf_subsets, the keys' in the caller's order) and S; payload float64 CUDA [S, N, K] or None -> (hitmask int32 CUDA [Q], the
    uint32 word qmask & OR of the matching keys' kmask; out float64 CUDA [S, Q, K]: per subset the elementwise maximum of its payload over the
    matching keys of that subset, -inf without one or for a query outside it -- None without a payload).
    evaluate.box_match_subsets_numpy gives the same bytes.  times = a dict that receives "sort_ms" and "kernel_ms"."""
    S = int(S)
    lib, qbox, qgroup, Q, N, G = _join_inputs("box match subsets", qbox, qgroup, kbox, kgroup, G, S)
    qwords, kwords = _subset_words(qmask, Q, "qmask"), _subset_words(kmask, N, "kmask")
    K = 0
    if payload is not None:
        assert payload.is_cuda and payload.dtype == torch.float64 and payload.ndim == 3 and payload.shape[:2] == (S, N)
        K = payload.shape[2]
        if not 1 <= K <= EVAL_MAX_K:
            raise ValueError(f"box match subsets: {K} payload columns (1 to {EVAL_MAX_K})")
    if lib.aq_box_match_subsets_scratch_bytes(Q, N, K, S) != 0:
        raise ValueError(f"box match subsets: {Q} queries x {N} keys x {K} columns x {S} subsets is more than one call takes")
    hit = torch.empty(Q, dtype=torch.int32, device=qbox.device)
    out = torch.empty((S, Q, K), dtype=torch.float64, device=qbox.device) if payload is not None else None
    if Q == 0:
        return hit, out
    ph = _Phases(times)
    ph.mark()
    order, start = box_match_sort(kbox, kgroup, G)
    kb, km = kbox[order].contiguous(), kwords[order].contiguous()
    pl = payload[:, order].contiguous() if payload is not None else None
    ph.mark()
    _check(lib.aq_box_match_subsets_f64(qbox.data_ptr(), qgroup.data_ptr(), qwords.data_ptr(), Q, kb.data_ptr() if N else None, km.data_ptr() if N else None,
                                        N, start.data_ptr(), G, pl.data_ptr() if pl is not None and N else None, K, S, hit.data_ptr(),
                                        out.data_ptr() if out is not None else None, _stream_ptr()))
    ph.done("sort_ms", "kernel_ms")
    for t_ in (qbox, qgroup, qwords, kb, km, start, hit) + ((pl, out) if pl is not None else ()):
        t_.record_stream(torch.cuda.current_stream())
    return hit, out


# ---- --model-errors: aq_model_error_match_f64 and aq_model_error_moments_f64 (the cage-area error distributions) ----

def model_error_match(qbox: torch.Tensor, qgroup: torch.Tensor, qarea: torch.Tensor, kbox: torch.Tensor, kgroup: torch.Tensor, karea: torch.Tensor,
                      G: int, times: Optional[dict] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """aq_model_error_match_f64 on the current stream: qbox float64 CUDA [Q, 4] (x0, y0, x1, y1), qgroup int32 CUDA [Q], qarea float64 CUDA [Q],
    kbox float64 CUDA [N, 4], kgroup int32 CUDA [N] with ids in [0, G), karea float64 CUDA [N], the keys in any order (box_match_sort sorts
    them) -> (match int32 CUDA [Q]: the row of the key of the query's group whose closed box overlaps the query's most, the smallest row among
    equals, -1 without one; overlap float64 CUDA [Q]: 100 x the intersection's share of the query's box; error float64 CUDA [Q]:
    karea[match] - qarea; both NaN without a match).  model_errors.match_numpy gives the same bytes.  times = a dict that receives "sort_ms"
    and "kernel_ms"."""
    assert qarea.dtype == torch.float64 and karea.dtype == torch.float64 and qarea.shape == qbox.shape[:1] and karea.shape == kbox.shape[:1]
    lib, qbox, qgroup, Q, N, G = _join_inputs("model errors", qbox, qgroup, kbox, kgroup, G)
    qarea = qarea.contiguous()
    match = torch.empty(Q, dtype=torch.int32, device=qbox.device)
    overlap = torch.empty(Q, dtype=torch.float64, device=qbox.device)
    error = torch.empty(Q, dtype=torch.float64, device=qbox.device)
    if Q == 0:
        return match, overlap, error
    ph = _Phases(times)
    ph.mark()
    order, start = box_match_sort(kbox, kgroup, G)
    kb, ka, kr = kbox[order].contiguous(), karea[order].contiguous(), order.to(torch.int32)
    ph.mark()
    _check(lib.aq_model_error_match_f64(qbox.data_ptr(), qgroup.data_ptr(), qarea.data_ptr(), Q, kb.data_ptr() if N else None,
                                        kr.data_ptr() if N else None, ka.data_ptr() if N else None, N, start.data_ptr(), G,
                                        match.data_ptr(), overlap.data_ptr(), error.data_ptr(), _stream_ptr()))
    ph.done("sort_ms", "kernel_ms")
    for t_ in (qbox, qgroup, qarea, kb, ka, kr, start, match, overlap, error):
        t_.record_stream(torch.cuda.current_stream())
    return match, overlap, error


def model_error_moments(error: torch.Tensor, match: torch.Tensor, mgroup: torch.Tensor, G: int,
                        times: Optional[dict] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """aq_model_error_moments_f64 on the current stream: error float64 CUDA [Q], match int32 CUDA [Q], mgroup int32 CUDA [Q] (a row outside
    [0, G) belongs to no group) -> (n int64 CUDA [G], mean float64 CUDA [G], sd float64 CUDA [G]) over the rows with match >= 0 and a finite
    error, per group, summed in the order include/aq_engine.h states; mean and sd are NaN where n = 0.  model_errors.moments_numpy gives the
    same bytes.  times = a dict that receives "kernel_ms"."""
    _require_gpu()
    lib = load_library()
    assert error.is_cuda and error.dtype == torch.float64 and match.dtype == torch.int32 and mgroup.dtype == torch.int32
    error, match, mgroup = error.contiguous(), match.contiguous(), mgroup.contiguous()
    Q, G = error.shape[0], int(G)
    assert error.shape == (Q,) and match.shape == (Q,) and mgroup.shape == (Q,)
    if G < 0:
        raise ValueError(f"model errors: {G} moment groups")
    n = torch.empty(G, dtype=torch.int64, device=error.device)
    mean = torch.empty(G, dtype=torch.float64, device=error.device)
    sd = torch.empty(G, dtype=torch.float64, device=error.device)
    if G == 0:
        return n, mean, sd
    ph = _Phases(times)
    ph.mark()
    _check(lib.aq_model_error_moments_f64(error.data_ptr() if Q else None, match.data_ptr() if Q else None, mgroup.data_ptr() if Q else None, Q, G,
                                          n.data_ptr(), mean.data_ptr(), sd.data_ptr(), _stream_ptr()))
    ph.done("kernel_ms")
    for t_ in (error, match, mgroup, n, mean, sd):
        t_.record_stream(torch.cuda.current_stream())
    return n, mean, sd


# ---- --tonnage: aq_tonnage_simulate_f64 / aq_tonnage_reduce_f64 (the production bootstrap) and the two test hooks ----

def tonnage_simulate(seed: int, k0: int, K: int, entry_start: torch.Tensor, area: torch.Tensor, err: torch.Tensor, flags: torch.Tensor,
                     depth: torch.Tensor, pass_id: torch.Tensor, pass_params: torch.Tensor, mix: float, min_depth: float, probs,
                     moments: torch.Tensor, entry_start_host: Optional[np.ndarray] = None,
                     pass_params_host: Optional[np.ndarray] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Simulations k0 .. k0 + K - 1 on the current stream -> (ton float64 CUDA [K, F], T float64 CUDA [K, P]); moments (float64 CUDA [F, 2],
    the caller's) grows by the chunk's sums and sums of squares.  entry_start int32 [F + 1], area float64 [E], err float64 [E, 2], flags
    uint8 [E], depth float64 [F], pass_id int32 [F], pass_params float64 [P, 6], all CUDA and contiguous; probs = the four depth
    probabilities.  entry_start_host, pass_params_host = the two tables' content in host memory (the ABI checks them there before it
    launches); a caller that has them passes them, else they are copied back here, which synchronises.  include/aq_engine.h states the
    arithmetic; tonnage.simulate_numpy gives the same bytes."""
    _require_gpu()
    lib = load_library()
    F, E, P = int(depth.shape[0]), int(area.shape[0]), int(pass_params.shape[0])
    for t_, dt, shape in ((entry_start, torch.int32, (F + 1,)), (area, torch.float64, (E,)), (err, torch.float64, (E, 2)), (flags, torch.uint8, (E,)),
                          (depth, torch.float64, (F,)), (pass_id, torch.int32, (F,)), (pass_params, torch.float64, (P, 6)), (moments, torch.float64, (F, 2))):
        if not t_.is_cuda or t_.dtype != dt or tuple(t_.shape) != shape or not t_.is_contiguous():
            raise ValueError(f"tonnage: a contiguous CUDA {dt} tensor of shape {shape} is needed, not {t_.dtype} {tuple(t_.shape)} on {t_.device}")
    K = int(K)
    ton = torch.empty((K, F), dtype=torch.float64, device=depth.device)
    T = torch.empty((K, P), dtype=torch.float64, device=depth.device)
    start_h = np.ascontiguousarray(entry_start.cpu().numpy() if entry_start_host is None else entry_start_host, dtype=np.int32)
    pp_h = np.ascontiguousarray(pass_params.cpu().numpy() if pass_params_host is None else pass_params_host, dtype=np.float64)
    if start_h.shape != (F + 1,) or pp_h.shape != (P, 6):
        raise ValueError(f"tonnage: host copies of shape {start_h.shape} and {pp_h.shape} for tables of shape {(F + 1,)} and {(P, 6)}")
    pr = np.ascontiguousarray(np.asarray(probs, np.float64).reshape(4))
    ptr = lambda t_: t_.data_ptr() if t_.numel() else None
    _check(lib.aq_tonnage_simulate_f64(int(seed), int(k0), K, entry_start.data_ptr(), start_h.ctypes.data, F, ptr(area), ptr(err), ptr(flags), E,
                                       ptr(depth), ptr(pass_id), ptr(pass_params), pp_h.ctypes.data, P, float(mix), float(min_depth),
                                       pr.ctypes.data, ptr(ton), _stream_ptr()))
    _check(lib.aq_tonnage_reduce_f64(ptr(ton), K, F, ptr(pass_id), P, ptr(T), ptr(moments), _stream_ptr()))
    for t_ in (entry_start, area, err, flags, depth, pass_id, pass_params, moments):
        t_.record_stream(torch.cuda.current_stream())
    return ton, T


def tonnage_ndtri(p: torch.Tensor) -> torch.Tensor:
    """aq_tonnage_ndtri_f64: the kernels' inverse normal distribution function of p (float64 CUDA [n])."""
    _require_gpu()
    p = p.contiguous()
    out = torch.empty_like(p)
    _check(load_library().aq_tonnage_ndtri_f64(p.data_ptr() if p.numel() else None, p.numel(), out.data_ptr() if p.numel() else None, _stream_ptr()))
    return out


def tonnage_uniform(seed: int, counters: torch.Tensor) -> torch.Tensor:
    """aq_tonnage_uniform_f64: the kernels' uniform draw of every counter (int32 CUDA [n, 4] holding the four unsigned words' bits)."""
    _require_gpu()
    counters = counters.contiguous()
    n = int(counters.shape[0])
    out = torch.empty(n, dtype=torch.float64, device=counters.device)
    _check(load_library().aq_tonnage_uniform_f64(int(seed), counters.data_ptr() if n else None, n, out.data_ptr() if n else None, _stream_ptr()))
    return out


# ---- --performance: aq_bernoulli_counts_i32 (the samples behind the population bound) ----

BERNOULLI_MAX_RATES = 16


def bernoulli_counts(seed: int, k0: int, K: int, S: int, rates, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """aq_bernoulli_counts_i32 on the current stream: int32 CUDA [K, R], row k the number of the S draws of simulation k0 + k that fall below
    each of the R rates (a sequence of doubles in [0, 1], at most 16); performance.counts_numpy gives the same bytes.  out = an int32 CUDA
    [K, R] tensor to write into (contiguous)."""
    _require_gpu()
    lib = load_library()
    rates_h = np.ascontiguousarray(np.asarray(rates, np.float64).reshape(-1))
    K, R = int(K), int(rates_h.shape[0])
    if K < 0:
        raise ValueError(f"population: {K} simulations")
    if out is None:
        out = torch.empty((K, R), dtype=torch.int32, device="cuda")
    elif not (out.is_cuda and out.dtype == torch.int32 and tuple(out.shape) == (K, R) and out.is_contiguous()):
        raise ValueError(f"population: a contiguous CUDA int32 tensor of shape {(K, R)} is needed, not {out.dtype} {tuple(out.shape)} on {out.device}")
    rates_d = torch.from_numpy(rates_h).to(out.device)
    _check(lib.aq_bernoulli_counts_i32(int(seed), int(k0), K, int(S), rates_d.data_ptr() if R else None, rates_h.ctypes.data if R else None, R,
                                       out.data_ptr() if out.numel() else None, _stream_ptr()))
    return out


# ---- --bathymetry: aq_depth_ranges_f64 / aq_depth_stats_f64 (the depth raster's cells under every facility's cages) ----

def depth_word_starts(windows: np.ndarray) -> np.ndarray:
    """int64 [F + 1]: the first bitmap word of every facility, (cells + 31) // 32 words each, from windows int32 [F, 4] (c0, c1, r0, r1)."""
    w = np.asarray(windows, np.int64).reshape(-1, 4)
    cells = np.maximum(w[:, 1] - w[:, 0] + 1, 0) * np.maximum(w[:, 3] - w[:, 2] + 1, 0)
    return np.ascontiguousarray(np.concatenate([[0], np.cumsum((cells + 31) // 32)]), dtype=np.int64)


def depth_stats(entry_start: torch.Tensor, cages: torch.Tensor, raster: torch.Tensor, x0: float, y0: float, dx: float, dy: float,
                nodata: Optional[float] = None, times: Optional[dict] = None) -> Tuple[torch.Tensor, torch.Tensor, np.ndarray]:
    """Both launches on the current stream: entry_start int32 CUDA [F + 1], cages float64 CUDA [E, 4] (lon_min, lon_max, lat_min, lat_max),
    raster float32 CUDA [nrows, ncols] with its north-west corner (x0, y0) and cell size (dx, dy); nodata None: no value is nodata ->
    (stats float64 CUDA [F, 3]: min, max, sum; count int64 CUDA [F]; windows int32 [F, 4] in host memory).  Between the launches the
    windows come back to the host, which lays out the bitmap (depth_word_starts) -- the one synchronisation.  include/aq_engine.h states
    the arithmetic; bathymetry.stats_numpy gives the same bytes.  times = a dict that receives "ranges_ms" and "stats_ms" (HIP events)
    and "bitmap_words"."""
    _require_gpu()
    lib = load_library()
    F, E = int(entry_start.shape[0]) - 1, int(cages.shape[0])
    for t_, dt, nd in ((entry_start, torch.int32, 1), (cages, torch.float64, 2), (raster, torch.float32, 2)):
        if not t_.is_cuda or t_.dtype != dt or t_.ndim != nd or not t_.is_contiguous():
            raise ValueError(f"depth: a contiguous CUDA {dt} tensor of {nd} dimensions is needed, not {t_.dtype} {tuple(t_.shape)} on {t_.device}")
    if F < 0 or tuple(cages.shape) != (E, 4):
        raise ValueError(f"depth: entry_start of shape {tuple(entry_start.shape)} and cages of shape {tuple(cages.shape)}")
    nrows, ncols = int(raster.shape[0]), int(raster.shape[1])
    dev = entry_start.device
    ranges = torch.empty((E, 4), dtype=torch.int32, device=dev)
    windows = torch.empty((F, 4), dtype=torch.int32, device=dev)
    stats = torch.empty((F, 3), dtype=torch.float64, device=dev)
    count = torch.empty((F,), dtype=torch.int64, device=dev)
    ptr = lambda t_: t_.data_ptr() if t_.numel() else None
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)] if times is not None else None
    if ev:
        ev[0].record()
    _check(lib.aq_depth_ranges_f64(entry_start.data_ptr(), F, ptr(cages), E, float(x0), float(y0), float(dx), float(dy), nrows, ncols, ptr(ranges),
                                   ptr(windows), _stream_ptr()))
    if ev:
        ev[1].record()
    win_h = np.ascontiguousarray(windows.cpu().numpy())
    start_h = depth_word_starts(win_h)
    words = int(start_h[-1])
    if words >= 1 << 31:
        raise ValueError(f"depth: a bitmap of {words} words for {F} facilities (fewer than 2^31 in one call): pass fewer facilities at a time")
    bitmap = torch.zeros(words, dtype=torch.int32, device=dev)
    start_d = torch.from_numpy(start_h).to(dev)
    if ev:
        ev[2].record()
    _check(lib.aq_depth_stats_f64(entry_start.data_ptr(), F, ptr(ranges), E, ptr(windows), win_h.ctypes.data, start_d.data_ptr(), start_h.ctypes.data,
                                  ptr(raster), nrows, ncols, float("nan") if nodata is None else float(nodata), ptr(bitmap), words, ptr(stats),
                                  ptr(count), _stream_ptr()))
    if ev:
        ev[3].record()
        ev[3].synchronize()
        times.update(ranges_ms=ev[0].elapsed_time(ev[1]), stats_ms=ev[2].elapsed_time(ev[3]), bitmap_words=words)
    for t_ in (entry_start, cages, raster, ranges, windows, start_d, bitmap, stats, count):
        t_.record_stream(torch.cuda.current_stream())
    return stats, count, win_h


# ---- --dedup-years: aq_dedup_fill_u32 / aq_dedup_sets_u32 / aq_dedup_select_f64 (one year's cages per tile and image pass) ----

DEDUP_MAX_SLOTS, DEDUP_MAX_PERMS = 5, 120
DEDUP_ABSENT, DEDUP_FULL, DEDUP_BITMAP = 0, 1, 2


def _dedup_tensor(name: str, t_: torch.Tensor, dt, shape) -> None:
    if not t_.is_cuda or t_.dtype != dt or not t_.is_contiguous() or any(b is not None and a != b for a, b in zip(t_.shape, shape)) or t_.ndim != len(shape):
        raise ValueError(f"dedup: {name} has to be a contiguous CUDA {dt} tensor of shape {shape}, not {t_.dtype} {tuple(t_.shape)} on {t_.device}")


def dedup_fill(ring_xy: torch.Tensor, ring_start: torch.Tensor, ring_frame: torch.Tensor, bitmap: torch.Tensor,
               ring_start_host: np.ndarray, ring_frame_host: np.ndarray) -> torch.Tensor:
    """aq_dedup_fill_u32 on the current stream: ring_xy int32 CUDA [V, 2], ring_start int32 CUDA [R + 1], ring_frame int32 CUDA [R, 4]
    (first word, w, h, 0), bitmap int32 CUDA [words], zeroed by the caller and filled in place; the *_host arrays hold the same tables in
    host memory (int32, contiguous).  include/aq_engine.h states the contract; dedup.fill_numpy gives the same bytes."""
    _require_gpu()
    V, R = int(ring_xy.shape[0]), int(ring_start.shape[0]) - 1
    for name, t_, dt, shape in (("ring_xy", ring_xy, torch.int32, (V, 2)), ("ring_start", ring_start, torch.int32, (R + 1,)),
                                ("ring_frame", ring_frame, torch.int32, (R, 4)), ("bitmap", bitmap, torch.int32, (None,))):
        _dedup_tensor(name, t_, dt, shape)
    rs, rf = np.ascontiguousarray(ring_start_host, dtype=np.int32), np.ascontiguousarray(ring_frame_host, dtype=np.int32)
    if rs.shape != (R + 1,) or rf.shape != (R, 4):
        raise ValueError("dedup: the host copies do not have the device tables' shapes")
    ptr = lambda t_: t_.data_ptr() if t_.numel() else None
    _check(load_library().aq_dedup_fill_u32(ptr(ring_xy), V, ptr(ring_start), rs.ctypes.data, ptr(ring_frame), rf.ctypes.data, R, ptr(bitmap),
                                            int(bitmap.shape[0]), _stream_ptr()))
    for t_ in (ring_xy, ring_start, ring_frame, bitmap):
        t_.record_stream(torch.cuda.current_stream())
    return bitmap


def dedup_sets(group: torch.Tensor, cage: torch.Tensor, bitmap: torch.Tensor, group_host: np.ndarray) -> torch.Tensor:
    """aq_dedup_sets_u32: group int32 CUDA [G, 16], cage int32 CUDA [C, 8], bitmap int32 CUDA [words] -> the cages' set words, int32 CUDA
    [C] (the uint32's bits).  dedup.sets_numpy gives the same bytes."""
    _require_gpu()
    G, Cn = int(group.shape[0]), int(cage.shape[0])
    for name, t_, dt, shape in (("group", group, torch.int32, (G, 16)), ("cage", cage, torch.int32, (Cn, 8)), ("bitmap", bitmap, torch.int32, (None,))):
        _dedup_tensor(name, t_, dt, shape)
    gh = np.ascontiguousarray(group_host, dtype=np.int32)
    if gh.shape != (G, 16):
        raise ValueError("dedup: the host copy does not have the group table's shape")
    words = torch.empty(Cn, dtype=torch.int32, device=cage.device)
    ptr = lambda t_: t_.data_ptr() if t_.numel() else None
    _check(load_library().aq_dedup_sets_u32(ptr(group), gh.ctypes.data, G, ptr(cage), Cn, ptr(bitmap), int(bitmap.shape[0]), ptr(words), _stream_ptr()))
    for t_ in (group, cage, bitmap, words):
        t_.record_stream(torch.cuda.current_stream())
    return words


def dedup_select(group: torch.Tensor, cage_start: torch.Tensor, cage: torch.Tensor, words: torch.Tensor, area: torch.Tensor,
                 random_order: torch.Tensor, group_host: np.ndarray, cage_start_host: np.ndarray) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """aq_dedup_select_f64: group int32 CUDA [G, 16], cage_start int32 CUDA [G + 1], cage int32 CUDA [C, 8], words int32 CUDA [C], area
    float64 CUDA [C], random_order int32 CUDA [G, 5] -> (sel uint8 CUDA [C], zero for the cages outside the G groups; chosen int32 CUDA
    [G, 4]: min, max, random, n!; sums float64 CUDA [G, 120]).  dedup.select_numpy gives the same bytes."""
    _require_gpu()
    G, Cn = int(group.shape[0]), int(cage.shape[0])
    for name, t_, dt, shape in (("group", group, torch.int32, (G, 16)), ("cage_start", cage_start, torch.int32, (G + 1,)), ("cage", cage, torch.int32, (Cn, 8)),
                                ("words", words, torch.int32, (Cn,)), ("area", area, torch.float64, (Cn,)), ("random_order", random_order, torch.int32, (G, 5))):
        _dedup_tensor(name, t_, dt, shape)
    gh, ch = np.ascontiguousarray(group_host, dtype=np.int32), np.ascontiguousarray(cage_start_host, dtype=np.int32)
    if gh.shape != (G, 16) or ch.shape != (G + 1,):
        raise ValueError("dedup: the host copies do not have the device tables' shapes")
    dev = group.device
    sel = torch.zeros(Cn, dtype=torch.uint8, device=dev)
    chosen = torch.empty((G, 4), dtype=torch.int32, device=dev)
    sums = torch.empty((G, DEDUP_MAX_PERMS), dtype=torch.float64, device=dev)
    ptr = lambda t_: t_.data_ptr() if t_.numel() else None
    _check(load_library().aq_dedup_select_f64(ptr(group), gh.ctypes.data, ptr(cage_start), ch.ctypes.data, G, ptr(cage), ptr(words), ptr(area), Cn,
                                              ptr(random_order), ptr(sel), ptr(chosen), ptr(sums), _stream_ptr()))
    for t_ in (group, cage_start, cage, words, area, random_order, sel, chosen, sums):
        t_.record_stream(torch.cuda.current_stream())
    return sel, chosen, sums


# ---- --tonnage-missing: aq_coverage_first_i32 (boxes against the union of a pass's image regions) ----

def _coverage_tensor(name: str, t_: torch.Tensor, dt, shape) -> None:
    if not t_.is_cuda or t_.dtype != dt or not t_.is_contiguous() or t_.ndim != len(shape) or any(b is not None and a != b for a, b in zip(t_.shape, shape)):
        raise ValueError(f"coverage: {name} has to be a contiguous CUDA {dt} tensor of shape {shape}, not {t_.dtype} {tuple(t_.shape)} on {t_.device}")


def coverage_first(rect: torch.Tensor, ring_start: torch.Tensor, xy: torch.Tensor, entry_img: torch.Tensor, band_start: torch.Tensor,
                   band: torch.Tensor, nbands: int, box: torch.Tensor, qpass: torch.Tensor, ring_start_host: np.ndarray,
                   band_start_host: np.ndarray, band_host: np.ndarray, times: Optional[dict] = None) -> torch.Tensor:
    """aq_coverage_first_i32 on the current stream: rect float64 CUDA [I, 4] (west, south, east, north), ring_start int32 CUDA [I + 1], xy
    float64 CUDA [V, 2], entry_img int32 CUDA [entries], band_start int32 CUDA [P nbands + 1], band float64 CUDA [P, 2] (Y0, h), box
    float64 CUDA [Q, 4], qpass int32 CUDA [Q]; the *_host arrays hold the same tables in host memory -> first int32 CUDA [Q].
    include/aq_engine.h states the contract; missing.first_numpy gives the same bytes.  times = a dict that receives "kernel_ms" (HIP
    events; the call then waits for them)."""
    _require_gpu()
    I, V, entries, P, Q = int(ring_start.shape[0]) - 1, int(xy.shape[0]), int(entry_img.shape[0]), int(band.shape[0]), int(box.shape[0])
    nbands = int(nbands)
    if I < 0 or nbands < 1:
        raise ValueError(f"coverage: ring_start of {I + 1} entries, nbands = {nbands}")
    for name, t_, dt, shape in (("rect", rect, torch.float64, (I, 4)), ("ring_start", ring_start, torch.int32, (I + 1,)), ("xy", xy, torch.float64, (V, 2)),
                                ("entry_img", entry_img, torch.int32, (entries,)), ("band_start", band_start, torch.int32, (P * nbands + 1,)),
                                ("band", band, torch.float64, (P, 2)), ("box", box, torch.float64, (Q, 4)), ("qpass", qpass, torch.int32, (Q,))):
        _coverage_tensor(name, t_, dt, shape)
    rs, bs = np.ascontiguousarray(ring_start_host, dtype=np.int32), np.ascontiguousarray(band_start_host, dtype=np.int32)
    bh = np.ascontiguousarray(band_host, dtype=np.float64)
    if rs.shape != (I + 1,) or bs.shape != (P * nbands + 1,) or bh.shape != (P, 2):
        raise ValueError("coverage: the host copies do not have the device tables' shapes")
    first = torch.empty(Q, dtype=torch.int32, device=box.device)
    scratch = torch.empty(entries * 32, dtype=torch.uint8, device=box.device)
    ptr = lambda t_: t_.data_ptr() if t_.numel() else None
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)] if times is not None else None
    if ev:
        ev[0].record()
    _check(load_library().aq_coverage_first_i32(ptr(rect), ptr(ring_start), rs.ctypes.data, I, ptr(xy), V, ptr(entry_img), entries, ptr(band_start),
                                                bs.ctypes.data, ptr(band), bh.ctypes.data if P else None, P, nbands, ptr(box), ptr(qpass), Q,
                                                ptr(scratch), scratch.numel(), ptr(first), _stream_ptr()))
    if ev:
        ev[1].record()
        ev[1].synchronize()
        times["kernel_ms"] = times.get("kernel_ms", 0.0) + ev[0].elapsed_time(ev[1])
    for t_ in (rect, ring_start, xy, entry_img, band_start, band, box, qpass, scratch, first):
        t_.record_stream(torch.cuda.current_stream())
    return first


# ---- --dedup-overlaps: aq_overlap_partners_f64, aq_overlap_clip_f64 (every cage once where the download boxes overlap) ----

def _overlap_tensor(name: str, t_: torch.Tensor, dt, shape) -> None:
    if not t_.is_cuda or t_.dtype != dt or not t_.is_contiguous() or t_.ndim != len(shape) or any(a != b for a, b in zip(t_.shape, shape)):
        raise ValueError(f"overlaps: {name} has to be a contiguous CUDA {dt} tensor of shape {shape}, not {t_.dtype} {tuple(t_.shape)} on {t_.device}")


def overlap_partners(boxes: torch.Tensor, entry_box: torch.Tensor, band_start: torch.Tensor, nbands: int, Y0: float, h: float,
                     times: Optional[dict] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """aq_overlap_partners_f64 on the current stream, both calls: boxes float64 CUDA [n, 4] (x0, y0, x1, y1) in file order, entry_box int32
    CUDA [entries] and band_start int32 CUDA [nbands + 1] from overlaps.band_table -> (start int64 CUDA [n + 1], partner int32 CUDA
    [start[n]]): box i's earlier partners, ascending, at partner[start[i] : start[i + 1]].  The list's size crosses to the host between the
    count and the fill.  include/aq_engine.h states the contract; overlaps.partners_numpy gives the same arrays.  times = a dict that
    receives "partners_ms" (HIP events around both calls, the host's wait for the size included)."""
    _require_gpu()
    n, entries, nbands = int(boxes.shape[0]), int(entry_box.shape[0]), int(nbands)
    for name, t_, dt, shape in (("boxes", boxes, torch.float64, (n, 4)), ("entry_box", entry_box, torch.int32, (entries,)),
                                ("band_start", band_start, torch.int32, (nbands + 1,))):
        _overlap_tensor(name, t_, dt, shape)
    lib = load_library()
    ptr = lambda t_: t_.data_ptr() if t_.numel() else None
    start = torch.empty(n + 1, dtype=torch.int64, device=boxes.device)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)] if times is not None else None
    if ev:
        ev[0].record()
    args = (ptr(boxes), n, ptr(entry_box), entries, ptr(band_start), nbands, float(Y0), float(h), start.data_ptr())
    _check(lib.aq_overlap_partners_f64(*args, None, 0, _stream_ptr()))
    total = int(start[n].item())
    partner = torch.empty(total, dtype=torch.int32, device=boxes.device)
    if total:
        _check(lib.aq_overlap_partners_f64(*args, partner.data_ptr(), total, _stream_ptr()))
    if ev:
        ev[1].record()
        ev[1].synchronize()
        times["partners_ms"] = times.get("partners_ms", 0.0) + ev[0].elapsed_time(ev[1])
    for t_ in (boxes, entry_box, band_start, start, partner):
        t_.record_stream(torch.cuda.current_stream())
    return start, partner


def overlap_clip(boxes: torch.Tensor, start: torch.Tensor, partner: torch.Tensor, det_row: torch.Tensor, dets: torch.Tensor,
                 times: Optional[dict] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """aq_overlap_clip_f64 on the current stream: boxes float64 CUDA [n, 4], (start int64 CUDA [n + 1], partner int32 CUDA [T]) the partner
    lists, det_row int32 CUDA [m] the detections' box rows, dets float64 CUDA [m, 4] -> (state uint8 CUDA [m], clip_bounds float64 CUDA
    [m, 4], clip_area float64 CUDA [m], has_region uint8 CUDA [n]).  overlaps.clip_numpy gives the same bytes.  times = a dict that
    receives "clip_ms" (HIP events; the call then waits for them)."""
    _require_gpu()
    n, T, m = int(boxes.shape[0]), int(partner.shape[0]), int(dets.shape[0])
    for name, t_, dt, shape in (("boxes", boxes, torch.float64, (n, 4)), ("start", start, torch.int64, (n + 1,)), ("partner", partner, torch.int32, (T,)),
                                ("det_row", det_row, torch.int32, (m,)), ("dets", dets, torch.float64, (m, 4))):
        _overlap_tensor(name, t_, dt, shape)
    dev = boxes.device
    state = torch.empty(m, dtype=torch.uint8, device=dev)
    bounds = torch.empty((m, 4), dtype=torch.float64, device=dev)
    area = torch.empty(m, dtype=torch.float64, device=dev)
    has_region = torch.empty(n, dtype=torch.uint8, device=dev)
    ptr = lambda t_: t_.data_ptr() if t_.numel() else None
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)] if times is not None else None
    if ev:
        ev[0].record()
    _check(load_library().aq_overlap_clip_f64(ptr(boxes), n, start.data_ptr(), ptr(partner), T, ptr(det_row), ptr(dets), m, ptr(state), ptr(bounds),
                                              ptr(area), ptr(has_region), _stream_ptr()))
    if ev:
        ev[1].record()
        ev[1].synchronize()
        times["clip_ms"] = times.get("clip_ms", 0.0) + ev[0].elapsed_time(ev[1])
    for t_ in (boxes, start, partner, det_row, dets, state, bounds, area, has_region):
        t_.record_stream(torch.cuda.current_stream())
    return state, bounds, area, has_region


# ---- --facility-sites: aq_facility_bounds_f64, aq_box_join_count_i32, aq_box_join_list_i32 (known and additional facilities) ----

def _sites_tensor(name: str, t_: torch.Tensor, dt, shape) -> None:
    if not t_.is_cuda or t_.dtype != dt or not t_.is_contiguous() or t_.ndim != len(shape) or any(a != b for a, b in zip(t_.shape, shape)):
        raise ValueError(f"facility sites: {name} has to be a contiguous CUDA {dt} tensor of shape {shape}, not {t_.dtype} {tuple(t_.shape)} on {t_.device}")


def facility_bounds(entry_start: torch.Tensor, entry_box: torch.Tensor, entry_use: torch.Tensor, entry_start_host: np.ndarray,
                    times: Optional[dict] = None) -> torch.Tensor:
    """aq_facility_bounds_f64 on the current stream: entry_start int32 CUDA [F + 1] (facility f owns the entries entry_start[f] ..
    entry_start[f + 1] - 1), entry_box float64 CUDA [E, 4] (x0, y0, x1, y1), entry_use uint8 CUDA [E] (0: the entry does not take part);
    entry_start_host holds the starts in host memory -> bounds float64 CUDA [F, 4]: the rectangle around the facility's entries that take
    part, four NaNs without one.  include/aq_engine.h states the contract; facility_sites.bounds_numpy gives the same bytes.  times = a dict
    that receives "bounds_ms" (HIP events; the call then waits for them)."""
    _require_gpu()
    F, E = int(entry_start.shape[0]) - 1, int(entry_box.shape[0])
    if F < 0:
        raise ValueError("facility sites: entry_start needs at least one entry")
    for name, t_, dt, shape in (("entry_start", entry_start, torch.int32, (F + 1,)), ("entry_box", entry_box, torch.float64, (E, 4)),
                                ("entry_use", entry_use, torch.uint8, (E,))):
        _sites_tensor(name, t_, dt, shape)
    es = np.ascontiguousarray(entry_start_host, dtype=np.int32)
    if es.shape != (F + 1,):
        raise ValueError("facility sites: the host copy does not have the entry starts' shape")
    bounds = torch.empty((F, 4), dtype=torch.float64, device=entry_start.device)
    ptr = lambda t_: t_.data_ptr() if t_.numel() else None
    ph = _Phases(times)
    ph.mark()
    _check(load_library().aq_facility_bounds_f64(ptr(entry_start), es.ctypes.data, F, ptr(entry_box), ptr(entry_use), E, ptr(bounds), _stream_ptr()))
    ph.done("bounds_ms")
    for t_ in (entry_start, entry_box, entry_use, bounds):
        t_.record_stream(torch.cuda.current_stream())
    return bounds


def box_join_keys(kbox: torch.Tensor, kgroup: torch.Tensor, G: int) -> dict:
    """The keys of box_join_count / box_join_list, sorted once for both: kbox float64 CUDA [N, 4], kgroup int32 CUDA [N] with ids in [0, G),
    in any order -> {"box": the boxes in box_match_sort's order, "kid" int32 [N]: their original rows, "start" int32 CUDA [G + 1],
    "start_host" the same in host memory, "N", "G"}."""
    _require_gpu()
    N, G = int(kbox.shape[0]), int(G)
    _sites_tensor("kbox", kbox, torch.float64, (N, 4))
    _sites_tensor("kgroup", kgroup, torch.int32, (N,))
    if G < 0 or (N and not (0 <= int(kgroup.min()) and int(kgroup.max()) < G)):
        raise ValueError(f"facility sites: the keys' group ids have to lie in [0, {G})")
    order, start = box_match_sort(kbox, kgroup, G)
    return {"box": kbox[order].contiguous(), "kid": order.to(torch.int32), "start": start.contiguous(),
            "start_host": np.ascontiguousarray(start.cpu().numpy(), dtype=np.int32), "N": N, "G": G}


def _box_join_queries(qbox: torch.Tensor, qgroup: torch.Tensor, kbox, kgroup, G, keys: Optional[dict]):
    _require_gpu()
    Q = int(qbox.shape[0])
    _sites_tensor("qbox", qbox, torch.float64, (Q, 4))
    _sites_tensor("qgroup", qgroup, torch.int32, (Q,))
    keys = box_join_keys(kbox, kgroup, G) if keys is None else keys
    ptr = lambda t_: t_.data_ptr() if t_.numel() else None
    args = (ptr(qbox), ptr(qgroup), Q, ptr(keys["box"]), ptr(keys["kid"]), keys["start"].data_ptr(), keys["start_host"].ctypes.data, keys["N"], keys["G"])
    return Q, keys, args


def box_join_count(qbox: torch.Tensor, qgroup: torch.Tensor, kbox: Optional[torch.Tensor] = None, kgroup: Optional[torch.Tensor] = None, G: int = 0,
                   keys: Optional[dict] = None, times: Optional[dict] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """aq_box_join_count_i32 on the current stream: qbox float64 CUDA [Q, 4] (x0, y0, x1, y1), qgroup int32 CUDA [Q], and the keys -- kbox,
    kgroup, G in any order, or keys = box_join_keys' result -> (count int32 CUDA [Q]: the keys of the query's group whose closed box meets
    the query's; first int32 CUDA [Q]: the smallest row among them, -1 without one).  facility_sites.join_count_numpy gives the same bytes.
    times = a dict that receives "count_ms"."""
    Q, keys, args = _box_join_queries(qbox, qgroup, kbox, kgroup, G, keys)
    count = torch.empty(Q, dtype=torch.int32, device=qbox.device)
    first = torch.empty(Q, dtype=torch.int32, device=qbox.device)
    ph = _Phases(times)
    ph.mark()
    _check(load_library().aq_box_join_count_i32(*args, count.data_ptr() if Q else None, first.data_ptr() if Q else None, _stream_ptr()))
    ph.done("count_ms")
    for t_ in (qbox, qgroup, keys["box"], keys["kid"], keys["start"], count, first):
        t_.record_stream(torch.cuda.current_stream())
    return count, first


def box_join_list(qbox: torch.Tensor, qgroup: torch.Tensor, kbox: Optional[torch.Tensor] = None, kgroup: Optional[torch.Tensor] = None, G: int = 0,
                  keys: Optional[dict] = None, count: Optional[torch.Tensor] = None, times: Optional[dict] = None) -> Tuple[np.ndarray, torch.Tensor]:
    """aq_box_join_list_i32 on the current stream, after box_join_count (count = its first result, computed here when not given): the
    same arguments -> (offset int64 [Q + 1] in host memory: the exclusive scan of the counts; list int32 CUDA [offset[Q]]: the rows of the
    keys that meet query q at list[offset[q] : offset[q + 1]], in the order of the sorted keys).  The counts cross to the host between the
    two launches.  facility_sites.join_list_numpy gives the same arrays.  times = a dict that receives "list_ms" (and "count_ms")."""
    Q, keys, args = _box_join_queries(qbox, qgroup, kbox, kgroup, G, keys)
    if count is None:
        count = box_join_count(qbox, qgroup, keys=keys, times=times)[0]
    _sites_tensor("count", count, torch.int32, (Q,))
    offset_h = np.zeros(Q + 1, np.int64)
    np.cumsum(count.cpu().numpy(), dtype=np.int64, out=offset_h[1:])
    total = int(offset_h[-1])
    if total >= 1 << 31:
        raise ValueError(f"facility sites: {total} list entries (fewer than 2^31 in one call): pass fewer queries at a time")
    offset = torch.from_numpy(offset_h).to(qbox.device)
    out = torch.empty(total, dtype=torch.int32, device=qbox.device)
    ph = _Phases(times)
    ph.mark()
    _check(load_library().aq_box_join_list_i32(*args, offset.data_ptr(), offset_h.ctypes.data, out.data_ptr() if total else None, total, _stream_ptr()))
    ph.done("list_ms")
    for t_ in (qbox, qgroup, keys["box"], keys["kid"], keys["start"], offset, out):
        t_.record_stream(torch.cuda.current_stream())
    return offset_h, out


# ---- yolov5/val.py: aq_val_expand_rows_f32, aq_val_match, aq_val_confusion, aq_val_scores_f64 (mAP and class confusion against YOLO labels) ----

VAL_NMS_ROWS = 131071                      # aq_nms takes fewer than 131072 rows per image


def _val_tensor(name: str, t_: torch.Tensor, dt, shape) -> None:
    if not t_.is_cuda or t_.dtype != dt or not t_.is_contiguous() or t_.ndim != len(shape) or any(a != b for a, b in zip(t_.shape, shape)):
        raise ValueError(f"val: {name} has to be a contiguous CUDA {dt} tensor of shape {shape}, not {t_.dtype} {tuple(t_.shape)} on {t_.device}")


def val_expand_rows(pred: torch.Tensor, conf_thres: float, M: Optional[int] = None, rows: Optional[torch.Tensor] = None,
                    counts: Optional[torch.Tensor] = None, scratch: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """aq_val_expand_rows_f32 on the current stream: pred float32 CUDA [B, N, 5 + nc] -> (rows float32 CUDA [B, M, 5 + nc], counts int32 CUDA
    [B]): upstream's multi_label candidates, one row per (source row, class) that passes, in that order, for ``nms`` in full-rows mode; M
    defaults to min(N nc, 131071).  counts holds the rows emitted per image whatever M is; when one exceeds M, rows is not written at all.
    val.expand_rows_numpy gives the same bytes."""
    _require_gpu()
    lib = load_library()
    if pred.dim() != 3 or pred.shape[2] < 6:
        raise ValueError("val: pred has to be [B, N, 5 + nc] with nc >= 1")
    B, N, no = (int(v) for v in pred.shape)
    nc = no - 5
    _val_tensor("pred", pred, torch.float32, (B, N, no))
    M = min(N * nc, VAL_NMS_ROWS) if M is None else int(M)
    if rows is None:
        rows = torch.empty((B, max(M, 0), no), dtype=torch.float32, device=pred.device)
    if counts is None:
        counts = torch.empty((B,), dtype=torch.int32, device=pred.device)
    _val_tensor("rows", rows, torch.float32, (B, M, no))
    _val_tensor("counts", counts, torch.int32, (B,))
    need = int(lib.aq_val_expand_scratch_bytes(B, N, nc))
    if scratch is None or scratch.numel() < need:
        scratch = torch.empty(max(need, 4), dtype=torch.uint8, device=pred.device)
    _check(lib.aq_val_expand_rows_f32(pred.data_ptr(), B, N, nc, float(conf_thres), M, scratch.data_ptr(), scratch.numel(),
                                      rows.data_ptr() if rows.numel() else None, counts.data_ptr(), _stream_ptr()))
    for t_ in (pred, rows, counts, scratch):
        t_.record_stream(torch.cuda.current_stream())
    return rows, counts


def val_match(dets: torch.Tensor, counts: torch.Tensor, label_box: torch.Tensor, label_cls: torch.Tensor, label_start: torch.Tensor,
              label_start_host: np.ndarray, geom: torch.Tensor, iouv: np.ndarray, out_conf: torch.Tensor, out_cls: torch.Tensor,
              out_bits: torch.Tensor, total: torch.Tensor, scratch: Optional[torch.Tensor] = None) -> None:
    """aq_val_match on the current stream: dets float32 CUDA [B, max_det, 6] and counts int32 CUDA [B] as ``nms`` returns them; label_box
    float32 CUDA [L, 4] (original pixels), label_cls int32 CUDA [L], label_start int32 CUDA [B + 1] and its host copy; geom float32 CUDA
    [B, 5] = (pad x, pad y, gain, w0, h0); iouv float32 [10] in host memory.  Appends the batch's detections to out_conf float32, out_cls
    int32 and out_bits int16 (the uint16 words) CUDA [cap] at total int64 CUDA [1], which it advances.  val.match_numpy gives the same values."""
    _require_gpu()
    if dets.dim() != 3 or dets.shape[2] != 6:
        raise ValueError("val: dets has to be [B, max_det, 6]")
    B, max_det = int(dets.shape[0]), int(dets.shape[1])
    L, cap = int(label_box.shape[0]), int(out_conf.shape[0])
    for name, t_, dt, shape in (("dets", dets, torch.float32, (B, max_det, 6)), ("counts", counts, torch.int32, (B,)),
                                ("label_box", label_box, torch.float32, (L, 4)), ("label_cls", label_cls, torch.int32, (L,)),
                                ("label_start", label_start, torch.int32, (B + 1,)), ("geom", geom, torch.float32, (B, 5)),
                                ("out_conf", out_conf, torch.float32, (cap,)), ("out_cls", out_cls, torch.int32, (cap,)),
                                ("out_bits", out_bits, torch.int16, (cap,)), ("total", total, torch.int64, (1,))):
        _val_tensor(name, t_, dt, shape)
    ls = np.ascontiguousarray(label_start_host, dtype=np.int32)
    iou = np.ascontiguousarray(iouv, dtype=np.float32)
    if ls.shape != (B + 1,) or iou.shape != (10,):
        raise ValueError("val: label_start_host has to hold B + 1 starts and iouv ten thresholds")
    if scratch is None or scratch.numel() < 10 * L:
        scratch = torch.empty(max(10 * L, 1), dtype=torch.int32, device=dets.device)
    ptr = lambda t_: t_.data_ptr() if t_.numel() else None
    _check(load_library().aq_val_match(ptr(dets), ptr(counts), B, max_det, ptr(label_box), ptr(label_cls), label_start.data_ptr(), ls.ctypes.data, L,
                                       ptr(geom), iou.ctypes.data, scratch.data_ptr(), ptr(out_conf), ptr(out_cls), ptr(out_bits), cap, total.data_ptr(),
                                       _stream_ptr()))
    for t_ in (dets, counts, label_box, label_cls, label_start, geom, out_conf, out_cls, out_bits, total, scratch):
        t_.record_stream(torch.cuda.current_stream())


def val_confusion(dets: torch.Tensor, counts: torch.Tensor, label_box: torch.Tensor, label_cls: torch.Tensor, label_start: torch.Tensor,
                  label_start_host: np.ndarray, geom: torch.Tensor, nc: int, conf: float, iou: float, matrix: torch.Tensor,
                  image: Optional[torch.Tensor] = None, label_cls_host: Optional[np.ndarray] = None, flag: Optional[torch.Tensor] = None,
                  scratch: Optional[torch.Tensor] = None) -> torch.Tensor:
    """aq_val_confusion on the current stream: the arguments of val_match up to geom, then nc, the confidence and the IoU threshold.  Adds
    the batch to matrix int64 CUDA [nc + 1, nc + 1] ([predicted][true], index nc = background) and returns image int32 CUDA [B, 4] =
    (labels, detections that take part, kept pairs, kept pairs of equal classes).  label_cls_host: the host copy of label_cls, checked
    against nc before the launch.  flag int32 CUDA [1] (zeroed by the caller) is set when an image holds a class outside [0, nc) and adds
    nothing; without it the call waits for the kernel and raises.  val.confusion_numpy gives the same values."""
    _require_gpu()
    lib = load_library()
    if dets.dim() != 3 or dets.shape[2] != 6:
        raise ValueError("val: dets has to be [B, max_det, 6]")
    B, max_det = int(dets.shape[0]), int(dets.shape[1])
    L, nc = int(label_box.shape[0]), int(nc)
    if image is None:
        image = torch.empty((B, 4), dtype=torch.int32, device=dets.device)
    own_flag = flag is None
    if own_flag:
        flag = torch.zeros(1, dtype=torch.int32, device=dets.device)
    for name, t_, dt, shape in (("dets", dets, torch.float32, (B, max_det, 6)), ("counts", counts, torch.int32, (B,)),
                                ("label_box", label_box, torch.float32, (L, 4)), ("label_cls", label_cls, torch.int32, (L,)),
                                ("label_start", label_start, torch.int32, (B + 1,)), ("geom", geom, torch.float32, (B, 5)),
                                ("matrix", matrix, torch.int64, (max(nc, 0) + 1, max(nc, 0) + 1)), ("image", image, torch.int32, (B, 4)),
                                ("flag", flag, torch.int32, (1,))):
        _val_tensor(name, t_, dt, shape)
    ls = np.ascontiguousarray(label_start_host, dtype=np.int32)
    if ls.shape != (B + 1,):
        raise ValueError("val: label_start_host has to hold B + 1 starts")
    lc = None if label_cls_host is None else np.ascontiguousarray(label_cls_host, dtype=np.int32)
    if lc is not None and lc.shape != (L,):
        raise ValueError("val: label_cls_host has to hold one class per label")
    need = int(lib.aq_val_confusion_scratch_bytes(B, max_det, L))
    if scratch is None or scratch.numel() < need:
        scratch = torch.empty(max(need, 8), dtype=torch.uint8, device=dets.device)
    ptr = lambda t_: t_.data_ptr() if t_.numel() else None
    _check(lib.aq_val_confusion(ptr(dets), ptr(counts), B, max_det, ptr(label_box), ptr(label_cls), lc.ctypes.data if lc is not None and L else None,
                                label_start.data_ptr(), ls.ctypes.data, L, ptr(geom), nc, float(conf), float(iou), scratch.data_ptr(),
                                scratch.numel(), matrix.data_ptr(), ptr(image), flag.data_ptr(), _stream_ptr()))
    for t_ in (dets, counts, label_box, label_cls, label_start, geom, matrix, image, flag, scratch):
        t_.record_stream(torch.cuda.current_stream())
    if own_flag and int(flag.item()):
        raise RuntimeError(f"val: a detection or label class outside [0, {nc}): the image added nothing to the confusion matrix")
    return image


def val_score_runs(run_range: np.ndarray) -> np.ndarray:
    """run_chunk0 int32 [C + 1] of aq_val_scores_f64: the exclusive scan of the runs' chunk counts."""
    ch = int(load_library().aq_val_score_chunk())
    rr = np.asarray(run_range, dtype=np.int64).reshape(-1, 2)
    out = np.zeros(rr.shape[0] + 1, np.int64)
    np.cumsum((rr[:, 1] - rr[:, 0] + ch - 1) // ch, out=out[1:])
    if out[-1] >= 1 << 31:
        raise ValueError("val: more than 2^31 chunks")
    return out.astype(np.int32)


def val_scores(bits: torch.Tensor, conf: torch.Tensor, run_range: np.ndarray, n_l: np.ndarray, x: np.ndarray, px: np.ndarray,
               times: Optional[dict] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """aq_val_scores_f64 on the current stream: bits int16 CUDA [n] (the uint16 words) and conf float32 CUDA [n], sorted by (class,
    -confidence, index); run_range int64 [C, 2] and n_l int32 [C] in host memory: the run and the label count of every class that has
    labels; x float64 [nx] and px float64 [npx] in host memory -> (ap [C, 10], p [C, npx], r [C, npx], pr [C, npx]) float64 CUDA.
    val.scores_numpy gives the same bytes.  times = a dict that receives "scores_ms"."""
    _require_gpu()
    lib = load_library()
    n = int(bits.shape[0])
    _val_tensor("bits", bits, torch.int16, (n,))
    _val_tensor("conf", conf, torch.float32, (n,))
    dev = bits.device
    rr = np.ascontiguousarray(run_range, dtype=np.int64).reshape(-1, 2)
    C_ = int(rr.shape[0])
    nl = np.ascontiguousarray(n_l, dtype=np.int32)
    xs, pxs = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(px, dtype=np.float64)
    if nl.shape != (C_,):
        raise ValueError("val: n_l has to hold one label count per run")
    rc0 = val_score_runs(rr)
    up = lambda a: torch.from_numpy(a).to(dev) if a.size else torch.empty(0, dtype=torch.from_numpy(a).dtype, device=dev)
    rr_d, nl_d, rc0_d, x_d, px_d = up(rr), up(nl), up(rc0), up(xs), up(pxs)
    need = int(lib.aq_val_scores_scratch_bytes(n, int(rc0[-1])))
    scratch = torch.empty(max(need, 8), dtype=torch.uint8, device=dev)
    ap = torch.empty((C_, 10), dtype=torch.float64, device=dev)
    p, r, pr = (torch.empty((C_, pxs.shape[0]), dtype=torch.float64, device=dev) for _ in range(3))
    ptr = lambda t_: t_.data_ptr() if t_.numel() else None
    ph = _Phases(times)
    ph.mark()
    _check(lib.aq_val_scores_f64(ptr(bits), ptr(conf), n, ptr(rr_d), rr.ctypes.data, ptr(nl_d), rc0_d.data_ptr(), rc0.ctypes.data, C_,
                                 x_d.data_ptr(), int(xs.shape[0]), px_d.data_ptr(), int(pxs.shape[0]), scratch.data_ptr(), scratch.numel(),
                                 ptr(ap), ptr(p), ptr(r), ptr(pr), _stream_ptr()))
    ph.done("scores_ms")
    for t_ in (bits, conf, rr_d, nl_d, rc0_d, x_d, px_d, scratch, ap, p, r, pr):
        t_.record_stream(torch.cuda.current_stream())
    return ap, p, r, pr


# ---- --land-filter: aq_land_filter_f64 (detection boxes against the segments of the land polygons) ----

LAND_MAX_BANDS = 65536                     # default band count: min(this, max(1, E // 8))


def _land_bands(y: torch.Tensor, y0: torch.Tensor, h: torch.Tensor) -> torch.Tensor:
    """floor((y - Y0) / h) as float64, unclamped: the kernel's expression.  y0 and h are 0-dim tensors on y's device, so that the division is a
    division (with a Python number torch multiplies by the reciprocal on the GPU, which rounds differently at a band's edge)."""
    return torch.floor((y - y0) / h)


def land_band_table(segs: torch.Tensor, band_height: Optional[float] = None) -> Tuple[torch.Tensor, torch.Tensor, int, float, float]:
    """The band table aq_land_filter_f64 takes: segs float64 [E, 4] (ax, ay, bx, by), E >= 1, on any device -> (entry_seg int32 [entries],
    band_start int32 [nbands + 1], nbands, Y0, h).  Y0 = the smallest y; band(y) = floor((y - Y0) / h); nbands = band(largest y) + 1, so no
    segment is clamped; every segment is entered in each band from band(min y) to band(max y); the entries are sorted by band (stable: by
    segment inside a band).  band_height = None: the y-extent divided by min(65536, max(1, E // 8)), doubled until there are at most
    8 E + nbands entries (long segments across many thin bands); a given band_height is taken as it is.  2^31 entries or more raise."""
    assert segs.dtype == torch.float64 and segs.ndim == 2 and segs.shape[1] == 4 and segs.shape[0] >= 1
    E = segs.shape[0]
    ylo, yhi = torch.minimum(segs[:, 1], segs[:, 3]), torch.maximum(segs[:, 1], segs[:, 3])
    y0_t, top_t = ylo.min(), yhi.max()
    Y0, top = float(y0_t), float(top_t)
    if not (np.isfinite(Y0) and np.isfinite(top) and bool(torch.isfinite(segs).all())):
        raise ValueError("land filter: a segment coordinate is not finite")
    if band_height is None:
        h = (top - Y0) / min(LAND_MAX_BANDS, max(1, E // 8))
        if not h > 0:
            h = 1.0                                         # every segment on one horizontal line: one band
    else:
        h = float(band_height)
        if not (h > 0 and np.isfinite(h)):
            raise ValueError(f"land filter: band height = {band_height} (it has to be positive and finite)")
    while True:
        h_t = torch.tensor(h, dtype=torch.float64, device=segs.device)
        lo, hi = _land_bands(ylo, y0_t, h_t), _land_bands(yhi, y0_t, h_t)
        nbands_f = float(hi.max()) + 1.0
        entries_f = float((hi - lo + 1.0).sum())            # (whole numbers in fp64: exact far beyond 2^31)
        if band_height is not None or entries_f <= 8 * E + nbands_f:
            break
        h *= 2.0
    if nbands_f >= 2.0 ** 31 or entries_f >= 2.0 ** 31:
        raise ValueError(f"land filter: {entries_f:.0f} band entries in {nbands_f:.0f} bands of {h:g} m for {E} segments (fewer than 2^31 "
                         f"of each in one call): use a larger band height")
    nbands, entries = int(nbands_f), int(entries_f)
    counts = (hi - lo).to(torch.int64) + 1
    seg_of = torch.repeat_interleave(torch.arange(E, device=segs.device), counts)
    first = torch.cumsum(counts, 0) - counts
    band_of = lo.to(torch.int64)[seg_of] + (torch.arange(entries, device=segs.device) - first[seg_of])
    band_sorted, order = torch.sort(band_of, stable=True)
    band_start = torch.searchsorted(band_sorted, torch.arange(nbands + 1, device=segs.device))
    return seg_of[order].to(torch.int32), band_start.to(torch.int32), nbands, Y0, h


def land_flags(boxes: torch.Tensor, segs: torch.Tensor, band_height: Optional[float] = None, times: Optional[dict] = None) -> torch.Tensor:
    """aq_land_filter_f64 on the current stream: boxes float64 CUDA [N, 4] (x0, y0, x1, y1; x0 <= x1, y0 <= y1), segs float64 CUDA [E, 4]
    (ax, ay, bx, by: every edge of every ring of the land) -> uint8 CUDA [N]: bit 0 = an edge meets the closed box, bit 1 = the corner
    (x0, y0) is inside the land; not 0 = on land (land.land_flags_numpy gives the same bytes).  The band table is torch's
    (land_band_table), the gather and the tests are the kernels'.  times = a dict that receives "table_ms" and "kernel_ms" (HIP events; the
    call then waits for them), "entries", "nbands" and "band_height"."""
    _require_gpu()
    lib = load_library()
    assert boxes.is_cuda and segs.is_cuda and boxes.dtype == torch.float64 and segs.dtype == torch.float64
    assert boxes.ndim == 2 and boxes.shape[1] == 4 and segs.ndim == 2 and segs.shape[1] == 4
    boxes, segs = boxes.contiguous(), segs.contiguous()
    N, E = boxes.shape[0], segs.shape[0]
    flags = torch.empty(N, dtype=torch.uint8, device=boxes.device)
    if N == 0 or E == 0:
        _check(lib.aq_land_filter_f64(None, E, None, 0, None, 1, 0.0, 1.0, None, N, None, 0, flags.data_ptr(), _stream_ptr()))
        flags.record_stream(torch.cuda.current_stream())
        return flags
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)] if times is not None else None
    if ev:
        ev[0].record()
    entry_seg, band_start, nbands, Y0, h = land_band_table(segs, band_height)
    entries = entry_seg.shape[0]
    scratch = torch.empty(int(lib.aq_land_scratch_bytes(entries)), dtype=torch.uint8, device=boxes.device)
    if ev:
        ev[1].record()
    _check(lib.aq_land_filter_f64(segs.data_ptr(), E, entry_seg.data_ptr(), entries, band_start.data_ptr(), nbands, Y0, h, boxes.data_ptr(), N,
                                  scratch.data_ptr(), scratch.numel(), flags.data_ptr(), _stream_ptr()))
    if ev:
        ev[2].record()
        ev[2].synchronize()
        times.update(table_ms=ev[0].elapsed_time(ev[1]), kernel_ms=ev[1].elapsed_time(ev[2]), entries=entries, nbands=nbands, band_height=h)
    for t_ in (boxes, segs, entry_seg, band_start, scratch, flags):
        t_.record_stream(torch.cuda.current_stream())
    return flags


def land_images(rects: torch.Tensor, segs: torch.Tensor, indent: float, band_height: Optional[float] = None,
                times: Optional[dict] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """aq_land_images_f64 on the current stream: rects float64 CUDA [N, 4] (x0, y0, x1, y1; x0 <= x1, y0 <= y1), segs float64 CUDA [E, 4] (as
    land_flags takes them), indent > 0 in metres -> (flags uint8 CUDA [N], dist2 float64 CUDA [N]): dist2 = the squared distance from the
    rectangle to the nearest land edge, capped at (2 indent)^2; bit 0 = dist2 < indent^2, bit 1 = the corner (x0, y0) is inside the land;
    2 = the image lies wholly on land, at least `indent` from the coast (land.land_images_numpy gives the same bytes and doubles).  The band
    table is land_band_table's, as for land_flags; neither output depends on its band height.  times = as for land_flags."""
    _require_gpu()
    lib = load_library()
    assert rects.is_cuda and segs.is_cuda and rects.dtype == torch.float64 and segs.dtype == torch.float64
    assert rects.ndim == 2 and rects.shape[1] == 4 and segs.ndim == 2 and segs.shape[1] == 4
    indent = float(indent)
    if not (indent > 0 and np.isfinite(indent)):
        raise ValueError(f"land images: indent = {indent} (it has to be positive and finite)")
    rects, segs = rects.contiguous(), segs.contiguous()
    N, E = rects.shape[0], segs.shape[0]
    flags = torch.empty(N, dtype=torch.uint8, device=rects.device)
    dist2 = torch.empty(N, dtype=torch.float64, device=rects.device)
    if N == 0 or E == 0:
        _check(lib.aq_land_images_f64(None, E, None, 0, None, 1, 0.0, 1.0, None, N, indent, None, 0, flags.data_ptr(), dist2.data_ptr(), _stream_ptr()))
        for t_ in (flags, dist2):
            t_.record_stream(torch.cuda.current_stream())
        return flags, dist2
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)] if times is not None else None
    if ev:
        ev[0].record()
    entry_seg, band_start, nbands, Y0, h = land_band_table(segs, band_height)
    entries = entry_seg.shape[0]
    scratch = torch.empty(int(lib.aq_land_images_scratch_bytes(entries)), dtype=torch.uint8, device=rects.device)
    if ev:
        ev[1].record()
    _check(lib.aq_land_images_f64(segs.data_ptr(), E, entry_seg.data_ptr(), entries, band_start.data_ptr(), nbands, Y0, h, rects.data_ptr(), N, indent,
                                  scratch.data_ptr(), scratch.numel(), flags.data_ptr(), dist2.data_ptr(), _stream_ptr()))
    if ev:
        ev[2].record()
        ev[2].synchronize()
        times.update(table_ms=ev[0].elapsed_time(ev[1]), kernel_ms=ev[1].elapsed_time(ev[2]), entries=entries, nbands=nbands, band_height=h)
    for t_ in (rects, segs, entry_seg, band_start, scratch, flags, dist2):
        t_.record_stream(torch.cuda.current_stream())
    return flags, dist2


def stem_conv_nhwc(tiles_u8: torch.Tensor, w_oihw: torch.Tensor, bias: torch.Tensor, act: bool = True, precision: str = "bf16") -> torch.Tensor:
    """uint8 [B,H,W,3] -> SiLU(conv6x6/s2/p2(x / 255, w) + b) as NHWC [B,H/2,W/2,cout] through aq_stem_conv (tests)."""
    _require_gpu()
    lib = load_library()
    prec = PRECISIONS[precision]
    B, H, W, _ = tiles_u8.shape
    cout = w_oihw.shape[0]
    w = np.ascontiguousarray(w_oihw.permute(0, 2, 3, 1).float().cpu().numpy())
    n = C.c_size_t()
    wp = w.ctypes.data_as(C.POINTER(C.c_float))
    _check(lib.aq_pack_stem_weights(wp, cout, prec, None, C.byref(n), None))
    wbuf = torch.empty(n.value, dtype=torch.uint8, device=tiles_u8.device)
    _check(lib.aq_pack_stem_weights(wp, cout, prec, wbuf.data_ptr(), C.byref(n), _stream_ptr()))
    bbuf = torch.zeros(64, dtype=torch.float32, device=tiles_u8.device)
    bbuf[:cout] = bias.float().to(tiles_u8.device)
    out = torch.empty((B, H // 2, W // 2, cout), dtype=_act_dtype(prec), device=tiles_u8.device)
    _check(lib.aq_stem_conv(tiles_u8.data_ptr(), out.data_ptr(), cout, 0, cout, wbuf.data_ptr(), bbuf.data_ptr(), B, H, W, int(act), prec,
                            _stream_ptr()))
    torch.cuda.current_stream().synchronize()
    return out


def bottleneck_nhwc(x: torch.Tensor, w1_oihw: torch.Tensor, b1: torch.Tensor, w2_oihw: torch.Tensor, b2: torch.Tensor,
                    shortcut: bool = True, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """bf16 NHWC [B,H,W,C] (may be a channel slice of a wider tensor) -> x + SiLU(conv3x3(SiLU(conv1x1(x)))) through
    aq_bottleneck (tests).  ``out`` may be a channel slice too; it must not overlap ``x``."""
    _require_gpu()
    lib = load_library()
    assert x.dtype == torch.bfloat16 and x.stride(3) == 1
    B, H, W, c = x.shape
    ld = x.stride(2)
    assert x.stride(1) == W * ld and x.stride(0) == H * W * ld, "x must be a channel slice of a dense NHWC tensor"
    w1 = np.ascontiguousarray(w1_oihw.permute(0, 2, 3, 1).float().cpu().numpy())
    w2 = np.ascontiguousarray(w2_oihw.permute(0, 2, 3, 1).float().cpu().numpy())
    n = C.c_size_t()
    p1, p2 = w1.ctypes.data_as(C.POINTER(C.c_float)), w2.ctypes.data_as(C.POINTER(C.c_float))
    _check(lib.aq_pack_bottleneck_weights(p1, p2, c, None, C.byref(n), None))
    wbuf = torch.empty(n.value, dtype=torch.uint8, device=x.device)
    _check(lib.aq_pack_bottleneck_weights(p1, p2, c, wbuf.data_ptr(), C.byref(n), _stream_ptr()))
    bbuf = torch.cat([b1.float(), b2.float()]).to(x.device).contiguous()
    if out is None:
        out = torch.empty((B, H, W, c), dtype=torch.bfloat16, device=x.device)
    old = out.stride(2)
    # data_ptr() of a channel slice already points at its first channel: pass ch_off = 0 with the parent's row length
    _check(lib.aq_bottleneck(x.data_ptr(), ld, 0, out.data_ptr(), old, 0, c, wbuf.data_ptr(), bbuf.data_ptr(), B, H, W, int(shortcut),
                             _stream_ptr()))
    torch.cuda.current_stream().synchronize()
    return out


def pack_bottleneck_c3tail(w1_oihw: torch.Tensor, b1: torch.Tensor, w2_oihw: torch.Tensor, b2: torch.Tensor, w3_oihw: torch.Tensor,
                           b3: torch.Tensor, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """(weight image, b1 | b2 | b3) of aq_bottleneck_c3tail: a C3 block's last Bottleneck (C = 48) and its cv3 1x1 (96 -> 96) (tests)."""
    lib = load_library()
    ws = [np.ascontiguousarray(w.permute(0, 2, 3, 1).float().cpu().numpy()) for w in (w1_oihw, w2_oihw, w3_oihw)]
    ps = [w.ctypes.data_as(C.POINTER(C.c_float)) for w in ws]
    n = C.c_size_t()
    _check(lib.aq_pack_bottleneck_c3tail_weights(*ps, None, C.byref(n), None))
    wbuf = torch.empty(n.value, dtype=torch.uint8, device=device)
    _check(lib.aq_pack_bottleneck_c3tail_weights(*ps, wbuf.data_ptr(), C.byref(n), _stream_ptr()))
    return wbuf, torch.cat([b1.float(), b2.float(), b3.float()]).to(device).contiguous()


def bottleneck_c3tail_supported(B: int, H: int, W: int, in_ld: int = 48, cat_ld: int = 96, out_ld: int = 96) -> bool:
    return bool(load_library().aq_bottleneck_c3tail_supported(B, H, W, in_ld, cat_ld, out_ld))


def bottleneck_c3tail_nhwc(x: torch.Tensor, c: torch.Tensor, packed: Tuple[torch.Tensor, torch.Tensor], shortcut: bool = True,
                           out: Optional[torch.Tensor] = None, sync: bool = True) -> torch.Tensor:
    """bf16 NHWC x [B,H,W,48] and cv2's output c [B,H,W,48] (channel slices of dense tensors) -> SiLU(W3 [Bottleneck(x) | c] + b3)
    [B,H,W,96] through aq_bottleneck_c3tail, on the current stream (tests, tools/time_c3tail.py).  ``packed``: pack_bottleneck_c3tail."""
    _require_gpu()
    lib = load_library()
    assert x.dtype == torch.bfloat16 and c.dtype == torch.bfloat16 and x.stride(3) == 1 and c.stride(3) == 1
    B, H, W, _ = x.shape
    if out is None:
        out = torch.empty((B, H, W, 96), dtype=torch.bfloat16, device=x.device)
    # data_ptr() of a channel slice already points at its first channel: ch_off = 0 with the parent's row length
    _check(lib.aq_bottleneck_c3tail(x.data_ptr(), x.stride(2), 0, c.data_ptr(), c.stride(2), 0, out.data_ptr(), out.stride(2), 0,
                                    packed[0].data_ptr(), packed[1].data_ptr(), B, H, W, int(shortcut), _stream_ptr()))
    if sync:
        torch.cuda.current_stream().synchronize()
    return out


def downblock_nhwc(x: torch.Tensor, wa_oihw: torch.Tensor, ba: torch.Tensor, wb_oihw: torch.Tensor, bb: torch.Tensor,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """bf16 NHWC [B,H,W,48] (may be a channel slice) -> SiLU(conv1x1(SiLU(conv3x3/s2(x)))) [B,H/2,W/2,96] through aq_downblock (tests)."""
    _require_gpu()
    lib = load_library()
    assert x.dtype == torch.bfloat16 and x.stride(3) == 1 and x.shape[3] == 48
    B, H, W, _ = x.shape
    ld = x.stride(2)
    assert x.stride(1) == W * ld and x.stride(0) == H * W * ld, "x must be a channel slice of a dense NHWC tensor"
    wa = np.ascontiguousarray(wa_oihw.permute(0, 2, 3, 1).float().cpu().numpy())
    wb = np.ascontiguousarray(wb_oihw.permute(0, 2, 3, 1).float().cpu().numpy())
    n = C.c_size_t()
    pa, pb = wa.ctypes.data_as(C.POINTER(C.c_float)), wb.ctypes.data_as(C.POINTER(C.c_float))
    _check(lib.aq_pack_downblock_weights(pa, pb, None, C.byref(n), None))
    wbuf = torch.empty(n.value, dtype=torch.uint8, device=x.device)
    _check(lib.aq_pack_downblock_weights(pa, pb, wbuf.data_ptr(), C.byref(n), _stream_ptr()))
    bbuf = torch.cat([ba.float(), bb.float()]).to(x.device).contiguous()
    if out is None:
        out = torch.empty((B, H // 2, W // 2, 96), dtype=torch.bfloat16, device=x.device)
    _check(lib.aq_downblock(x.data_ptr(), ld, 0, out.data_ptr(), out.stride(2), 0, wbuf.data_ptr(), bbuf.data_ptr(), B, H, W, _stream_ptr()))
    torch.cuda.current_stream().synchronize()
    return out


CONV_CFG_DIRECT1X1 = 1000   # AQ_CONV_CFG_DIRECT1X1
CONV_CFG_ASM1X1 = 1004      # AQ_CONV_CFG_ASM1X1
CONV_CFG_DIRECT3X3S2 = 1001  # AQ_CONV_CFG_DIRECT3X3S2
CONV_CFG_PL3X3 = 1002       # AQ_CONV_CFG_PL3X3
CONV_CFG_PL3X3S2 = 1003     # AQ_CONV_CFG_PL3X3S2
CONV_CFG_ONE_TILE_PER_WG = 4096  # AQ_CONV_CFG_ONE_TILE_PER_WG (OR-ed into a tile configuration id)


def conv3x3_pl_nhwc(x: torch.Tensor, w_oihw: torch.Tensor, bias: torch.Tensor, act: bool = True,
                    residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, w8: bool = False) -> torch.Tensor:
    """bf16 NHWC [B,H,W,cin] (may be a channel slice) -> (residual +) SiLU(conv3x3/s1/p1(x) + b) through aq_conv3x3_pl (tests).
    ``out`` and ``residual`` may be channel slices of wider tensors; ``residual`` may be ``out`` itself (in-place shortcut).
    ``w8``: through aq_conv3x3_pl_w8 (e4m3 weight stream; ``w_oihw`` must lie on an fp8 grid, quant.quantize_rows)."""
    _require_gpu()
    lib = load_library()
    assert x.dtype == torch.bfloat16 and x.stride(3) == 1
    B, H, W, cin = x.shape
    cout = w_oihw.shape[0]
    ld = x.stride(2)
    assert x.stride(1) == W * ld and x.stride(0) == H * W * ld, "x must be a channel slice of a dense NHWC tensor"
    w = np.ascontiguousarray(w_oihw.permute(0, 2, 3, 1).float().cpu().numpy())
    n = C.c_size_t()
    wp = w.ctypes.data_as(C.POINTER(C.c_float))
    if w8:
        if not lib.aq_conv3x3_pl_w8_supported(cin, cout, B, H, W):
            raise RuntimeError("aq_conv3x3_pl_w8 does not support this shape")
        bh = np.ascontiguousarray(bias.float().cpu().numpy())
        bp = bh.ctypes.data_as(C.POINTER(C.c_float))
        _check(lib.aq_pack_conv3x3_pl_w8(wp, bp, cin, cout, None, C.byref(n), None, None))
        wbuf = torch.empty(n.value, dtype=torch.uint8, device=x.device)
        bbuf = torch.empty(2048, dtype=torch.float32, device=x.device)
        _check(lib.aq_pack_conv3x3_pl_w8(wp, bp, cin, cout, wbuf.data_ptr(), C.byref(n), bbuf.data_ptr(), _stream_ptr()))
    else:
        _check(lib.aq_pack_conv3x3_pl(wp, cin, cout, None, C.byref(n), None))
        wbuf = torch.empty(n.value, dtype=torch.uint8, device=x.device)
        _check(lib.aq_pack_conv3x3_pl(wp, cin, cout, wbuf.data_ptr(), C.byref(n), _stream_ptr()))
        bbuf = bias.float().to(x.device).contiguous()
    if out is None:
        out = torch.empty((B, H, W, cout), dtype=torch.bfloat16, device=x.device)
    assert out.stride(3) == 1 and (residual is None or residual.stride(3) == 1)
    _check((lib.aq_conv3x3_pl_w8 if w8 else lib.aq_conv3x3_pl)(x.data_ptr(), ld * 2, 16, cin, out.data_ptr(), out.stride(2), 0, cout,
                             residual.data_ptr() if residual is not None else None, residual.stride(2) if residual is not None else 0, 0,
                             wbuf.data_ptr(), bbuf.data_ptr(), B, H, W, int(act), _stream_ptr()))
    torch.cuda.current_stream().synchronize()
    return out


def conv1x1_direct_nhwc(x: torch.Tensor, w_oihw: torch.Tensor, bias: torch.Tensor, act: bool = True, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """bf16 [..., cin] pixels (may be a channel slice of a wider dense tensor) -> SiLU(W x + b) through aq_conv1x1_direct (tests)."""
    _require_gpu()
    lib = load_library()
    assert x.dtype == torch.bfloat16 and x.stride(-1) == 1
    cin, cout = x.shape[-1], w_oihw.shape[0]
    ld = x.stride(-2)
    npix = x.numel() // cin
    w = np.ascontiguousarray(w_oihw.reshape(cout, cin).float().cpu().numpy())
    n = C.c_size_t()
    wp = w.ctypes.data_as(C.POINTER(C.c_float))
    _check(lib.aq_pack_conv1x1_direct(wp, cin, cout, None, C.byref(n), None))
    wbuf = torch.empty(n.value, dtype=torch.uint8, device=x.device)
    _check(lib.aq_pack_conv1x1_direct(wp, cin, cout, wbuf.data_ptr(), C.byref(n), _stream_ptr()))
    bbuf = bias.float().to(x.device).contiguous()
    if out is None:
        out = torch.empty(x.shape[:-1] + (cout,), dtype=torch.bfloat16, device=x.device)
    _check(lib.aq_conv1x1_direct(x.data_ptr(), ld, 0, out.data_ptr(), out.stride(-2), 0, cin, cout, wbuf.data_ptr(), bbuf.data_ptr(), npix, int(act),
                                 _stream_ptr()))
    torch.cuda.current_stream().synchronize()
    return out


def conv1x1_asm_nhwc(x: torch.Tensor, w_oihw: torch.Tensor, bias: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """bf16 [..., cin] pixels (may be a channel slice of a wider dense tensor) -> SiLU(W x + b) through aq_conv1x1_asm, the generated-assembly
    wide 1x1 (tests, tools/time_conv1x1_asm.py)."""
    _require_gpu()
    lib = load_library()
    assert x.dtype == torch.bfloat16 and x.stride(-1) == 1
    cin, cout = x.shape[-1], w_oihw.shape[0]
    ld = x.stride(-2)
    npix = x.numel() // cin
    w = np.ascontiguousarray(w_oihw.reshape(cout, cin).float().cpu().numpy())
    n = C.c_size_t()
    wp = w.ctypes.data_as(C.POINTER(C.c_float))
    _check(lib.aq_pack_conv1x1_asm(wp, cin, cout, None, C.byref(n), None))
    wbuf = torch.empty(n.value, dtype=torch.uint8, device=x.device)
    _check(lib.aq_pack_conv1x1_asm(wp, cin, cout, wbuf.data_ptr(), C.byref(n), _stream_ptr()))
    bbuf = bias.float().to(x.device).contiguous()
    if out is None:
        out = torch.empty(x.shape[:-1] + (cout,), dtype=torch.bfloat16, device=x.device)
    _check(lib.aq_conv1x1_asm(x.data_ptr(), ld, 0, out.data_ptr(), out.stride(-2), 0, cin, cout, wbuf.data_ptr(), bbuf.data_ptr(), npix, 1, _stream_ptr()))
    torch.cuda.current_stream().synchronize()
    return out


def conv3x3s2_direct_nhwc(x: torch.Tensor, w_oihw: torch.Tensor, bias: torch.Tensor, act: bool = True, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """bf16 NHWC [B,H,W,cin] (may be a channel slice) -> SiLU(conv3x3/s2/p1(x) + b) [B,H/2,W/2,cout] through aq_conv3x3s2_direct (tests)."""
    _require_gpu()
    lib = load_library()
    assert x.dtype == torch.bfloat16 and x.stride(3) == 1
    B, H, W, cin = x.shape
    cout = w_oihw.shape[0]
    ld = x.stride(2)
    assert x.stride(1) == W * ld and x.stride(0) == H * W * ld, "x must be a channel slice of a dense NHWC tensor"
    w = np.ascontiguousarray(w_oihw.permute(0, 2, 3, 1).float().cpu().numpy())
    n = C.c_size_t()
    wp = w.ctypes.data_as(C.POINTER(C.c_float))
    _check(lib.aq_pack_conv3x3s2_direct(wp, cin, cout, None, C.byref(n), None))
    wbuf = torch.empty(n.value, dtype=torch.uint8, device=x.device)
    _check(lib.aq_pack_conv3x3s2_direct(wp, cin, cout, wbuf.data_ptr(), C.byref(n), _stream_ptr()))
    bbuf = bias.float().to(x.device).contiguous()
    if out is None:
        out = torch.empty((B, H // 2, W // 2, cout), dtype=torch.bfloat16, device=x.device)
    _check(lib.aq_conv3x3s2_direct(x.data_ptr(), ld, 0, out.data_ptr(), out.stride(2), 0, cin, cout, wbuf.data_ptr(), bbuf.data_ptr(), B, H, W, int(act),
                                   _stream_ptr()))
    torch.cuda.current_stream().synchronize()
    return out


def conv3x3_pl_s2_nhwc(x: torch.Tensor, w_oihw: torch.Tensor, bias: torch.Tensor, act: bool = True, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """bf16 NHWC [B,H,W,cin] (may be a channel slice) -> SiLU(conv3x3/s2/p1(x) + b) [B,H/2,W/2,cout] (may be a channel slice) through
    aq_conv3x3_pl_s2, the planar stride-2 kernel (tests, tools)."""
    _require_gpu()
    lib = load_library()
    assert x.dtype == torch.bfloat16 and x.stride(3) == 1
    B, H, W, cin = x.shape
    cout = w_oihw.shape[0]
    ld = x.stride(2)
    assert x.stride(1) == W * ld and x.stride(0) == H * W * ld, "x must be a channel slice of a dense NHWC tensor"
    w = np.ascontiguousarray(w_oihw.permute(0, 2, 3, 1).float().cpu().numpy())
    n = C.c_size_t()
    wp = w.ctypes.data_as(C.POINTER(C.c_float))
    _check(lib.aq_pack_conv3x3_pl_s2(wp, cin, cout, None, C.byref(n), None))
    wbuf = torch.empty(n.value, dtype=torch.uint8, device=x.device)
    _check(lib.aq_pack_conv3x3_pl_s2(wp, cin, cout, wbuf.data_ptr(), C.byref(n), _stream_ptr()))
    bbuf = torch.zeros((cout + 255) // 256 * 256 + 1024, dtype=torch.float32, device=x.device)    # the kernel's bias tile over-reads up to 1024 floats
    bbuf[:cout] = bias.float().to(x.device)
    if out is None:
        out = torch.empty((B, H // 2, W // 2, cout), dtype=torch.bfloat16, device=x.device)
    assert out.stride(3) == 1 and out.stride(1) == (W // 2) * out.stride(2)
    # channel offsets are expressed through the base pointers (slices): in_choff = out_choff = 0
    _check(lib.aq_conv3x3_pl_s2(x.data_ptr(), ld, 0, cin, out.data_ptr(), out.stride(2), 0, cout, wbuf.data_ptr(), bbuf.data_ptr(), B, H, W, int(act),
                                _stream_ptr()))
    torch.cuda.current_stream().synchronize()
    return out


def conv3x3_pl_f8_nhwc(xq: torch.Tensor, act_scale: float, w_oihw: torch.Tensor, bias: torch.Tensor, act: bool = True,
                       residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """e4m3 codes NHWC [B,H,W,cin] (uint8 or float8_e4m3fn view; may be a channel slice; value = code x act_scale) ->
    (residual +) SiLU(conv3x3/s1/p1 + b) as bf16 [B,H,W,cout] through aq_conv3x3_pl_f8 (fp8 MFMA on both operands; tests, tools)."""
    _require_gpu()
    lib = load_library()
    xq = xq.view(torch.uint8)
    assert xq.stride(3) == 1
    B, H, W, cin = xq.shape
    cout = w_oihw.shape[0]
    ld = xq.stride(2)
    assert xq.stride(1) == W * ld and xq.stride(0) == H * W * ld, "x must be a channel slice of a dense NHWC tensor"
    w = np.ascontiguousarray(w_oihw.permute(0, 2, 3, 1).float().cpu().numpy())
    bh = np.ascontiguousarray(bias.float().cpu().numpy())
    n = C.c_size_t()
    wp, bp = w.ctypes.data_as(C.POINTER(C.c_float)), bh.ctypes.data_as(C.POINTER(C.c_float))
    _check(lib.aq_pack_conv3x3_pl_f8(wp, bp, cin, cout, float(act_scale), None, C.byref(n), None, None))
    wbuf = torch.empty(n.value, dtype=torch.uint8, device=xq.device)
    sb = torch.empty(2048, dtype=torch.float32, device=xq.device)
    _check(lib.aq_pack_conv3x3_pl_f8(wp, bp, cin, cout, float(act_scale), wbuf.data_ptr(), C.byref(n), sb.data_ptr(), _stream_ptr()))
    if out is None:
        out = torch.empty((B, H, W, cout), dtype=torch.bfloat16, device=xq.device)
    assert out.dtype == torch.bfloat16 and out.stride(3) == 1 and (residual is None or (residual.dtype == torch.bfloat16 and residual.stride(3) == 1))
    _check(lib.aq_conv3x3_pl_f8(xq.data_ptr(), ld, 0, cin, out.data_ptr(), out.stride(2), 0, cout,
                                residual.data_ptr() if residual is not None else None, residual.stride(2) if residual is not None else 0, 0,
                                wbuf.data_ptr(), sb.data_ptr(), B, H, W, int(act), _stream_ptr()))
    torch.cuda.current_stream().synchronize()
    return out


JPEG_WS_MAX = 16383     # AQ_JPEG_WS_MAX (include/aq_engine.h): the acceptance rule of the device half of the JPEG decode


def jpeg_idct_rgb_checked(coef: torch.Tensor, coef_off: torch.Tensor, qt: torch.Tensor, H: int, W: int, out: Optional[torch.Tensor] = None,
                          scratch: Optional[torch.Tensor] = None, flags: Optional[torch.Tensor] = None):
    """The device half of the split JPEG decode (aq_jpeg_idct_rgb_checked): coef int16 CUDA (the images' coefficient blocks), coef_off int64
    [B] (first value of each image, multiples of 64), qt uint16 [B,3,64]  ->  (uint8 RGB [B,H,W,3], flags int32 CUDA [B]).  Image b's pixels
    are the ones libjpeg(-turbo) produces iff flags[b] == 0: a flag of 1 says that one of its blocks is outside the acceptance rule
    (a pass-1 IDCT workspace value beyond +-JPEG_WS_MAX), where the library's own pixels are not defined; the caller refuses the file."""
    _require_gpu()
    lib = load_library()
    B = int(coef_off.shape[0])
    assert coef.is_cuda and coef.dtype == torch.int16 and coef_off.dtype == torch.int64 and qt.dtype in (torch.uint16, torch.int16) and qt.numel() == B * 192
    if out is None:
        out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=coef.device)
    n = lib.aq_jpeg_scratch_bytes(B, H, W)
    if scratch is None or scratch.numel() < n:
        scratch = torch.empty(n, dtype=torch.uint8, device=coef.device)
    if flags is None:
        flags = torch.empty(B, dtype=torch.int32, device=coef.device)
    assert flags.is_cuda and flags.dtype == torch.int32 and flags.is_contiguous() and flags.numel() >= B
    _check(lib.aq_jpeg_idct_rgb_checked(coef.data_ptr(), coef_off.data_ptr(), qt.data_ptr(), B, H, W, scratch.data_ptr(), out.data_ptr(),
                                        flags.data_ptr(), _stream_ptr()))
    return out, flags[:B]


def jpeg_idct_rgb(coef: torch.Tensor, coef_off: torch.Tensor, qt: torch.Tensor, H: int, W: int, out: Optional[torch.Tensor] = None,
                  scratch: Optional[torch.Tensor] = None) -> torch.Tensor:
    """jpeg_idct_rgb_checked without its flags: the pixels libjpeg(-turbo) produces for images inside the acceptance rule, and no word
    about the others.  For callers that know their files (tests, tools); detect.py uses the checked call."""
    return jpeg_idct_rgb_checked(coef, coef_off, qt, H, W, out=out, scratch=scratch)[0]


def jpeg_huffman_decode(streams: torch.Tensor, segs: torch.Tensor, tabsets: torch.Tensor, coef: torch.Tensor, status: Optional[torch.Tensor] = None) -> torch.Tensor:
    """GPU entropy decode (aq_jpeg_huffman_decode): ``streams`` uint8 CUDA = the upload buffer jpeg.GpuDecodeBatch filled, ``segs`` uint8
    CUDA [nseg, 32] = its segment descriptors, ``tabsets`` uint8 CUDA [n_sets, jpeg.TABSET_BYTES]; ``coef`` int16 CUDA, ZEROED by the caller,
    receives the quantised coefficient blocks in the host decoder's layout.  Returns the per-segment status tensor (int32; 0 = ok)."""
    _require_gpu()
    lib = load_library()
    assert streams.is_cuda and streams.dtype == torch.uint8 and segs.is_cuda and segs.dtype == torch.uint8 and segs.dim() == 2 and segs.shape[1] == 32
    assert tabsets.is_cuda and tabsets.dtype == torch.uint8 and coef.is_cuda and coef.dtype == torch.int16
    nseg = int(segs.shape[0])
    if status is None:
        status = torch.empty(nseg, dtype=torch.int32, device=streams.device)
    _check(lib.aq_jpeg_huffman_decode(streams.data_ptr(), segs.data_ptr(), nseg, tabsets.data_ptr(), coef.data_ptr(), status.data_ptr(), _stream_ptr()))
    return status


def jpeg_slots_to_rgb(slots: torch.Tensor, H: int, W: int, scratch: Optional[torch.Tensor] = None, flags: Optional[torch.Tensor] = None):
    """A batch as the decode workers' coefficient mode delivers it -- uint8 CUDA [b, jpeg.slot_bytes(H, W)]: per image the int16 coefficient
    blocks, then three uint16 quantisation tables -- to (RGB tiles uint8 [b, H, W, 3], flags int32 [b]) on the device, as
    jpeg_idct_rgb_checked returns them."""
    from . import jpeg
    assert slots.is_cuda and slots.dtype == torch.uint8 and slots.dim() == 2 and slots.is_contiguous() and slots.shape[1] == jpeg.slot_bytes(H, W)
    b = slots.shape[0]
    nco = jpeg.coef_count(H, W)
    qt = slots[:, 2 * nco:2 * nco + 384].contiguous().view(torch.int16)
    off = torch.arange(b, dtype=torch.int64, device=slots.device) * (slots.shape[1] // 2)
    return jpeg_idct_rgb_checked(slots.view(torch.int16).reshape(-1), off, qt, H, W, scratch=scratch, flags=flags)


def _head_level_buffers(x: torch.Tensor, w_oi: torch.Tensor, bias: torch.Tensor, anchors_px, nc: int, cap: int, count_stride: int,
                        counts, cand, rows):
    """Packed weights, anchors and the output buffers of one aq_head_decode[_aug] call (tests).  Without caller-supplied buffers: zeroed
    counters [(B - 1) * count_stride + 1], cand [B, cap] filled with -1, zeroed rows [B, cap, nc + 5]; supplied ones are appended to."""
    lib = load_library()
    assert x.dtype == torch.bfloat16 and x.stride(3) == 1
    B, ny, nx, cin = x.shape
    ld = x.stride(2)
    assert x.stride(1) == nx * ld and x.stride(0) == ny * nx * ld
    cout = len(anchors_px) * (nc + 5)
    w = np.ascontiguousarray(w_oi.float().cpu().numpy().reshape(cout, cin))
    bh = np.ascontiguousarray(bias.float().cpu().numpy())
    n = C.c_size_t()
    fp = C.POINTER(C.c_float)
    _check(lib.aq_pack_head_weights(w.ctypes.data_as(fp), bh.ctypes.data_as(fp), cin, cout, None, C.byref(n), None))
    wbuf = torch.empty(n.value, dtype=torch.uint8, device=x.device)
    _check(lib.aq_pack_head_weights(w.ctypes.data_as(fp), bh.ctypes.data_as(fp), cin, cout, C.c_void_p(wbuf.data_ptr()), C.byref(n), C.c_void_p(_stream_ptr())))
    assert count_stride >= 1
    if counts is None:
        counts = torch.zeros((B - 1) * count_stride + 1, dtype=torch.int32, device=x.device)
    if cand is None:
        cand = torch.full((B, cap), -1, dtype=torch.int32, device=x.device)
    if rows is None:
        rows = torch.zeros((B, cap, nc + 5), dtype=torch.float32, device=x.device)
    assert counts.dtype == torch.int32 and counts.is_contiguous() and counts.numel() >= (B - 1) * count_stride + 1
    assert cand.dtype == torch.int32 and cand.is_contiguous() and cand.numel() >= B * cap
    assert rows.dtype == torch.float32 and rows.is_contiguous() and rows.numel() >= B * cap * (nc + 5)
    anch = np.ascontiguousarray(np.asarray(anchors_px, np.float32).reshape(-1))
    return wbuf, anch, counts, cand, rows


def head_decode_level(x: torch.Tensor, w_oi: torch.Tensor, bias: torch.Tensor, cand_off: int, stride: float, anchors_px, nc: int,
                      conf_thres: float, cap: int, count_stride: int = 1, counts: Optional[torch.Tensor] = None,
                      cand: Optional[torch.Tensor] = None, rows: Optional[torch.Tensor] = None):
    """One Detect level through aq_head_decode (tests): x bf16 NHWC [B, ny, nx, cin] (may be a channel slice), w [na * (nc + 5), cin].
    Returns (counts int32, cand [B, cap] int32, rows [B, cap, nc + 5] float32); the order within an image is unspecified.  Image b's
    counter is counts[b * count_stride].  ``counts`` / ``cand`` / ``rows``: the caller's buffers, appended to (several levels into one
    list, as the engine runs them); by default fresh ones."""
    _require_gpu()
    lib = load_library()
    B, ny, nx, cin = x.shape
    wbuf, anch, counts, cand, rows = _head_level_buffers(x, w_oi, bias, anchors_px, nc, cap, count_stride, counts, cand, rows)
    _check(lib.aq_head_decode(C.c_void_p(x.data_ptr()), x.stride(2), 0, cin, C.c_void_p(wbuf.data_ptr()), B, ny, nx, cand_off, C.c_float(stride),
                              anch.ctypes.data_as(C.POINTER(C.c_float)), nc, len(anchors_px), C.c_float(conf_thres), C.c_void_p(cand.data_ptr()),
                              C.c_void_p(rows.data_ptr()), C.c_void_p(counts.data_ptr()), count_stride, cap, C.c_void_p(_stream_ptr())))
    torch.cuda.current_stream().synchronize()
    return counts, cand, rows


def head_counts_gather(wide: torch.Tensor, count_stride: int, B: int) -> torch.Tensor:
    """aq_head_counts_gather (tests): the B counters kept count_stride ints apart, as the compact int32 [B] array aq_nms reads."""
    _require_gpu()
    lib = load_library()
    assert wide.dtype == torch.int32 and wide.is_contiguous() and wide.numel() >= (B - 1) * count_stride + 1
    out = torch.full((B,), -1, dtype=torch.int32, device=wide.device)
    _check(lib.aq_head_counts_gather(C.c_void_p(wide.data_ptr()), count_stride, C.c_void_p(out.data_ptr()), B, C.c_void_p(_stream_ptr())))
    torch.cuda.current_stream().synchronize()
    return out


def stemdown_nhwc(tiles_u8: torch.Tensor, ws_oihw: torch.Tensor, bs: torch.Tensor, wa_oihw: torch.Tensor, ba: torch.Tensor,
                  wb_oihw: torch.Tensor, bb: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 [B,Hi,Wi,3] -> stem (6x6/s2, 3 -> 48) -> 3x3/s2 (48 -> 96) -> 1x1 (96 -> 96), SiLU after each, as bf16 NHWC
    [B,Hi/4,Wi/4,96] through aq_stemdown (tests): one launch, the stem's output never leaves the CU."""
    _require_gpu()
    lib = load_library()
    B, Hi, Wi, _ = tiles_u8.shape
    assert tiles_u8.dtype == torch.uint8 and tiles_u8.is_contiguous() and ws_oihw.shape[0] == 48
    dev = tiles_u8.device
    fp = C.POINTER(C.c_float)
    ws = np.ascontiguousarray(ws_oihw.permute(0, 2, 3, 1).float().cpu().numpy())
    n = C.c_size_t()
    _check(lib.aq_pack_stem_weights(ws.ctypes.data_as(fp), 48, AQ_BF16, None, C.byref(n), None))
    wsbuf = torch.empty(n.value, dtype=torch.uint8, device=dev)
    _check(lib.aq_pack_stem_weights(ws.ctypes.data_as(fp), 48, AQ_BF16, wsbuf.data_ptr(), C.byref(n), _stream_ptr()))
    bsbuf = torch.zeros(64, dtype=torch.float32, device=dev)
    bsbuf[:48] = bs.float().to(dev)
    wa = np.ascontiguousarray(wa_oihw.permute(0, 2, 3, 1).float().cpu().numpy())
    wb = np.ascontiguousarray(wb_oihw.permute(0, 2, 3, 1).float().cpu().numpy())
    _check(lib.aq_pack_downblock_weights(wa.ctypes.data_as(fp), wb.ctypes.data_as(fp), None, C.byref(n), None))
    wbuf = torch.empty(n.value, dtype=torch.uint8, device=dev)
    _check(lib.aq_pack_downblock_weights(wa.ctypes.data_as(fp), wb.ctypes.data_as(fp), wbuf.data_ptr(), C.byref(n), _stream_ptr()))
    bbuf = torch.cat([ba.float(), bb.float()]).to(dev).contiguous()
    if out is None:
        out = torch.empty((B, Hi // 4, Wi // 4, 96), dtype=torch.bfloat16, device=dev)
    _check(lib.aq_stemdown(C.c_void_p(tiles_u8.data_ptr()), C.c_void_p(out.data_ptr()), out.stride(2), 0, C.c_void_p(wsbuf.data_ptr()),
                           C.c_void_p(bsbuf.data_ptr()), C.c_void_p(wbuf.data_ptr()), C.c_void_p(bbuf.data_ptr()), B, Hi, Wi, C.c_void_p(_stream_ptr())))
    torch.cuda.current_stream().synchronize()
    return out


def _aug_taps_device(H: int, W: int, h: int, w: int, flip: bool, device):
    from . import augment as _aug
    ytab = torch.from_numpy(_aug.bilinear_taps(H, h).view(np.int32).copy()).to(device)
    xtab = torch.from_numpy(_aug.bilinear_taps(W, w, flip).view(np.int32).copy()).to(device)
    return ytab, xtab


def stem_conv_scaled_nhwc(tiles_u8: torch.Tensor, w_oihw: torch.Tensor, bias: torch.Tensor, h: int, w: int, hp: int, wp: int, flip: bool,
                          act: bool = True, precision: str = "bf16") -> torch.Tensor:
    """aq_stem_conv_scaled (tests): the stem on scale_img(flip(u8 / 255)) -- interpolated to h x w, padded with 0.447 to hp x wp --
    as NHWC [B, hp/2, wp/2, cout]."""
    _require_gpu()
    lib = load_library()
    prec = PRECISIONS[precision]
    B, H, W, _ = tiles_u8.shape
    cout = w_oihw.shape[0]
    wk = np.ascontiguousarray(w_oihw.permute(0, 2, 3, 1).float().cpu().numpy())
    n = C.c_size_t()
    wptr = wk.ctypes.data_as(C.POINTER(C.c_float))
    _check(lib.aq_pack_stem_weights(wptr, cout, prec, None, C.byref(n), None))
    wbuf = torch.empty(n.value, dtype=torch.uint8, device=tiles_u8.device)
    _check(lib.aq_pack_stem_weights(wptr, cout, prec, wbuf.data_ptr(), C.byref(n), _stream_ptr()))
    bbuf = torch.zeros(64, dtype=torch.float32, device=tiles_u8.device)
    bbuf[:cout] = bias.float().to(tiles_u8.device)
    ytab, xtab = _aug_taps_device(H, W, h, w, flip, tiles_u8.device)
    out = torch.empty((B, hp // 2, wp // 2, cout), dtype=_act_dtype(prec), device=tiles_u8.device)
    _check(lib.aq_stem_conv_scaled(tiles_u8.data_ptr(), H, W, ytab.data_ptr(), xtab.data_ptr(), h, w, out.data_ptr(), cout, 0, cout,
                                   wbuf.data_ptr(), bbuf.data_ptr(), B, hp, wp, int(act), prec, _stream_ptr()))
    torch.cuda.current_stream().synchronize()
    return out


def preprocess_s2d_scaled(tiles_u8: torch.Tensor, h: int, w: int, hp: int, wp: int, flip: bool, precision: str = "fp32") -> torch.Tensor:
    """aq_preprocess_s2d_scaled (tests): space-to-depth [B, hp/2, wp/2, 16] of the scaled network input (channels 12..15 zero)."""
    _require_gpu()
    lib = load_library()
    prec = PRECISIONS[precision]
    B, H, W, _ = tiles_u8.shape
    ytab, xtab = _aug_taps_device(H, W, h, w, flip, tiles_u8.device)
    out = torch.empty((B, hp // 2, wp // 2, 16), dtype=_act_dtype(prec), device=tiles_u8.device)
    _check(lib.aq_preprocess_s2d_scaled(tiles_u8.data_ptr(), H, W, ytab.data_ptr(), xtab.data_ptr(), h, w, out.data_ptr(), B, hp, wp, prec,
                                        _stream_ptr()))
    torch.cuda.current_stream().synchronize()
    return out


def detect_decode_aug(heads, H: int, W: int, nc: int, anchors_px, strides, level_mask: int, cand_base: int, rows_per_image: int,
                      scale: float, flip_w: float) -> torch.Tensor:
    """aq_detect_decode_aug in pred mode (tests): fp32 head maps [B, ny, nx, na * (nc + 5)] per level -> pred [B, rows_per_image, nc + 5]
    with this pass's rows at cand_base + n (the other rows stay zero)."""
    _require_gpu()
    lib = load_library()
    heads = [h.contiguous() for h in heads]
    B, na = heads[0].shape[0], len(anchors_px[0])
    pred = torch.zeros((B, rows_per_image, nc + 5), dtype=torch.float32, device=heads[0].device)
    hp = (C.c_void_p * 3)(*[h.data_ptr() for h in heads])
    anch = (C.c_float * (3 * na * 2))(*[float(v) for lvl in anchors_px for a in lvl for v in a])
    st = (C.c_float * 3)(*[float(s) for s in strides])
    _check(lib.aq_detect_decode_aug(hp, int(heads[0].shape[3]), B, H, W, nc, na, anch, st, level_mask, cand_base, rows_per_image,
                                    C.c_float(scale), C.c_float(flip_w), pred.data_ptr(), C.c_float(0.0), None, None, None, 0, _stream_ptr()))
    torch.cuda.current_stream().synchronize()
    return pred


def head_decode_level_aug(x: torch.Tensor, w_oi: torch.Tensor, bias: torch.Tensor, cand_off: int, stride: float, anchors_px, nc: int,
                          conf_thres: float, cap: int, scale: float, flip_w: float, count_stride: int = 1,
                          counts: Optional[torch.Tensor] = None, cand: Optional[torch.Tensor] = None, rows: Optional[torch.Tensor] = None):
    """head_decode_level through aq_head_decode_aug (tests): the same outputs, the boxes de-scaled."""
    _require_gpu()
    lib = load_library()
    B, ny, nx, cin = x.shape
    wbuf, anch, counts, cand, rows = _head_level_buffers(x, w_oi, bias, anchors_px, nc, cap, count_stride, counts, cand, rows)
    _check(lib.aq_head_decode_aug(x.data_ptr(), x.stride(2), 0, cin, wbuf.data_ptr(), B, ny, nx, cand_off, stride,
                                  anch.ctypes.data_as(C.POINTER(C.c_float)), nc, len(anchors_px), conf_thres, scale, flip_w, cand.data_ptr(),
                                  rows.data_ptr(), counts.data_ptr(), count_stride, cap, _stream_ptr()))
    torch.cuda.current_stream().synchronize()
    return counts, cand, rows
