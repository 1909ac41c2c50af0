"""ctypes binding of libhnet_hip.so — the C ABI declared in include/hnet.h.

There is no CPU fallback: if the HIP library is missing or a call fails, this raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as _np

_PKG = os.path.dirname(os.path.abspath(__file__))
# HNET_LIB_PATH: another build of the SAME library (same-box A/B of two source states with tools/ab_bench.py); never a fallback
LIB_PATH = os.environ.get("HNET_LIB_PATH") or os.path.join(_PKG, "libhnet_hip.so")

HNET_OK = 0
PREC_FP32, PREC_BF16, PREC_BF16X3, PREC_F16X2 = 0, 1, 2, 3
PIX_U8, PIX_F32 = 0, 1
ERR_NOT_READY = 4

# every symbol include/hnet.h declares (tests check the library exports all of them)
SYMBOLS = [
    "hnet_default_config", "hnet_create", "hnet_create_from_memory", "hnet_destroy", "hnet_status_string",
    "hnet_last_error", "hnet_version", "hnet_push_image", "hnet_attach_images", "hnet_image_count", "hnet_latest_time", "hnet_infer",
    "hnet_infer_batch", "hnet_infer_batch_device", "hnet_infer_batch_packed_device", "hnet_infer_mc_partial_device", "hnet_mc_finish_device",
    "hnet_mc_finish_packed_device", "hnet_mc_finish_gathered_device",
    "hnet_synchronize", "hnet_last_timing", "hnet_time_batch_device", "hnet_stage_count", "hnet_stage_name",
    "hnet_stage_flops_per_pair", "hnet_stage_kernels", "hnet_get_config", "hnet_profile_batch_device", "hnet_op_warp", "hnet_op_dlt", "hnet_op_conv",
    "hnet_op_prep", "hnet_op_prep_u8", "hnet_op_prep_batch", "hnet_debug_layer_output", "hnet_debug_h_part1",
    "hnet_set_camera", "hnet_set_undistort_maps", "hnet_get_undistort_maps", "hnet_push_raw_image", "hnet_op_undistort",
    "hnet_op_block4_fused", "hnet_op_block3_fused", "hnet_op_block42_fused", "hnet_precision", "hnet_overflow_flag",
    "hnet_create_group", "hnet_create_group_from_memory", "hnet_destroy_group", "hnet_group_size", "hnet_group_context", "hnet_group_stream",
    "hnet_group_last_error", "hnet_group_infer_batch_packed_device", "hnet_group_join", "hnet_group_synchronize", "hnet_group_overflow_flag",
    "hnet_create_sessions", "hnet_destroy_sessions", "hnet_sessions_push", "hnet_sessions_add_camera", "hnet_sessions_bind_camera",
    "hnet_sessions_push_raw", "hnet_sessions_infer", "hnet_sessions_image_count", "hnet_sessions_latest_time", "hnet_sessions_set_seq",
    "hnet_sessions_seq", "hnet_sessions_reset", "hnet_sessions_get_frame", "hnet_sessions_last_timing", "hnet_infer_batch_seqs_packed_device",
    "hnet_filter_default_params", "hnet_create_filters", "hnet_destroy_filters", "hnet_filters_set_params", "hnet_filters_set_state",
    "hnet_filters_get_state", "hnet_filters_step", "hnet_filters_last_priors", "hnet_filters_last_timing",
    "hnet_filter_default_init_params", "hnet_filters_enable_feed", "hnet_filters_set_init_params", "hnet_filters_feed_imu", "hnet_filters_initialized",
    "hnet_filters_uninitialize", "hnet_filters_advance", "hnet_filters_last_selection",
    "hnet_sessions_set_iterative_model", "hnet_sessions_infer_iter",
    "hnet_filters_predict", "hnet_filters_newest_imu_time", "hnet_filters_last_predict_device_ms",
    "hnet_filters_predict_cov", "hnet_filters_last_predict_cov_device_ms",
    "hnet_filters_enable_innovations", "hnet_filters_set_nis_gate", "hnet_filters_last_innovations", "hnet_filters_innovation_stats",
    "hnet_filters_reset_innovation_stats",
    "hnet_op_photo_residual", "hnet_sessions_photo_residual", "hnet_filters_enable_photometric", "hnet_filters_last_photometric",
    "hnet_filters_set_photo_gate", "hnet_filters_photo_stats", "hnet_filters_reset_photo_stats", "hnet_filters_set_photo_gate_taps",
    "hnet_photo_align_default_opts", "hnet_op_photo_align", "hnet_sessions_photo_align", "hnet_last_photo_align_device_ms",
    "hnet_op_photo_align_pyramid", "hnet_sessions_photo_align_pyramid", "hnet_op_photo_pyramid",
    "hnet_photo_robust_default_opts", "hnet_op_photo_align_robust", "hnet_sessions_photo_align_robust", "hnet_photo_robust_marginal",
    "hnet_op_photo_align_masked", "hnet_keyframe_localise_default_opts", "hnet_op_keyframe_localise", "hnet_sessions_enable_keyframe_localise",
    "hnet_sessions_keyframe_localise",
    "hnet_photo_refine_default_opts", "hnet_filters_set_photo_refine", "hnet_filters_last_refine", "hnet_filters_refine_stats", "hnet_filters_reset_refine_stats",
    "hnet_photo_search_default_opts", "hnet_op_photo_search", "hnet_sessions_photo_search",
    "hnet_keyframe_relocalise_default_opts", "hnet_sessions_keyframe_relocalise",
    "hnet_photo_search_make_hyp", "hnet_photo_search_yaw_table", "hnet_photo_search_default_yaw_table", "hnet_op_photo_search_oriented",
    "hnet_sessions_photo_search_oriented", "hnet_sessions_keyframe_relocalise_oriented",
    "hnet_photo_search_fine_default_opts", "hnet_photo_search_fine_yaw_table", "hnet_op_photo_search_fine", "hnet_sessions_photo_search_fine",
    "hnet_sessions_keyframe_relocalise_fine",
    "hnet_keyframe_default_opts", "hnet_sessions_enable_keyframes", "hnet_sessions_keyframe_track", "hnet_sessions_keyframe_reset", "hnet_sessions_get_keyframe",
    "hnet_sessions_last_keyframe_device_ms",
    "hnet_keyframe_revisit_default_opts", "hnet_sessions_enable_keyframe_map", "hnet_sessions_keyframe_revisit", "hnet_sessions_keyframe_map_info",
    "hnet_sessions_get_map_keyframe",
    "hnet_keyframe_recover_default_opts", "hnet_sessions_keyframe_track_recover",
    "hnet_keyframe_measure_default_opts", "hnet_filters_set_keyframe_measure", "hnet_filters_last_keyframe_measure", "hnet_filters_keyframe_measure_stats",
    "hnet_filters_reset_keyframe_measure_stats", "hnet_filters_set_keyframe_recover", "hnet_filters_last_keyframe_recover",
    "hnet_keyframe_render_fit_view", "hnet_op_keyframe_render", "hnet_sessions_enable_keyframe_render", "hnet_sessions_keyframe_render",
    "hnet_keyframe_adjust_default_opts", "hnet_op_keyframe_adjust_solve", "hnet_op_keyframe_adjust", "hnet_sessions_enable_keyframe_adjust",
    "hnet_sessions_keyframe_adjust",
]
# hnet_filters_advance's status per listed session (include/hnet.h HNET_ADV_*)
ADV_STEPPED, ADV_WAIT_IMU, ADV_WAIT_INIT, ADV_INITIALIZED, ADV_PROPAGATED, ADV_NO_FRAME = range(6)
# hnet_filters_predict's status per listed session (include/hnet.h HNET_PRED_*)
PRED_OK, PRED_NO_STATE, PRED_WAIT_IMU, PRED_AT_STATE = range(4)
# an innovation record's flag (include/hnet.h HNET_INNOV_*)
INNOV_NONE, INNOV_USED, INNOV_REJECTED, INNOV_SINGULAR, INNOV_SKIPPED = range(5)


class Config(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("device_id", C.c_int32), ("use_prior", C.c_int32),
                ("blocks_to_run", C.c_int32), ("mc_samples", C.c_int32), ("dropout_p", C.c_float),
                ("mc_seed", C.c_uint64), ("emit_error_map", C.c_int32), ("precision", C.c_int32),
                ("max_batch", C.c_int32), ("mc_sample_begin", C.c_int32), ("mc_sample_end", C.c_int32),
                ("warp_exact", C.c_int32), ("graph", C.c_int32), ("variant", C.c_uint32)]


class Camera(C.Structure):
    """hnet_camera: fisheye flag, raw size, (fx, fy, cx, cy), distortion (k1..k4 or k1, k2, p1, p2)"""
    _fields_ = [("fisheye", C.c_int32), ("raw_rows", C.c_int32), ("raw_cols", C.c_int32), ("k", C.c_double * 4), ("d", C.c_double * 4)]


class Timing(C.Structure):
    _fields_ = [("device_ms", C.c_double), ("host_ms", C.c_double), ("n_inferences", C.c_int64),
                ("sum_device_ms_after_100", C.c_double), ("n_main_inferences", C.c_int64)]


class FilterParams(C.Structure):
    """hnet_filter_params: extrinsics, noise densities, gravity, network covariance scale, camera-IMU time offset, IMU averaging"""
    _fields_ = [("c_R_i", C.c_double * 9), ("i_t_i2c", C.c_double * 3), ("sigma_w", C.c_double), ("sigma_a", C.c_double),
                ("sigma_wb", C.c_double), ("sigma_ab", C.c_double), ("gravity_mag", C.c_double), ("k_net_cov", C.c_double),
                ("cam_imu_dt", C.c_double), ("imu_avg", C.c_int32)]


class InnovationStats(C.Structure):
    """hnet_innovation_stats: records by flag, the sum of the NIS over the USED records, the largest NIS seen"""
    _fields_ = [("used", C.c_int64), ("rejected", C.c_int64), ("singular", C.c_int64), ("sum_nis", C.c_double), ("max_nis", C.c_double)]


class PhotoStats(C.Structure):
    """hnet_photo_stats: estimate records judged, those rejected / degenerate among them, sum and maximum of the estimate / prior residual ratio"""
    _fields_ = [("judged", C.c_int64), ("rejected", C.c_int64), ("degenerate", C.c_int64), ("sum_ratio", C.c_double), ("max_ratio", C.c_double)]


class InitParams(C.Structure):
    """hnet_init_params: the static initialiser's window length, excitation threshold, initial height and wait_for_jerk"""
    _fields_ = [("window_time", C.c_double), ("imu_thresh", C.c_double), ("init_height", C.c_double), ("wait_for_jerk", C.c_int32)]


# hnet_filter_state / hnet_imu as numpy records (the C structs are packed doubles)

FILTER_STATE_DTYPE = _np.dtype([("t", "<f8"), ("p", "<f8", 3), ("q", "<f8", 4), ("v", "<f8", 3), ("ba", "<f8", 3), ("bg", "<f8", 3),
                                ("offset", "<f8", (4, 3)), ("cov", "<f8", (27, 27))])
IMU_DTYPE = _np.dtype([("t", "<f8"), ("wm", "<f8", 3), ("am", "<f8", 3)])
# hnet_odometry: what hnet_filters_predict writes per listed session
ODOMETRY_DTYPE = _np.dtype([("t_cam", "<f8"), ("t_imu", "<f8"), ("p", "<f8", 3), ("q", "<f8", 4), ("v", "<f8", 3), ("w_pos", "<f8", 3),
                            ("rpy", "<f8", 3), ("body_pos", "<f8", 3), ("body_vel", "<f8", 3), ("prior_px", "<f8", 8),
                            ("intervals", "<i4"), ("status", "<i4")])
# hnet_odometry_cov: what hnet_filters_predict_cov writes per listed session next to its hnet_odometry
ODOMETRY_COV_DTYPE = _np.dtype([("pose_cov", "<f8", (6, 6)), ("body_pos_cov", "<f8", (3, 3)), ("body_vel_cov", "<f8", (3, 3)), ("prior_cov_px", "<f8", (8, 8))])
# hnet_innovation: one record per IEKF iteration and stepping session (hnet_filters_last_innovations)
INNOVATION_DTYPE = _np.dtype([("r", "<f8", 8), ("s_diag", "<f8", 8), ("nis", "<f8"), ("iteration", "<i4"), ("flag", "<i4")])


# hnet_photo_residual: one record per (frame pair, candidate offsets); flags: PHOTO_DEGENERATE, PHOTO_REJECTED (include/hnet.h HNET_PHOTO_*)
PHOTO_RESIDUAL_DTYPE = _np.dtype([("sum", "<f8"), ("sum_inside", "<f8"), ("n_inside", "<i4"), ("flags", "<i4")])
PHOTO_DEGENERATE = 1
PHOTO_REJECTED = 2
PHOTO_MAX_CANDIDATES = 66

# hnet_photo_align: one record per aligned frame pair; flags: ALIGN_* (include/hnet.h HNET_ALIGN_*)
PHOTO_ALIGN_DTYPE = _np.dtype([("offsets_px", "<f4", 8), ("mse0", "<f8"), ("mse", "<f8"), ("n_valid0", "<i4"), ("n_valid", "<i4"), ("trials", "<i4"),
                               ("accepted", "<i4"), ("flags", "<i4"), ("pad", "<i4"), ("lambda", "<f8"), ("grad", "<f8", 8), ("info", "<f8", (8, 8))])
assert PHOTO_ALIGN_DTYPE.itemsize == 656      # (pad: the C struct's alignment gap, written as 0 - named, so that numpy copies it and records compare byte for byte)
ALIGN_CONVERGED, ALIGN_SINGULAR, ALIGN_DEGENERATE, ALIGN_FEW_PIXELS = 1, 2, 4, 8
ALIGN_MAX_ITERATIONS = 32
ALIGN_MAX_LEVELS = 4                          # hnet_op_photo_align_pyramid: levels 1 .. 4
PHOTO_PYRAMID_BYTES = 17920 + 4480 + 1120     # hnet_op_photo_pyramid: levels 1 .. 3 of one frame, packed

# hnet_photo_robust: hnet_photo_align's fields under "px", then gain, bias, the outlier counts and the ten-parameter gradient and matrix
PHOTO_ROBUST_DTYPE = _np.dtype([("px", PHOTO_ALIGN_DTYPE), ("gain", "<f8"), ("bias", "<f8"), ("n_outliers0", "<i4"), ("n_outliers", "<i4"),
                                ("grad10", "<f8", 10), ("info10", "<f8", (10, 10))])
assert PHOTO_ROBUST_DTYPE.itemsize == 1560


class PhotoAlignOpts(C.Structure):
    """hnet_photo_align_opts: trials at the most, valid pixels a point needs, initial damping, convergence threshold in pixels"""
    _fields_ = [("max_iterations", C.c_int32), ("min_valid", C.c_int32), ("lambda0", C.c_double), ("eps_px", C.c_double)]


def photo_align_opts(**kw):
    """the defaults of hnet_photo_align_default_opts with the given fields replaced"""
    o = PhotoAlignOpts()
    lib().hnet_photo_align_default_opts(C.byref(o))
    for k, v in kw.items():
        if k not in ("max_iterations", "min_valid", "lambda0", "eps_px"):
            raise TypeError(f"hnet_photo_align_opts has no field {k!r}")
        setattr(o, k, v)
    return o


class PhotoRobustOpts(C.Structure):
    """hnet_photo_robust_opts: the alignment's options, the brightness model (0 off, 1 gain + bias), the Huber threshold in grey levels (0: quadratic) and
    the start gain and bias"""
    _fields_ = [("base", PhotoAlignOpts), ("brightness", C.c_int32), ("pad", C.c_int32), ("huber_k", C.c_double), ("gain0", C.c_double), ("bias0", C.c_double)]


def photo_robust_opts(**kw):
    """the defaults of hnet_photo_robust_default_opts with the given fields replaced (the fields of `base` by their own names)"""
    o = PhotoRobustOpts()
    lib().hnet_photo_robust_default_opts(C.byref(o))
    for k, v in kw.items():
        if k in ("max_iterations", "min_valid", "lambda0", "eps_px"):
            setattr(o.base, k, v)
        elif k in ("brightness", "huber_k", "gain0", "bias0"):
            setattr(o, k, v)
        else:
            raise TypeError(f"hnet_photo_robust_opts has no field {k!r}")
    return o


# hnet_photo_refine: the level-0 record of a fallback alignment, R_px, the fallback's innovation, flags REFINE_* (include/hnet.h HNET_REFINE_*)
PHOTO_REFINE_DTYPE = _np.dtype([("rec", PHOTO_ROBUST_DTYPE), ("r_px", "<f8", (8, 8)), ("innov", INNOVATION_DTYPE), ("flags", "<i4"), ("pad", "<i4")])
assert PHOTO_REFINE_DTYPE.itemsize == 1560 + 512 + 144 + 8
REFINE_ASKED, REFINE_APPLIED, REFINE_NIS_REJECTED, REFINE_S_SINGULAR = 1, 2, 4, 8
REFINE_BAD_K_NET_COV, REFINE_STOPPED, REFINE_NO_STEP, REFINE_MSE_ABOVE_MAX, REFINE_NO_FACTOR, REFINE_NON_FINITE = 16, 32, 64, 128, 256, 512
REFINE_UNUSABLE = 16 | 32 | 64 | 128 | 256 | 512


class PhotoRefineOpts(C.Structure):
    """hnet_photo_refine_opts: the alignment's options and levels (shared by the refining sessions of a call), and per session the scale on
    mse * inverse(info), the floor added to the diagonal (px) and the largest usable mse (0: no limit)"""
    _fields_ = [("align", PhotoRobustOpts), ("levels", C.c_int32), ("pad", C.c_int32), ("cov_scale", C.c_double), ("sigma_floor_px", C.c_double),
                ("max_mse", C.c_double)]


class RefineStats(C.Structure):
    """hnet_refine_stats: fallbacks asked for, applied, unusable, refused by the NIS gate; sum and maximum of the fallbacks' NIS"""
    _fields_ = [("asked", C.c_int64), ("applied", C.c_int64), ("unusable", C.c_int64), ("nis_rejected", C.c_int64), ("sum_nis", C.c_double), ("max_nis", C.c_double)]


def photo_refine_opts(**kw):
    """the defaults of hnet_photo_refine_default_opts (cov_scale = 0: the caller must choose it) with the given fields replaced (the fields of `align`
    and its `base` by their own names)"""
    o = PhotoRefineOpts()
    lib().hnet_photo_refine_default_opts(C.byref(o))
    for k, v in kw.items():
        if k in ("max_iterations", "min_valid", "lambda0", "eps_px"):
            setattr(o.align.base, k, v)
        elif k in ("brightness", "huber_k", "gain0", "bias0"):
            setattr(o.align, k, v)
        elif k in ("levels", "cov_scale", "sigma_floor_px", "max_mse"):
            setattr(o, k, v)
        else:
            raise TypeError(f"hnet_photo_refine_opts has no field {k!r}")
    return o


# hnet_keyframe_track: one record per tracked session (hnet_sessions_keyframe_track); flags KF_* (include/hnet.h HNET_KF_*)
KEYFRAME_TRACK_DTYPE = _np.dtype([("rec", PHOTO_ROBUST_DTYPE), ("start_px", "<f4", 8), ("key_px", "<f4", 8), ("h_origin_curr", "<f8", (3, 3)), ("overlap", "<f8"),
                                  ("age", "<i4"), ("keyframes", "<i4"), ("flags", "<i4"), ("pad", "<i4")])
assert KEYFRAME_TRACK_DTYPE.itemsize == 1560 + 160
KF_FIRST, KF_REKEYED, KF_BRIDGED, KF_GAP, KF_LOW_OVERLAP, KF_MAX_AGE = 1, 2, 4, 8, 16, 32
KF_NO_START, KF_STOPPED, KF_MSE_ABOVE_MAX, KF_NON_FINITE, KF_ORIGIN_RESTARTED = 64, 128, 256, 512, 1024
KF_LOST = 64 | 128 | 256 | 512


class KeyframeOpts(C.Structure):
    """hnet_keyframe_opts: the alignment's options and levels, whether the session re-keys by itself, the age (frames) and the overlap (fraction of the
    frame) at which it does, and the largest mse of a tracked frame (0: no limit)"""
    _fields_ = [("align", PhotoRobustOpts), ("levels", C.c_int32), ("auto_rekey", C.c_int32), ("max_age", C.c_int32), ("pad", C.c_int32),
                ("rekey_overlap", C.c_double), ("max_mse", C.c_double)]


assert C.sizeof(KeyframeOpts) == 56 + 32


def keyframe_opts(**kw):
    """the defaults of hnet_keyframe_default_opts with the given fields replaced (the fields of `align` and its `base` by their own names)"""
    o = KeyframeOpts()
    lib().hnet_keyframe_default_opts(C.byref(o))
    for k, v in kw.items():
        if k in ("max_iterations", "min_valid", "lambda0", "eps_px"):
            setattr(o.align.base, k, v)
        elif k in ("brightness", "huber_k", "gain0", "bias0"):
            setattr(o.align, k, v)
        elif k in ("levels", "auto_rekey", "max_age", "rekey_overlap", "max_mse"):
            setattr(o, k, v)
        else:
            raise TypeError(f"hnet_keyframe_opts has no field {k!r}")
    return o


# hnet_keyframe_measure: a session's in-step keyframe track as a filter measurement (hnet_filters_set_keyframe_measure): the track's record, the filter's
# step, z_px, R_px, the measurement's innovation, flags KFM_* (include/hnet.h HNET_KFM_*)
KEYFRAME_MEASURE_DTYPE = _np.dtype([("track", KEYFRAME_TRACK_DTYPE), ("step_px", "<f4", 8), ("z_px", "<f4", 8), ("r_px", "<f8", (8, 8)),
                                    ("innov", INNOVATION_DTYPE), ("flags", "<i4"), ("pad", "<i4")])
assert KEYFRAME_MEASURE_DTYPE.itemsize == 1720 + 64 + 512 + 144 + 8
KFM_ALWAYS, KFM_IF_NONE = 0, 1
KFM_ASKED, KFM_APPLIED, KFM_NIS_REJECTED, KFM_S_SINGULAR = 1, 2, 4, 8
KFM_BAD_K_NET_COV, KFM_STOPPED, KFM_NO_STEP, KFM_MSE_ABOVE_MAX, KFM_NO_FACTOR, KFM_NON_FINITE = 16, 32, 64, 128, 256, 512
KFM_FIRST, KFM_TRACK_LOST, KFM_TRACK_GAP, KFM_PREV_NOT_MEASURED, KFM_NO_INVERSE, KFM_NOT_SELECTED = 1024, 2048, 4096, 8192, 16384, 32768
KFM_UNUSABLE = 16 | 32 | 64 | 128 | 256 | 512 | 1024 | 2048 | 4096 | 8192 | 16384


class KeyframeMeasureOpts(C.Structure):
    """hnet_keyframe_measure_opts: the in-step track's options (shared by the measuring sessions of a call), and per session the scale on
    mse * inverse(info), the floor added to the diagonal (px), the largest usable mse (0: no limit) and when the measurement is applied"""
    _fields_ = [("track", KeyframeOpts), ("cov_scale", C.c_double), ("sigma_floor_px", C.c_double), ("max_mse", C.c_double), ("when", C.c_int32),
                ("pad", C.c_int32)]


assert C.sizeof(KeyframeMeasureOpts) == 88 + 32


class KeyframeMeasureStats(C.Structure):
    """hnet_keyframe_measure_stats: measurements asked for, applied, unusable, refused by the NIS gate; sum and maximum of their NIS"""
    _fields_ = [("asked", C.c_int64), ("applied", C.c_int64), ("unusable", C.c_int64), ("nis_rejected", C.c_int64), ("sum_nis", C.c_double), ("max_nis", C.c_double)]


def keyframe_measure_opts(**kw):
    """the defaults of hnet_keyframe_measure_default_opts (cov_scale = 0: the caller must choose it) with the given fields replaced: the track's by their
    own names (its max_mse as track_max_mse), the measurement's cov_scale, sigma_floor_px, max_mse and when"""
    o = KeyframeMeasureOpts()
    lib().hnet_keyframe_measure_default_opts(C.byref(o))
    for k, v in kw.items():
        if k in ("max_iterations", "min_valid", "lambda0", "eps_px"):
            setattr(o.track.align.base, k, v)
        elif k in ("brightness", "huber_k", "gain0", "bias0"):
            setattr(o.track.align, k, v)
        elif k in ("levels", "auto_rekey", "max_age", "rekey_overlap"):
            setattr(o.track, k, v)
        elif k == "track_max_mse":
            o.track.max_mse = v
        elif k in ("cov_scale", "sigma_floor_px", "max_mse", "when"):
            setattr(o, k, v)
        else:
            raise TypeError(f"hnet_keyframe_measure_opts has no field {k!r}")
    return o


# the keyframe map (hnet_sessions_enable_keyframe_map): a session's entries and map state (hnet_sessions_keyframe_map_info), and one record per revisited
# session (hnet_sessions_keyframe_revisit); flags RV_* (include/hnet.h HNET_RV_*)
KEYFRAME_MAP_ENTRY_DTYPE = _np.dtype([("valid", "<i4"), ("links", "<i4"), ("serial", "<i4"), ("pad", "<i4"), ("h_origin_key", "<f8", (3, 3))])
KEYFRAME_MAP_STATE_DTYPE = _np.dtype([("cur_slot", "<i4"), ("cur_links", "<i4"), ("cursor", "<i4"), ("serial", "<i4")])
KEYFRAME_REVISIT_DTYPE = _np.dtype([("rec", PHOTO_ROBUST_DTYPE), ("start_px", "<f4", 8), ("key_px", "<f4", 8), ("h_origin_before", "<f8", (3, 3)),
                                    ("h_origin_curr", "<f8", (3, 3)), ("closure_px", "<f8", 8), ("overlap", "<f8"), ("slot", "<i4"), ("links", "<i4"),
                                    ("grid", "<i4"), ("flags", "<i4"), ("pad", "<i4", 2)])
assert KEYFRAME_MAP_ENTRY_DTYPE.itemsize == 88 and KEYFRAME_MAP_STATE_DTYPE.itemsize == 16 and KEYFRAME_REVISIT_DTYPE.itemsize == 1560 + 304
RV_NO_CANDIDATE, RV_ATTACHED, RV_STOPPED, RV_MSE_ABOVE_MAX, RV_NON_FINITE, RV_LOW_OVERLAP, RV_CLOSURE_ABOVE_MAX, RV_CHAIN = 1, 2, 4, 8, 16, 32, 64, 128
RV_REJECTED = 4 | 8 | 16 | 32 | 64 | 128
KEYFRAME_MAP_MIN_CAPACITY, KEYFRAME_MAP_MAX_CAPACITY = 2, 8


class KeyframeRevisitOpts(C.Structure):
    """hnet_keyframe_revisit_opts: the alignment's options and levels, the fewest grid points (of 64) of a stored keyframe that must lie inside the current
    frame, the smallest overlap (fraction of the frame) of an accepted alignment, its largest mse and the largest distance (px) of its offsets from the
    predicted start (0: no limit, both)"""
    _fields_ = [("align", PhotoRobustOpts), ("levels", C.c_int32), ("min_grid", C.c_int32), ("min_overlap", C.c_double), ("max_mse", C.c_double),
                ("max_closure_px", C.c_double)]


assert C.sizeof(KeyframeRevisitOpts) == 56 + 32


def keyframe_revisit_opts(**kw):
    """the defaults of hnet_keyframe_revisit_default_opts with the given fields replaced (the fields of `align` and its `base` by their own names)"""
    o = KeyframeRevisitOpts()
    lib().hnet_keyframe_revisit_default_opts(C.byref(o))
    for k, v in kw.items():
        if k in ("max_iterations", "min_valid", "lambda0", "eps_px"):
            setattr(o.align.base, k, v)
        elif k in ("brightness", "huber_k", "gain0", "bias0"):
            setattr(o.align, k, v)
        elif k in ("levels", "min_grid", "min_overlap", "max_mse", "max_closure_px"):
            setattr(o, k, v)
        else:
            raise TypeError(f"hnet_keyframe_revisit_opts has no field {k!r}")
    return o


# a keyframe map rendered into a view (hnet_op_keyframe_render, hnet_sessions_keyframe_render): one record per rendered map; modes RENDER_*
# (include/hnet.h HNET_RENDER_*)
KEYFRAME_RENDER_DTYPE = _np.dtype([("h_origin_view", "<f8", (3, 3)), ("n_covered", "<u8"), ("n_overlap", "<u8"), ("n", "<u8", 8), ("sse", "<u8", 8),
                                   ("used_mask", "<i4"), ("skipped_mask", "<i4")])
assert KEYFRAME_RENDER_DTYPE.itemsize == 224
RENDER_FEWEST_LINKS, RENDER_NEWEST, RENDER_MEAN = 0, 1, 2
RENDER_MAX_DIM = 8192


class KeyframeLocaliseOpts(C.Structure):
    """hnet_keyframe_localise_opts: the masked alignment's options and levels, the render mode of the template, the smallest cover of the template and
    overlap of an accepted alignment (fractions of the frame), its largest mse and the largest |offset| (px; 0: no limit, both), and apply (0 / 1)"""
    _fields_ = [("align", PhotoRobustOpts), ("levels", C.c_int32), ("mode", C.c_int32), ("min_cover", C.c_double), ("min_overlap", C.c_double),
                ("max_mse", C.c_double), ("max_shift_px", C.c_double), ("apply", C.c_int32), ("pad", C.c_int32)]


assert C.sizeof(KeyframeLocaliseOpts) == 104
KEYFRAME_LOCALISE_DTYPE = _np.dtype([("rec", PHOTO_ROBUST_DTYPE), ("h_origin_before", "<f8", (3, 3)), ("h_origin_curr", "<f8", (3, 3)), ("correction_px", "<f8", 8),
                                     ("cover", "<f8"), ("overlap", "<f8"), ("used_mask", "<i4"), ("links_before", "<i4"), ("links", "<i4"), ("flags", "<i4"),
                                     ("pad", "<i4", 2)])
assert KEYFRAME_LOCALISE_DTYPE.itemsize == 1808
LOC_NO_MAP, LOC_LOW_COVER, LOC_STOPPED, LOC_MSE_ABOVE_MAX, LOC_NON_FINITE, LOC_LOW_OVERLAP, LOC_SHIFT_ABOVE_MAX, LOC_CHAIN, LOC_LOCALISED = 1, 2, 4, 8, 16, 32, 64, 128, 256


def keyframe_localise_opts(**kw):
    """the defaults of hnet_keyframe_localise_default_opts with the given fields replaced (the fields of `align` and its `base` by their own names)"""
    o = KeyframeLocaliseOpts()
    lib().hnet_keyframe_localise_default_opts(C.byref(o))
    for k, v in kw.items():
        if k in ("max_iterations", "min_valid", "lambda0", "eps_px"):
            setattr(o.align.base, k, v)
        elif k in ("brightness", "huber_k", "gain0", "bias0"):
            setattr(o.align, k, v)
        elif k in ("levels", "mode", "min_cover", "min_overlap", "max_mse", "max_shift_px", "apply"):
            setattr(o, k, v)
        else:
            raise TypeError(f"unknown option {k}")
    return o


class KeyframeRenderOpts(C.Structure):
    """hnet_keyframe_render_opts: the view's size and how the samples that cover a pixel are blended (RENDER_*)"""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("mode", C.c_int32), ("pad", C.c_int32)]


assert C.sizeof(KeyframeRenderOpts) == 16


def keyframe_render_fit_view(entries, width, height, margin_px=0.0):
    """hnet_keyframe_render_fit_view: the view [3, 3] of width x height pixels that shows every valid entry of `entries` (KEYFRAME_MAP_ENTRY_DTYPE) with
    margin_px free on every side, or None when there is none (no usable entry, a map or a view without extent)"""
    e = _np.ascontiguousarray(entries, dtype=KEYFRAME_MAP_ENTRY_DTYPE).reshape(-1)
    h = _np.zeros((3, 3))
    ok = lib().hnet_keyframe_render_fit_view(e.ctypes.data, len(e), int(width), int(height), float(margin_px), h.ctypes.data)
    return h if ok else None


# the joint adjustment of a keyframe map (hnet_op_keyframe_adjust_solve, hnet_op_keyframe_adjust, hnet_sessions_keyframe_adjust): one record per
# session with its table of 28 edges; verdicts ADJ_*, edge flags ADJ_EDGE_*, weightings ADJ_WEIGHT_* (include/hnet.h HNET_ADJ_*)
KEYFRAME_ADJUST_EDGE_DTYPE = _np.dtype([("i", "<i4"), ("j", "<i4"), ("grid", "<i4"), ("flags", "<i4"), ("start_px", "<f4", 8), ("offsets_px", "<f4", 8),
                                        ("mse", "<f8"), ("overlap", "<f8"), ("r0_px", "<f8"), ("r_px", "<f8")])
KEYFRAME_ADJUST_DTYPE = _np.dtype([("flags", "<i4"), ("anchor", "<i4"), ("n_pairs", "<i4"), ("n_jobs", "<i4"), ("n_edges", "<i4"), ("adjusted_mask", "<i4"),
                                   ("unconnected_mask", "<i4"), ("trials", "<i4"), ("accepted", "<i4"), ("pad", "<i4"), ("cost0", "<f8"), ("cost", "<f8"),
                                   ("lambda", "<f8"), ("delta_px", "<f8", (8, 8)), ("h_origin_key", "<f8", (8, 3, 3)), ("edge", KEYFRAME_ADJUST_EDGE_DTYPE, 28)])
assert KEYFRAME_ADJUST_EDGE_DTYPE.itemsize == 112 and KEYFRAME_ADJUST_DTYPE.itemsize == 40 + 24 + 512 + 576 + 28 * 112
ADJ_FEW_ENTRIES, ADJ_NO_EDGES, ADJ_SINGULAR, ADJ_NO_GAIN, ADJ_SHIFT_ABOVE_MAX, ADJ_CHAIN, ADJ_ADJUSTED, ADJ_CONVERGED = 1, 2, 4, 8, 16, 32, 64, 128
ADJ_EDGE_ACCEPTED, ADJ_EDGE_STOPPED, ADJ_EDGE_MSE_ABOVE_MAX, ADJ_EDGE_NON_FINITE, ADJ_EDGE_LOW_OVERLAP, ADJ_EDGE_CLOSURE_ABOVE_MAX = 1, 2, 4, 8, 16, 32
ADJ_EDGE_NO_RELATIVE = 64
ADJ_WEIGHT_UNIT, ADJ_WEIGHT_INFO = 0, 1
ADJ_MAX_EDGES, ADJ_MAX_TRIALS = 28, 64


class KeyframeAdjustOpts(C.Structure):
    """hnet_keyframe_adjust_opts: the alignment's options and levels and the revisit's gates for a pair and its edge (min_grid, min_overlap, max_mse,
    max_closure_px), the weighting of the edges (ADJ_WEIGHT_*) with the floor under an edge's mse, the solve's trials at the most, initial damping and
    convergence threshold (px), the largest accepted |delta| (px; 0: no limit) and whether the new matrices are written into the map"""
    _fields_ = [("align", PhotoRobustOpts), ("levels", C.c_int32), ("min_grid", C.c_int32), ("min_overlap", C.c_double), ("max_mse", C.c_double),
                ("max_closure_px", C.c_double), ("weighting", C.c_int32), ("max_trials", C.c_int32), ("mse_floor", C.c_double), ("lambda0", C.c_double),
                ("eps_px", C.c_double), ("max_shift_px", C.c_double), ("apply", C.c_int32), ("pad", C.c_int32)]


assert C.sizeof(KeyframeAdjustOpts) == 56 + 80


def keyframe_adjust_opts(**kw):
    """the defaults of hnet_keyframe_adjust_default_opts with the given fields replaced: the alignment's by their own names with its lambda0 and eps_px as
    align_lambda0 and align_eps_px, the adjustment's by theirs"""
    o = KeyframeAdjustOpts()
    lib().hnet_keyframe_adjust_default_opts(C.byref(o))
    for k, v in kw.items():
        if k in ("max_iterations", "min_valid"):
            setattr(o.align.base, k, v)
        elif k in ("align_lambda0", "align_eps_px"):
            setattr(o.align.base, k[6:], v)
        elif k in ("brightness", "huber_k", "gain0", "bias0"):
            setattr(o.align, k, v)
        elif k in ("levels", "min_grid", "min_overlap", "max_mse", "max_closure_px", "weighting", "max_trials", "mse_floor", "lambda0", "eps_px", "max_shift_px",
                   "apply"):
            setattr(o, k, v)
        else:
            raise TypeError(f"hnet_keyframe_adjust_opts has no field {k!r}")
    return o


# the coarse search over integer translations (hnet_op_photo_search): one record per pair; flags PS_* (include/hnet.h HNET_PS_*).  A score table is
# [PS_SHIFTS_Y, PS_SHIFTS_X] doubles, index [dy + PS_MAX_RY, dx + PS_MAX_RX]
PHOTO_SEARCH_DTYPE = _np.dtype([("start_px", "<f4", 8), ("dx", "<i4"), ("dy", "<i4"), ("dx2", "<i4"), ("dy2", "<i4"), ("n_overlap", "<i4"), ("flags", "<i4"),
                                ("score", "<f8"), ("second", "<f8"), ("sa", "<i4"), ("sb", "<i4"), ("sab", "<i4"), ("saa", "<i4"), ("sbb", "<i4"), ("pad", "<i4")])
assert PHOTO_SEARCH_DTYPE.itemsize == 96
PS_FOUND, PS_NO_TEXTURE, PS_LOW_SCORE, PS_AMBIGUOUS = 1, 2, 4, 8
PS_MAX_RX, PS_MAX_RY, PS_SHIFTS_X, PS_SHIFTS_Y = 30, 20, 61, 41
PS_THUMB_W, PS_THUMB_H = 40, 28


class PhotoSearchOpts(C.Structure):
    """hnet_photo_search_opts: the radii of the search and the fewest pixels of an overlap (level-3 pixels), the lowest score of a FOUND peak and the
    least margin over the best score elsewhere"""
    _fields_ = [("radius_x", C.c_int32), ("radius_y", C.c_int32), ("min_overlap", C.c_int32), ("pad", C.c_int32), ("min_score", C.c_double),
                ("min_margin", C.c_double)]


assert C.sizeof(PhotoSearchOpts) == 32
_SEARCH_FIELDS = ("radius_x", "radius_y", "min_overlap", "min_score", "min_margin")


def photo_search_opts(**kw):
    """the defaults of hnet_photo_search_default_opts with the given fields replaced"""
    o = PhotoSearchOpts()
    lib().hnet_photo_search_default_opts(C.byref(o))
    for k, v in kw.items():
        if k not in _SEARCH_FIELDS:
            raise TypeError(f"hnet_photo_search_opts has no field {k!r}")
        setattr(o, k, v)
    return o


# hnet_keyframe_relocalise: one record per listed session (hnet_sessions_keyframe_relocalise); rv.flags RL_* (include/hnet.h HNET_RL_*)
KEYFRAME_RELOC_DTYPE = _np.dtype([("rv", KEYFRAME_REVISIT_DTYPE), ("search", PHOTO_SEARCH_DTYPE), ("target", "<i4"), ("n_searched", "<i4"), ("n_found", "<i4"),
                                  ("pad", "<i4")])
assert KEYFRAME_RELOC_DTYPE.itemsize == 1864 + 96 + 16
RL_NO_CANDIDATE, RL_ATTACHED, RL_STOPPED, RL_MSE_ABOVE_MAX, RL_NON_FINITE, RL_LOW_OVERLAP, RL_CLOSURE_ABOVE_MAX, RL_CHAIN, RL_RETRACKED = 1, 2, 4, 8, 16, 32, 64, 128, 256
RL_REJECTED = 4 | 8 | 16 | 32 | 64 | 128
RL_TARGET_HELD, RL_TARGET_NONE = -1, -2


class KeyframeRelocOpts(C.Structure):
    """hnet_keyframe_relocalise_opts: the alignment's options and levels, the search's options, the smallest overlap (fraction of the frame) of an accepted
    alignment, its largest mse and the largest distance (px) of its offsets from the searched start (0: no limit, both)"""
    _fields_ = [("align", PhotoRobustOpts), ("levels", C.c_int32), ("pad", C.c_int32), ("search", PhotoSearchOpts), ("min_overlap", C.c_double),
                ("max_mse", C.c_double), ("max_closure_px", C.c_double)]


assert C.sizeof(KeyframeRelocOpts) == 56 + 64


def keyframe_relocalise_opts(**kw):
    """the defaults of hnet_keyframe_relocalise_default_opts with the given fields replaced (the fields of `align`, its `base` and `search` by their own
    names; the search's min_overlap as search_min_overlap)"""
    o = KeyframeRelocOpts()
    lib().hnet_keyframe_relocalise_default_opts(C.byref(o))
    for k, v in kw.items():
        if k in ("max_iterations", "min_valid", "lambda0", "eps_px"):
            setattr(o.align.base, k, v)
        elif k in ("brightness", "huber_k", "gain0", "bias0"):
            setattr(o.align, k, v)
        elif k in ("levels", "min_overlap", "max_mse", "max_closure_px"):
            setattr(o, k, v)
        elif k == "search_min_overlap":
            o.search.min_overlap = v
        elif k in _SEARCH_FIELDS:
            setattr(o.search, k, v)
        else:
            raise TypeError(f"hnet_keyframe_relocalise_opts has no field {k!r}")
    return o


# the search under a table of orientation hypotheses (hnet_op_photo_search_oriented): a table entry, and one record per pair: 7r's record of the winning
# entry, then the winner's index, the entries with a scored shift, the runner-up's index and score, and the winner's matrix
PHOTO_SEARCH_HYP_DTYPE = _np.dtype([("a", "<f8", 4), ("b", "<i4", 4)])
PHOTO_SEARCH_ORIENTED_DTYPE = _np.dtype([("base", PHOTO_SEARCH_DTYPE), ("hyp", "<i4"), ("n_scored", "<i4"), ("hyp2", "<i4"), ("pad0", "<i4"), ("score2", "<f8"),
                                         ("a", "<f8", 4), ("pad", "<i4", 2)])
KEYFRAME_RELOC_ORIENTED_DTYPE = _np.dtype([("rv", KEYFRAME_REVISIT_DTYPE), ("search", PHOTO_SEARCH_ORIENTED_DTYPE), ("target", "<i4"), ("n_searched", "<i4"),
                                           ("n_found", "<i4"), ("pad", "<i4")])
assert PHOTO_SEARCH_HYP_DTYPE.itemsize == 48 and PHOTO_SEARCH_ORIENTED_DTYPE.itemsize == 160 and KEYFRAME_RELOC_ORIENTED_DTYPE.itemsize == 1864 + 160 + 16
PS_MAX_HYP, PS_DEFAULT_HYP = 64, 60


def photo_search_hyp(angle_rad, scale=1.0):
    """one table entry (hnet_photo_search_make_hyp) -> [1] of PHOTO_SEARCH_HYP_DTYPE; ValueError for a non-finite angle or a scale outside [0.5, 2]"""
    out = _np.zeros(1, PHOTO_SEARCH_HYP_DTYPE)
    if not lib().hnet_photo_search_make_hyp(float(angle_rad), float(scale), out.ctypes.data):
        raise ValueError("hnet_photo_search_make_hyp: a finite angle and 0.5 <= scale <= 2")
    return out


def photo_search_yaw_table(first_deg=-180.0, step_deg=6.0, count=PS_DEFAULT_HYP):
    """`count` entries of scale 1 at first_deg + k step_deg degrees (hnet_photo_search_yaw_table); the defaults are the documented default table"""
    if not 1 <= int(count) <= PS_MAX_HYP:
        raise ValueError("hnet_photo_search_yaw_table: 1 <= count <= 64")
    out = _np.zeros(int(count), PHOTO_SEARCH_HYP_DTYPE)
    if not lib().hnet_photo_search_yaw_table(float(first_deg), float(step_deg), int(count), out.ctypes.data):
        raise ValueError("hnet_photo_search_yaw_table: finite angles")
    return out


def photo_search_table(hyps):
    """the table a call passes on: None = the default yaw table; else [n_hyp] of PHOTO_SEARCH_HYP_DTYPE as it is (the library refuses what it must)"""
    if hyps is None:
        return photo_search_yaw_table()
    return _np.ascontiguousarray(hyps, PHOTO_SEARCH_HYP_DTYPE).reshape(-1)


# the fine stage around the oriented winner (hnet_op_photo_search_fine): the oriented record, then the fine part: the final start, flags PSF_* (include/hnet.h
# HNET_PSF_*), the best fine entry j and its offsets (ex, ey), the level-2 shift, the overlap, the score, the fine entry's matrix and the sums.  A fine
# score table is [n_fine, 9, 9] doubles, index [j, ey + 4, ex + 4]
PHOTO_SEARCH_FINE_PART_DTYPE = _np.dtype([("start_px", "<f4", 8), ("flags", "<i4"), ("j", "<i4"), ("ex", "<i4"), ("ey", "<i4"), ("sx", "<i4"), ("sy", "<i4"),
                                          ("n_overlap", "<i4"), ("pad0", "<i4"), ("score", "<f8"), ("a", "<f8", 4), ("sa", "<i4"), ("sb", "<i4"), ("sab", "<i4"),
                                          ("saa", "<i4"), ("sbb", "<i4"), ("pad1", "<i4")])
PHOTO_SEARCH_FINE_DTYPE = _np.dtype([("coarse", PHOTO_SEARCH_ORIENTED_DTYPE), ("fine", PHOTO_SEARCH_FINE_PART_DTYPE)])
KEYFRAME_RELOC_FINE_DTYPE = _np.dtype([("base", KEYFRAME_RELOC_ORIENTED_DTYPE), ("fine", PHOTO_SEARCH_FINE_PART_DTYPE)])
assert PHOTO_SEARCH_FINE_PART_DTYPE.itemsize == 128 and PHOTO_SEARCH_FINE_DTYPE.itemsize == 288 and KEYFRAME_RELOC_FINE_DTYPE.itemsize == 2040 + 128
PSF_REFINED, PSF_SKIPPED, PSF_NOTHING_SCORED, PSF_LOW_SCORE = 1, 2, 4, 8
PSF_MAX_FINE, PSF_MAX_RADIUS, PSF_SHIFTS = 9, 4, 9


class PhotoSearchFineOpts(C.Structure):
    """hnet_photo_search_fine_opts: the radius of the fine shifts (level-2 pixels), the entries per row of the fine table and the lowest score of a
    REFINED result (the coarse default, not calibrated for level 2)"""
    _fields_ = [("radius", C.c_int32), ("n_fine", C.c_int32), ("min_score", C.c_double), ("pad", C.c_int32 * 2)]


assert C.sizeof(PhotoSearchFineOpts) == 24


def photo_search_fine_opts(**kw):
    """the defaults of hnet_photo_search_fine_default_opts with the given fields (radius, n_fine, min_score) replaced"""
    o = PhotoSearchFineOpts()
    lib().hnet_photo_search_fine_default_opts(C.byref(o))
    for k, v in kw.items():
        if k not in ("radius", "n_fine", "min_score"):
            raise TypeError(f"hnet_photo_search_fine_opts has no field {k!r}")
        setattr(o, k, v)
    return o


def photo_search_fine_yaw_table(first_deg=-180.0, step_deg=6.0, count=PS_DEFAULT_HYP, n_fine=5):
    """[count, n_fine] entries around those of photo_search_yaw_table(first_deg, step_deg, count) (hnet_photo_search_fine_yaw_table)"""
    if not 1 <= int(count) <= PS_MAX_HYP or not 1 <= int(n_fine) <= PSF_MAX_FINE:
        raise ValueError("hnet_photo_search_fine_yaw_table: 1 <= count <= 64, 1 <= n_fine <= 9")
    out = _np.zeros((int(count), int(n_fine)), PHOTO_SEARCH_HYP_DTYPE)
    if not lib().hnet_photo_search_fine_yaw_table(float(first_deg), float(step_deg), int(count), int(n_fine), out.ctypes.data):
        raise ValueError("hnet_photo_search_fine_yaw_table: finite angles")
    return out


def photo_search_fine_table(fine, hyps, n_fine, step_deg=None):
    """the fine table a call passes on -> [n_hyp, n_fine] of PHOTO_SEARCH_HYP_DTYPE.  fine given: as it is (the library refuses what it must).  fine None:
    the table that matches `hyps`: for hyps None the default tables' (photo_search_fine_yaw_table()); else entry [h, j] is hyps[h] turned by
    (j - (n_fine - 1) / 2) (step_deg / n_fine) degrees at its own scale, step_deg defaulting to the smallest angle between two neighbouring entries of
    hyps (6 degrees for a single entry), and for odd n_fine the middle entry is hyps[h] itself"""
    n_fine = int(n_fine)
    if fine is not None:
        return _np.ascontiguousarray(fine, PHOTO_SEARCH_HYP_DTYPE).reshape(-1, n_fine)
    if hyps is None:
        return photo_search_fine_yaw_table(n_fine=n_fine)
    h = photo_search_table(hyps)
    deg = _np.rad2deg(_np.arctan2(h["a"][:, 2], h["a"][:, 0]))
    scale = _np.hypot(h["a"][:, 0], h["a"][:, 2])
    if step_deg is None:
        d = _np.abs((_np.diff(deg) + 180.0) % 360.0 - 180.0)
        step_deg = float(d[d > 0].min()) if (d > 0).any() else 6.0
    out = _np.zeros((len(h), n_fine), PHOTO_SEARCH_HYP_DTYPE)
    for k in range(len(h)):
        for j in range(n_fine):
            off = (j - (n_fine - 1) / 2.0) * (step_deg / n_fine)
            out[k, j] = h[k] if off == 0.0 else photo_search_hyp(_np.deg2rad(deg[k] + off), min(max(float(scale[k]), 0.5), 2.0))[0]
    return out


# hnet_keyframe_recover: one record per listed session of a track with recovery (hnet_sessions_keyframe_track_recover): the track's record, whose flags may
# hold KF_RECOVERED, and the oriented relocalise's (all zero but target = -2 for a session that was not lost)
KF_RECOVERED = 2048
KEYFRAME_RECOVER_DTYPE = _np.dtype([("track", KEYFRAME_TRACK_DTYPE), ("reloc", KEYFRAME_RELOC_ORIENTED_DTYPE)])
assert KEYFRAME_RECOVER_DTYPE.itemsize == 1720 + 2040


class KeyframeRecoverOpts(C.Structure):
    """hnet_keyframe_recover_opts: the track's options and the relocalise's"""
    _fields_ = [("track", KeyframeOpts), ("reloc", KeyframeRelocOpts)]


assert C.sizeof(KeyframeRecoverOpts) == 88 + 120


def keyframe_recover_opts(track=None, reloc=None):
    """the defaults of hnet_keyframe_recover_default_opts with either block replaced: a KeyframeOpts / KeyframeRelocOpts as it is, or a dict in the keyword
    form of keyframe_opts / keyframe_relocalise_opts"""
    o = KeyframeRecoverOpts()
    lib().hnet_keyframe_recover_default_opts(C.byref(o))
    if track is not None:
        o.track = track if isinstance(track, KeyframeOpts) else keyframe_opts(**track)
    if reloc is not None:
        o.reloc = reloc if isinstance(reloc, KeyframeRelocOpts) else keyframe_relocalise_opts(**reloc)
    return o


# hnet_keyframe_measure_recover: a measuring session's record with recovery inside its in-step track (hnet_filters_set_keyframe_recover): the measure
# record, whose track may hold KF_RECOVERED and whose flags may hold the two bits below, and the oriented relocalise's record
KFM_FROM_RELOC, KFM_REATTACHED = 65536, 131072
KFMR_UNUSABLE = KFM_UNUSABLE | KFM_REATTACHED
KEYFRAME_MEASURE_RECOVER_DTYPE = _np.dtype([("m", KEYFRAME_MEASURE_DTYPE), ("reloc", KEYFRAME_RELOC_ORIENTED_DTYPE)])
assert KEYFRAME_MEASURE_RECOVER_DTYPE.itemsize == 2448 + 2040


def photo_robust_marginal(rec):
    """hnet_photo_robust_marginal of one record -> (info8 [8, 8], grad8 [8]); ValueError when the brightness block has no Cholesky factor"""
    r = _np.ascontiguousarray(rec, PHOTO_ROBUST_DTYPE).reshape(1)
    info, grad = _np.zeros((8, 8)), _np.zeros(8)
    if lib().hnet_photo_robust_marginal(C.c_void_p(r.ctypes.data), C.c_void_p(info.ctypes.data), C.c_void_p(grad.ctypes.data)) != 0:
        raise ValueError("hnet_photo_robust_marginal: the brightness block has no Cholesky factor")
    return info, grad


# the block-4 input planes (csrc/kernels.h B4_*): [plane][pair][B4_HP][B4_WP] dwords, pixel (u, v) at row v + B4_PADY, column u + B4_PADX
# (tests/cpp/b41_tap_check.cpp pins these numbers to the header)
B4_HP, B4_WP, B4_PADX, B4_PADY = 235, 336, 5, 5
B4_SENTINEL = 0xA5A5A5A5      # what hnet_op_prep_batch fills its plane buffer with before the launch


class HnetError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__(f"hnet status {status}: {msg}")
        self.status = status


_lib = None


def lib():
    """load libhnet_hip.so (built by __graft_entry__.build() / csrc/Makefile); fail loudly when absent"""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} not found: build the HIP extension first "
                          "(python -c 'import __graft_entry__ as g; g.build()'); there is no CPU fallback")
    L = C.CDLL(LIB_PATH)
    vp, fp, u8p, dp = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_double)
    L.hnet_default_config.argtypes = [C.POINTER(Config)]
    L.hnet_default_config.restype = None
    L.hnet_create.argtypes = [C.POINTER(Config), C.c_char_p, C.POINTER(vp)]
    L.hnet_create_from_memory.argtypes = [C.POINTER(Config), vp, C.c_size_t, C.POINTER(vp)]
    L.hnet_destroy.argtypes = [vp]
    L.hnet_destroy.restype = None
    L.hnet_status_string.argtypes = [C.c_int]
    L.hnet_status_string.restype = C.c_char_p
    L.hnet_last_error.argtypes = [vp]
    L.hnet_last_error.restype = C.c_char_p
    L.hnet_version.restype = C.c_char_p
    L.hnet_push_image.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_double]
    L.hnet_set_camera.argtypes = [vp, C.POINTER(Camera)]
    L.hnet_set_undistort_maps.argtypes = [vp, fp, fp, C.c_int, C.c_int]
    L.hnet_get_undistort_maps.argtypes = [vp, fp, fp]
    L.hnet_push_raw_image.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_double]
    L.hnet_op_undistort.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp]
    L.hnet_attach_images.argtypes = [vp, vp]
    L.hnet_image_count.argtypes = [vp]
    L.hnet_precision.argtypes = [vp]
    L.hnet_latest_time.argtypes = [vp]
    L.hnet_latest_time.restype = C.c_double
    L.hnet_infer.argtypes = [vp, dp, C.c_int, fp, fp, u8p]
    L.hnet_infer_batch.argtypes = [vp, vp, vp, C.c_int, fp, C.c_int, C.c_uint64, fp, fp, fp]
    L.hnet_infer_batch_device.argtypes = [vp, vp, vp, C.c_int, vp, C.c_int, C.c_uint64, vp, vp, vp, vp]
    L.hnet_infer_mc_partial_device.argtypes = [vp, vp, vp, C.c_int, vp, C.c_int, C.c_uint64, vp, vp, vp, vp]
    L.hnet_mc_finish_device.argtypes = [vp, vp, vp, C.c_int, vp, C.c_int, vp, vp, vp]
    L.hnet_infer_batch_packed_device.argtypes = [vp, vp, vp, C.c_int, vp, C.c_int, C.c_uint64, vp, vp, vp]
    L.hnet_mc_finish_packed_device.argtypes = [vp, vp, vp, C.c_int, vp, C.c_int, vp, vp]
    L.hnet_mc_finish_gathered_device.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_int, vp, vp]
    L.hnet_get_config.argtypes = [vp, C.POINTER(Config)]
    L.hnet_synchronize.argtypes = [vp, vp]
    L.hnet_overflow_flag.argtypes = [vp, vp, C.POINTER(C.c_int)]
    L.hnet_last_timing.argtypes = [vp, C.POINTER(Timing)]
    L.hnet_time_batch_device.argtypes = [vp, vp, vp, C.c_int, vp, C.c_int, C.c_uint64, vp, vp, C.c_int, fp, fp]
    L.hnet_stage_count.argtypes = [vp]
    L.hnet_stage_name.argtypes = [vp, C.c_int]
    L.hnet_stage_name.restype = C.c_char_p
    L.hnet_stage_flops_per_pair.argtypes = [vp, C.c_int]
    L.hnet_stage_kernels.argtypes = [vp, C.c_int]
    L.hnet_stage_flops_per_pair.restype = C.c_double
    L.hnet_profile_batch_device.argtypes = [vp, vp, vp, C.c_int, vp, C.c_int, C.c_uint64, vp, vp, C.c_int, fp]
    L.hnet_op_warp.argtypes = [vp, fp, fp, fp]
    L.hnet_op_dlt.argtypes = [vp, fp, C.c_int, fp]
    L.hnet_op_conv.argtypes = [vp, C.c_int, fp, C.c_int, C.c_int, C.c_int, fp]
    L.hnet_op_block4_fused.argtypes = [vp, fp, C.c_int, C.c_int, fp]
    L.hnet_op_block3_fused.argtypes = [vp, fp, C.c_int, fp]
    L.hnet_op_block42_fused.argtypes = [vp, fp, C.c_int, fp]
    L.hnet_op_prep.argtypes = [vp, fp, fp, fp, C.c_int, fp]
    L.hnet_op_prep_u8.argtypes = [vp, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), fp, C.c_int, fp]
    L.hnet_op_prep_batch.argtypes = [vp, vp, vp, C.c_int, fp, C.c_int, C.c_int, C.c_int, fp, vp]
    L.hnet_debug_layer_output.argtypes = [vp, C.c_int, C.c_int, fp, C.c_size_t]
    L.hnet_debug_h_part1.argtypes = [vp, C.c_int, fp]
    L.hnet_create_group.argtypes = [C.POINTER(Config), C.c_char_p, C.c_int, C.POINTER(vp)]
    L.hnet_create_group_from_memory.argtypes = [C.POINTER(Config), vp, C.c_size_t, C.c_int, C.POINTER(vp)]
    L.hnet_destroy_group.argtypes = [vp]
    L.hnet_destroy_group.restype = None
    L.hnet_group_size.argtypes = [vp]
    L.hnet_group_context.argtypes = [vp, C.c_int]
    L.hnet_group_context.restype = vp
    L.hnet_group_stream.argtypes = [vp, C.c_int]
    L.hnet_group_stream.restype = vp
    L.hnet_group_last_error.argtypes = [vp]
    L.hnet_group_last_error.restype = C.c_char_p
    L.hnet_group_infer_batch_packed_device.argtypes = [vp, vp, vp, C.c_int, vp, C.c_int, C.c_uint64, vp, vp, C.POINTER(C.c_int)]
    L.hnet_group_join.argtypes = [vp, vp]
    L.hnet_group_synchronize.argtypes = [vp]
    L.hnet_group_overflow_flag.argtypes = [vp, C.POINTER(C.c_int)]
    L.hnet_create_sessions.argtypes = [vp, C.c_int, C.POINTER(vp)]
    L.hnet_destroy_sessions.argtypes = [vp]
    L.hnet_destroy_sessions.restype = None
    L.hnet_sessions_push.argtypes = [vp, C.c_int, vp, vp, C.c_int, C.c_size_t, vp]
    L.hnet_sessions_add_camera.argtypes = [vp, C.POINTER(Camera), C.POINTER(C.c_int)]
    L.hnet_sessions_bind_camera.argtypes = [vp, C.c_int, C.c_int]
    L.hnet_sessions_push_raw.argtypes = [vp, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, C.c_size_t, vp]
    L.hnet_sessions_infer.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp]
    L.hnet_sessions_set_iterative_model.argtypes = [vp, vp]
    L.hnet_sessions_infer_iter.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, vp, vp]
    L.hnet_sessions_image_count.argtypes = [vp, C.c_int]
    L.hnet_sessions_latest_time.argtypes = [vp, C.c_int]
    L.hnet_sessions_latest_time.restype = C.c_double
    L.hnet_sessions_set_seq.argtypes = [vp, C.c_int, C.c_uint64]
    L.hnet_sessions_seq.argtypes = [vp, C.c_int]
    L.hnet_sessions_seq.restype = C.c_uint64
    L.hnet_sessions_reset.argtypes = [vp, C.c_int]
    L.hnet_sessions_get_frame.argtypes = [vp, C.c_int, C.c_int, vp]
    L.hnet_sessions_last_timing.argtypes = [vp, C.POINTER(Timing)]
    L.hnet_infer_batch_seqs_packed_device.argtypes = [vp, vp, vp, C.c_int, vp, C.c_int, vp, vp, vp, vp]
    L.hnet_filter_default_params.argtypes = [C.POINTER(FilterParams)]
    L.hnet_filter_default_params.restype = None
    L.hnet_create_filters.argtypes = [vp, C.c_int, C.POINTER(vp)]
    L.hnet_destroy_filters.argtypes = [vp]
    L.hnet_destroy_filters.restype = None
    L.hnet_filters_set_params.argtypes = [vp, C.c_int, C.POINTER(FilterParams)]
    L.hnet_filters_set_state.argtypes = [vp, C.c_int, vp]
    L.hnet_filters_get_state.argtypes = [vp, C.c_int, vp, vp]
    L.hnet_filters_step.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp, vp]
    L.hnet_filters_last_priors.argtypes = [vp, C.c_int, vp]
    L.hnet_filters_last_timing.argtypes = [vp, C.POINTER(Timing)]
    L.hnet_filter_default_init_params.argtypes = [C.POINTER(InitParams)]
    L.hnet_filter_default_init_params.restype = None
    L.hnet_filters_enable_feed.argtypes = [vp, C.c_int]
    L.hnet_filters_set_init_params.argtypes = [vp, C.c_int, C.POINTER(InitParams)]
    L.hnet_filters_feed_imu.argtypes = [vp, C.c_int, vp, vp, vp]
    L.hnet_filters_initialized.argtypes = [vp, C.c_int]
    L.hnet_filters_uninitialize.argtypes = [vp, C.c_int]
    L.hnet_filters_advance.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp]
    L.hnet_filters_last_selection.argtypes = [vp, C.c_int, vp, C.c_int, C.POINTER(C.c_int)]
    L.hnet_filters_predict.argtypes = [vp, C.c_int, vp, vp, vp]
    L.hnet_filters_newest_imu_time.argtypes = [vp, C.c_int]
    L.hnet_filters_newest_imu_time.restype = C.c_double
    L.hnet_filters_last_predict_device_ms.argtypes = [vp]
    L.hnet_filters_last_predict_device_ms.restype = C.c_double
    L.hnet_filters_predict_cov.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp]
    L.hnet_filters_last_predict_cov_device_ms.argtypes = [vp]
    L.hnet_filters_last_predict_cov_device_ms.restype = C.c_double
    L.hnet_filters_enable_innovations.argtypes = [vp]
    L.hnet_filters_set_nis_gate.argtypes = [vp, C.c_int, C.c_double]
    L.hnet_filters_last_innovations.argtypes = [vp, C.c_int, vp]
    L.hnet_filters_innovation_stats.argtypes = [vp, C.c_int, C.POINTER(InnovationStats)]
    L.hnet_filters_reset_innovation_stats.argtypes = [vp, C.c_int]
    L.hnet_op_photo_residual.argtypes = [vp, vp, vp, C.c_int, fp, C.c_int, vp, vp]
    L.hnet_sessions_photo_residual.argtypes = [vp, C.c_int, vp, fp, C.c_int, vp]
    L.hnet_filters_enable_photometric.argtypes = [vp]
    L.hnet_filters_last_photometric.argtypes = [vp, C.c_int, vp]
    L.hnet_filters_set_photo_gate.argtypes = [vp, C.c_int, C.c_double, C.c_int32]
    L.hnet_filters_photo_stats.argtypes = [vp, C.c_int, C.POINTER(PhotoStats)]
    L.hnet_filters_reset_photo_stats.argtypes = [vp, C.c_int]
    L.hnet_filters_set_photo_gate_taps.argtypes = [vp, C.c_int]
    L.hnet_photo_align_default_opts.argtypes = [C.POINTER(PhotoAlignOpts)]
    L.hnet_photo_align_default_opts.restype = None
    L.hnet_op_photo_align.argtypes = [vp, vp, vp, C.c_int, vp, vp, vp]
    L.hnet_sessions_photo_align.argtypes = [vp, C.c_int, vp, vp, vp, vp]
    L.hnet_last_photo_align_device_ms.argtypes = [vp]
    L.hnet_op_photo_align_pyramid.argtypes = [vp, vp, vp, C.c_int, vp, vp, C.c_int, vp, vp]
    L.hnet_sessions_photo_align_pyramid.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int, vp, vp]
    L.hnet_op_photo_pyramid.argtypes = [vp, vp, C.c_int, vp]
    L.hnet_photo_robust_default_opts.argtypes = [C.POINTER(PhotoRobustOpts)]
    L.hnet_photo_robust_default_opts.restype = None
    L.hnet_op_photo_align_robust.argtypes = [vp, vp, vp, C.c_int, vp, vp, C.c_int, vp, vp]
    L.hnet_op_photo_align_masked.argtypes = [vp, vp, vp, vp, C.c_int, vp, vp, C.c_int, vp, vp]
    L.hnet_keyframe_localise_default_opts.argtypes = [C.POINTER(KeyframeLocaliseOpts)]
    L.hnet_keyframe_localise_default_opts.restype = None
    L.hnet_op_keyframe_localise.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp]
    L.hnet_sessions_enable_keyframe_localise.argtypes = [vp]
    L.hnet_sessions_keyframe_localise.argtypes = [vp, C.c_int, vp, vp, vp]
    L.hnet_sessions_photo_align_robust.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int, vp, vp]
    L.hnet_photo_robust_marginal.argtypes = [vp, vp, vp]
    L.hnet_keyframe_default_opts.argtypes = [C.POINTER(KeyframeOpts)]
    L.hnet_keyframe_default_opts.restype = None
    L.hnet_sessions_enable_keyframes.argtypes = [vp]
    L.hnet_sessions_keyframe_track.argtypes = [vp, C.c_int, vp, vp, vp, vp]
    L.hnet_sessions_keyframe_reset.argtypes = [vp, C.c_int]
    L.hnet_sessions_get_keyframe.argtypes = [vp, C.c_int, vp]
    L.hnet_sessions_last_keyframe_device_ms.argtypes = [vp]
    L.hnet_sessions_last_keyframe_device_ms.restype = C.c_double
    L.hnet_keyframe_revisit_default_opts.argtypes = [C.POINTER(KeyframeRevisitOpts)]
    L.hnet_keyframe_revisit_default_opts.restype = None
    L.hnet_sessions_enable_keyframe_map.argtypes = [vp, C.c_int]
    L.hnet_sessions_keyframe_revisit.argtypes = [vp, C.c_int, vp, vp, vp]
    L.hnet_sessions_keyframe_map_info.argtypes = [vp, C.c_int, vp, vp]
    L.hnet_sessions_get_map_keyframe.argtypes = [vp, C.c_int, C.c_int, vp]
    L.hnet_photo_search_default_opts.argtypes = [C.POINTER(PhotoSearchOpts)]
    L.hnet_photo_search_default_opts.restype = None
    L.hnet_op_photo_search.argtypes = [vp, vp, vp, C.c_int, vp, vp, vp]
    L.hnet_sessions_photo_search.argtypes = [vp, C.c_int, vp, vp, vp]
    L.hnet_keyframe_relocalise_default_opts.argtypes = [C.POINTER(KeyframeRelocOpts)]
    L.hnet_keyframe_relocalise_default_opts.restype = None
    L.hnet_sessions_keyframe_relocalise.argtypes = [vp, C.c_int, vp, vp, vp]
    L.hnet_photo_search_make_hyp.argtypes = [C.c_double, C.c_double, vp]
    L.hnet_photo_search_yaw_table.argtypes = [C.c_double, C.c_double, C.c_int, vp]
    L.hnet_photo_search_default_yaw_table.argtypes = [vp]
    L.hnet_op_photo_search_oriented.argtypes = [vp, vp, vp, C.c_int, vp, vp, C.c_int, vp, vp]
    L.hnet_sessions_photo_search_oriented.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int, vp]
    L.hnet_sessions_keyframe_relocalise_oriented.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int, vp]
    L.hnet_photo_search_fine_default_opts.argtypes = [C.POINTER(PhotoSearchFineOpts)]
    L.hnet_photo_search_fine_default_opts.restype = None
    L.hnet_photo_search_fine_yaw_table.argtypes = [C.c_double, C.c_double, C.c_int, C.c_int, vp]
    L.hnet_op_photo_search_fine.argtypes = [vp, vp, vp, C.c_int, vp, vp, C.c_int, vp, vp, vp, vp]
    L.hnet_sessions_photo_search_fine.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int, vp, vp, vp]
    L.hnet_sessions_keyframe_relocalise_fine.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int, vp, vp, vp]
    L.hnet_keyframe_recover_default_opts.argtypes = [C.POINTER(KeyframeRecoverOpts)]
    L.hnet_keyframe_recover_default_opts.restype = None
    L.hnet_sessions_keyframe_track_recover.argtypes = [vp, C.c_int, vp, vp, vp, vp, C.c_int, vp]
    L.hnet_last_photo_align_device_ms.restype = C.c_double
    L.hnet_photo_refine_default_opts.argtypes = [C.POINTER(PhotoRefineOpts)]
    L.hnet_photo_refine_default_opts.restype = None
    L.hnet_filters_set_photo_refine.argtypes = [vp, C.c_int, C.POINTER(PhotoRefineOpts)]
    L.hnet_filters_last_refine.argtypes = [vp, C.c_int, vp]
    L.hnet_filters_refine_stats.argtypes = [vp, C.c_int, C.POINTER(RefineStats)]
    L.hnet_filters_reset_refine_stats.argtypes = [vp, C.c_int]
    L.hnet_keyframe_measure_default_opts.argtypes = [C.POINTER(KeyframeMeasureOpts)]
    L.hnet_keyframe_measure_default_opts.restype = None
    L.hnet_filters_set_keyframe_measure.argtypes = [vp, C.c_int, C.POINTER(KeyframeMeasureOpts)]
    L.hnet_filters_last_keyframe_measure.argtypes = [vp, C.c_int, vp]
    L.hnet_filters_keyframe_measure_stats.argtypes = [vp, C.c_int, C.POINTER(KeyframeMeasureStats)]
    L.hnet_filters_reset_keyframe_measure_stats.argtypes = [vp, C.c_int]
    L.hnet_filters_set_keyframe_recover.argtypes = [vp, C.c_int, vp, vp, C.c_int]
    L.hnet_filters_last_keyframe_recover.argtypes = [vp, C.c_int, vp]
    L.hnet_keyframe_render_fit_view.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_double, vp]
    L.hnet_op_keyframe_render.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp, vp]
    L.hnet_sessions_enable_keyframe_render.argtypes = [vp, C.c_int, C.c_int]
    L.hnet_sessions_keyframe_render.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp]
    L.hnet_keyframe_adjust_default_opts.argtypes = [vp]
    L.hnet_keyframe_adjust_default_opts.restype = None
    L.hnet_op_keyframe_adjust_solve.argtypes = [vp, C.c_int, vp, C.c_int, vp, vp, vp, vp]
    L.hnet_op_keyframe_adjust.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp]
    L.hnet_sessions_enable_keyframe_adjust.argtypes = [vp]
    L.hnet_sessions_keyframe_adjust.argtypes = [vp, C.c_int, vp, vp, vp, vp]
    for name in SYMBOLS:
        getattr(L, name)   # AttributeError here = the library does not export what include/hnet.h declares
    _lib = L
    return L


def check(ctx, status):
    if status != HNET_OK:
        L = lib()
        msg = L.hnet_status_string(status).decode()
        detail = L.hnet_last_error(ctx).decode() if ctx else ""
        raise HnetError(status, f"{msg}{': ' + detail if detail else ''}")
