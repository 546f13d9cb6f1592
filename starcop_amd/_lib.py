"""ctypes binding of libstarcop_hip.so (the C ABI in include/starcop_hip.h).

This is the binding a maintainer of the reference would add.
There is NO fallback: if the shared library is missing, or the current device is
not gfx950, every call raises.  Nothing here imports ``oracle``.
"""
import ctypes as C
import os
import subprocess

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libstarcop_hip.so")
CSRC = os.path.join(_HERE, "csrc")

SC_CST = 8
STAT_CONV3, STAT_CONV1, STAT_DW, STAT_STEM, STAT_BNBWD, STAT_CONV1K, STAT_PW3 = 0, 1, 2, 3, 4, 5, 6

SRC_RAW, SRC_AFFINE, SRC_BNBWD, SRC_NORM = 0, 1, 2, 3
ACT_NONE, ACT_RELU, ACT_RELU6 = 0, 1, 2


class StarcopHipError(RuntimeError):
    pass


class sc_src(C.Structure):
    _fields_ = [("x", C.c_void_p), ("aux", C.c_void_p), ("cst", C.c_void_p),
                ("C", C.c_int32), ("mode", C.c_int32), ("act", C.c_int32), ("up", C.c_int32)]


class sc_conv_args(C.Structure):
    _fields_ = [("src", sc_src * 2), ("nsrc", C.c_int32), ("wpk", C.c_void_p),
                ("N", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("Cout", C.c_int32),
                ("ks", C.c_int32), ("co_t", C.c_int32),
                ("out0", C.c_void_p), ("out1", C.c_void_p),
                ("csplit", C.c_int32), ("accum0", C.c_int32), ("accum1", C.c_int32),
                ("add0", C.c_void_p), ("add1", C.c_void_p), ("stats", C.c_void_p), ("terms", C.c_int32), ("down0", C.c_int32),
                ("absmax", C.c_void_p), ("xbound", C.c_void_p * 2), ("bnr", C.c_void_p)]


class sc_bn_tail(C.Structure):
    """producer-tail BatchNorm finalize (include/starcop_hip.h: sc_bn_tail)"""
    _fields_ = [("gamma", C.c_void_p), ("beta", C.c_void_p), ("running_mean", C.c_void_p), ("running_var", C.c_void_p),
                ("momentum", C.c_float), ("eps", C.c_float), ("cst", C.c_void_p), ("act_bound", C.c_void_p), ("tickets", C.c_void_p)]


class sc_bnr_args(C.Structure):
    """BatchNorm-backward sums left by a data-gradient launch (include/starcop_hip.h: sc_bnr_args)"""
    _fields_ = [("y", C.c_void_p), ("cst", C.c_void_p), ("act", C.c_int32), ("rows", C.c_void_p), ("absmax", C.c_void_p)]


class sc_wgrad_args(C.Structure):
    _fields_ = [("dy", sc_src), ("src", sc_src * 2), ("nsrc", C.c_int32),
                ("N", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("Cout", C.c_int32), ("Cin", C.c_int32), ("ks", C.c_int32),
                ("part", C.c_void_p), ("part_floats", C.c_size_t), ("dw", C.c_void_p), ("terms", C.c_int32),
                ("absmax", C.c_void_p), ("xbound", C.c_void_p * 2)]


class sc_irt_args(C.Structure):
    _fields_ = [("x", sc_src), ("w_expand", C.c_void_p), ("w_dw", C.c_void_p), ("cst_expand", C.c_void_p),
                ("N", C.c_int32), ("Cin", C.c_int32), ("hidden", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("stride", C.c_int32)]


class sc_irb_args(C.Structure):
    _fields_ = [("x", sc_src), ("wpk_expand", C.c_void_p), ("cst_expand", C.c_void_p), ("w_dw", C.c_void_p), ("cst_dw", C.c_void_p),
                ("wpk_project", C.c_void_p), ("cst_project", C.c_void_p), ("out", C.c_void_p), ("z_absmax", C.c_void_p),
                ("N", C.c_int32), ("Cin", C.c_int32), ("hidden", C.c_int32), ("Cout", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("stride", C.c_int32), ("residual", C.c_int32)]


class sc_wgrad_pending(C.Structure):
    _fields_ = [("part", C.c_void_p), ("dw", C.c_void_p), ("nparts", C.c_int32), ("taps", C.c_int32), ("Cout", C.c_int32),
                ("Cin", C.c_int32), ("CoP", C.c_int32), ("CiP", C.c_int32), ("total", C.c_uint64)]


class sc_mag1c_args(C.Structure):
    _fields_ = [("x", C.c_void_p), ("x_is_f64", C.c_int32), ("xoff", C.c_void_p),
                ("P", C.c_void_p), ("Ppad", C.c_void_p), ("poff", C.c_void_p), ("statmask", C.c_void_p),
                ("G", C.c_int32), ("S", C.c_int32), ("npix", C.c_int64),
                ("templ", C.c_void_p), ("num_iter", C.c_int32), ("alpha", C.c_double),
                ("cov_update_scaling", C.c_double),
                ("albedo_override", C.c_int32), ("zero_override", C.c_int32),
                ("sparse_override", C.c_int32), ("apply_scaling", C.c_int32),
                ("work", C.c_void_p), ("mf_out", C.c_void_p), ("albedo_out", C.c_void_p),
                ("status", C.c_void_p), ("energy", C.c_void_p), ("logdet", C.c_void_p),
                ("cube", C.c_void_p), ("S_total", C.c_int32), ("band0", C.c_int32), ("pix_index", C.c_void_p),
                ("scatter_mf", C.c_void_p), ("scatter_alb", C.c_void_p), ("scatter_is_f64", C.c_int32)]


# enum sc_mag1c_launch (include/starcop_hip.h): what sc_mag1c_variant answers
MAG1C_TILE4, MAG1C_TILE4_SHRINK, MAG1C_TILE4_ENERGY, MAG1C_TILE4_ENERGY_SHRINK = 1100, 1101, 1110, 1111
MAG1C_TILE8_ENERGY, MAG1C_TILE8_ENERGY_SHRINK, MAG1C_TILE8_PAIR, MAG1C_TILE8_PAIR_SHRINK = 1210, 1211, 1220, 1221
MAG1C_TILE8_DIRECT, MAG1C_TILE8_DIRECT_SHRINK = 1230, 1231
MAG1C_F64_FAST, MAG1C_F64_512, MAG1C_F64_512_ENERGY, MAG1C_F64_1024, MAG1C_F64_1024_ENERGY = 2000, 2100, 2110, 2200, 2210
MAG1C_LAUNCHES = {          # the enumerators by name (without the SC_MAG1C_ prefix)
    "TILE4": MAG1C_TILE4, "TILE4_SHRINK": MAG1C_TILE4_SHRINK, "TILE4_ENERGY": MAG1C_TILE4_ENERGY,
    "TILE4_ENERGY_SHRINK": MAG1C_TILE4_ENERGY_SHRINK, "TILE8_ENERGY": MAG1C_TILE8_ENERGY,
    "TILE8_ENERGY_SHRINK": MAG1C_TILE8_ENERGY_SHRINK, "TILE8_PAIR": MAG1C_TILE8_PAIR, "TILE8_PAIR_SHRINK": MAG1C_TILE8_PAIR_SHRINK,
    "TILE8_DIRECT": MAG1C_TILE8_DIRECT, "TILE8_DIRECT_SHRINK": MAG1C_TILE8_DIRECT_SHRINK, "F64_FAST": MAG1C_F64_FAST,
    "F64_512": MAG1C_F64_512, "F64_512_ENERGY": MAG1C_F64_512_ENERGY, "F64_1024": MAG1C_F64_1024,
    "F64_1024_ENERGY": MAG1C_F64_1024_ENERGY}


class sc_mlr_args(C.Structure):
    """multiple-linear-regression ratio operands (include/starcop_hip.h: sc_mlr_args)"""
    _fields_ = [("base", C.c_void_p), ("band_off", C.c_longlong * 16), ("k", C.c_int32), ("tile_stride", C.c_longlong),
                ("target", C.c_void_p), ("target_tile_stride", C.c_longlong), ("B", C.c_int32), ("n", C.c_size_t)]


MLR_C_MATCHED, MLR_SIMPLE_PLUS, MLR_RESIDUAL = 0, 1, 2


class sc_srf_args(C.Structure):
    """spectral-response-function band simulation operands (include/starcop_hip.h: sc_srf_args)"""
    _fields_ = [("x", C.c_void_p), ("line_stride", C.c_int64), ("sample_stride", C.c_int64), ("band_stride", C.c_int64),
                ("L", C.c_int32), ("S", C.c_int32), ("B", C.c_int32), ("n_out", C.c_int32),
                ("ptr", C.c_void_p), ("band", C.c_void_p), ("w", C.c_void_p), ("ptr_host", C.c_void_p), ("band_host", C.c_void_p),
                ("out", C.c_void_p), ("out_plane_stride", C.c_int64), ("out_line_stride", C.c_int64),
                ("has_fill", C.c_int32), ("fill", C.c_float)]


class sc_resize_axis(C.Structure):
    """tap tables of one axis of the anti-aliased resize (include/starcop_hip.h: sc_resize_axis)"""
    _fields_ = [("n", C.c_int32), ("o", C.c_int32), ("n_tables", C.c_int32), ("T", C.c_int32),
                ("start", C.c_void_p), ("taps", C.c_void_p), ("w", C.c_void_p), ("wc", C.c_void_p),
                ("start_host", C.c_void_p), ("taps_host", C.c_void_p)]


class sc_resize_args(C.Structure):
    """anti-aliased resize operands (include/starcop_hip.h: sc_resize_args)"""
    _fields_ = [("x", C.c_void_p), ("plane_stride", C.c_int64), ("line_stride", C.c_int64), ("sample_stride", C.c_int64),
                ("P", C.c_int32), ("cval", C.c_float),
                ("out", C.c_void_p), ("out_plane_stride", C.c_int64), ("out_line_stride", C.c_int64),
                ("y", sc_resize_axis), ("xs", sc_resize_axis),
                ("table_y", C.c_void_p), ("table_x", C.c_void_p), ("table_y_host", C.c_void_p), ("table_x_host", C.c_void_p),
                ("work", C.c_void_p), ("work_bytes", C.c_size_t)]


class sc_winstats_args(C.Structure):
    """window-statistics operands (include/starcop_hip.h: sc_winstats_args)"""
    _fields_ = [("x", C.c_void_p), ("row_stride", C.c_int64), ("H", C.c_int32), ("W", C.c_int32),
                ("has_fill", C.c_int32), ("fill", C.c_float), ("clip_max", C.c_float), ("n_win", C.c_int32),
                ("windows", C.c_void_p), ("windows_host", C.c_void_p),
                ("count", C.c_void_p), ("sum_mean", C.c_void_p), ("stats", C.c_void_p)]


ORTHO_MAX_PLANES = 64


class sc_ortho_args(C.Structure):
    """GLT orthorectification operands (include/starcop_hip.h: sc_ortho_args)"""
    _fields_ = [("glt_x", C.c_void_p), ("glt_y", C.c_void_p), ("out_h", C.c_int32), ("out_w", C.c_int32),
                ("rows", C.c_int32), ("cols", C.c_int32), ("P", C.c_int32), ("elem_bytes", C.c_int32),
                ("absolute", C.c_int32), ("reserved", C.c_int32),
                ("src", C.c_void_p * ORTHO_MAX_PLANES), ("row_stride", C.c_int64 * ORTHO_MAX_PLANES),
                ("col_stride", C.c_int64 * ORTHO_MAX_PLANES), ("plane_rows", C.c_int32 * ORTHO_MAX_PLANES),
                ("plane_cols", C.c_int32 * ORTHO_MAX_PLANES), ("fill_bits", C.c_uint64 * ORTHO_MAX_PLANES),
                ("out", C.c_void_p), ("oob_count", C.c_void_p)]


WARP_MAX_PLANES = 32
WARP_NEAREST, WARP_BILINEAR, WARP_UNBOUNDED = 0, 1, 1


class sc_warp_args(C.Structure):
    """reprojection operands (include/starcop_hip.h: sc_warp_args)"""
    _fields_ = [("dst_gt", C.c_double * 6), ("src_inv", C.c_double * 6), ("dst_crs", C.c_int32), ("src_crs", C.c_int32),
                ("out_h", C.c_int32), ("out_w", C.c_int32), ("src_h", C.c_int32), ("src_w", C.c_int32), ("P", C.c_int32),
                ("elem_bytes", C.c_int32), ("resampling", C.c_int32), ("flags", C.c_int32),
                ("src", C.c_void_p * WARP_MAX_PLANES), ("row_stride", C.c_int64 * WARP_MAX_PLANES),
                ("col_stride", C.c_int64 * WARP_MAX_PLANES), ("nodata_bits", C.c_uint64 * WARP_MAX_PLANES),
                ("out", C.c_void_p), ("coords", C.c_void_p), ("oob_count", C.c_void_p)]


WARP_AREA_AVERAGE, WARP_AREA_MAX, WARP_AREA_MIN, WARP_AREA_MODE = 2, 3, 4, 5
WARP_AREA_THREAD, WARP_AREA_LANES = 1, 2


class sc_warp_area_args(C.Structure):
    """footprint resampling operands (include/starcop_hip.h: sc_warp_area_args)"""
    _fields_ = [("dst_gt", C.c_double * 6), ("src_inv", C.c_double * 6), ("dst_crs", C.c_int32), ("src_crs", C.c_int32),
                ("out_h", C.c_int32), ("out_w", C.c_int32), ("src_h", C.c_int32), ("src_w", C.c_int32), ("P", C.c_int32),
                ("elem_bytes", C.c_int32), ("mode", C.c_int32), ("variant", C.c_int32), ("min_coverage", C.c_double),
                ("src", C.c_void_p * WARP_MAX_PLANES), ("row_stride", C.c_int64 * WARP_MAX_PLANES),
                ("col_stride", C.c_int64 * WARP_MAX_PLANES), ("nodata_bits", C.c_uint64 * WARP_MAX_PLANES),
                ("out", C.c_void_p), ("coverage", C.c_void_p), ("boxes", C.c_void_p)]


MOSAIC_MAX_SOURCES, MOSAIC_MEAN_PLANES = 64, 4
MOSAIC_FIRST, MOSAIC_LAST, MOSAIC_MAX, MOSAIC_MIN, MOSAIC_MEAN, MOSAIC_BY_INDEX = range(6)
MOSAIC_KEY_FLOAT = 1


class sc_mosaic_source(C.Structure):
    """one source of a mosaic (include/starcop_hip.h: sc_mosaic_source)"""
    _fields_ = [("src_inv", C.c_double * 6), ("src_crs", C.c_int32), ("src_h", C.c_int32), ("src_w", C.c_int32),
                ("reserved", C.c_int32), ("box", C.c_int32 * 4), ("src", C.c_void_p * WARP_MAX_PLANES),
                ("row_stride", C.c_int64 * WARP_MAX_PLANES), ("col_stride", C.c_int64 * WARP_MAX_PLANES)]


class sc_mosaic_args(C.Structure):
    """mosaic operands (include/starcop_hip.h: sc_mosaic_args)"""
    _fields_ = [("dst_gt", C.c_double * 6), ("dst_crs", C.c_int32), ("out_h", C.c_int32), ("out_w", C.c_int32), ("N", C.c_int32),
                ("P", C.c_int32), ("elem_bytes", C.c_int32), ("rule", C.c_int32), ("key_plane", C.c_int32),
                ("resampling", C.c_int32), ("flags", C.c_int32), ("nodata_bits", C.c_uint64 * WARP_MAX_PLANES),
                ("sources", C.POINTER(sc_mosaic_source)), ("table", C.c_void_p), ("out", C.c_void_p), ("index", C.c_void_p),
                ("count", C.c_void_p), ("select", C.c_void_p)]


WCUT_MAX_PLANES = 64
WCUT_FILL, WCUT_SCALE, WCUT_CLIP = 1, 2, 4


class sc_wcut_args(C.Structure):
    """window-cut operands (include/starcop_hip.h: sc_wcut_args)"""
    _fields_ = [("scene_rows", C.c_int32), ("scene_cols", C.c_int32), ("out_h", C.c_int32), ("out_w", C.c_int32),
                ("P", C.c_int32), ("elem_bytes", C.c_int32), ("n_win", C.c_int32), ("reserved", C.c_int32),
                ("win_off", C.c_void_p), ("win_off_host", C.c_void_p),
                ("src", C.c_void_p * WCUT_MAX_PLANES), ("row_stride", C.c_int64 * WCUT_MAX_PLANES),
                ("col_stride", C.c_int64 * WCUT_MAX_PLANES), ("row0", C.c_int32 * WCUT_MAX_PLANES),
                ("col0", C.c_int32 * WCUT_MAX_PLANES), ("rows", C.c_int32 * WCUT_MAX_PLANES), ("cols", C.c_int32 * WCUT_MAX_PLANES),
                ("ops", C.c_uint32 * WCUT_MAX_PLANES), ("fill_bits", C.c_uint32 * WCUT_MAX_PLANES),
                ("scale", C.c_float * WCUT_MAX_PLANES), ("clip_lo", C.c_float * WCUT_MAX_PLANES),
                ("clip_hi", C.c_float * WCUT_MAX_PLANES), ("out", C.c_void_p)]


class sc_scene_win(C.Structure):
    """one window of a scene plan (include/starcop_hip.h: sc_scene_win)"""
    _fields_ = [("row_off", C.c_int32), ("col_off", C.c_int32), ("core_y0", C.c_int32), ("core_y1", C.c_int32),
                ("core_x0", C.c_int32), ("core_x1", C.c_int32), ("dst_row", C.c_int32), ("dst_col", C.c_int32)]


class sc_scene_args(C.Structure):
    """reflect-padded window gather operands (include/starcop_hip.h: sc_scene_args)"""
    _fields_ = [("src", C.c_void_p), ("elem_bytes", C.c_int32), ("C", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("chan_stride", C.c_int64), ("row_stride", C.c_int64), ("col_stride", C.c_int64),
                ("pad_top", C.c_int32), ("pad_left", C.c_int32), ("n", C.c_int32), ("win_h", C.c_int32), ("win_w", C.c_int32),
                ("scale", C.c_float), ("win", C.c_void_p), ("win_host", C.c_void_p), ("out", C.c_void_p)]


SCENE_MAX_PLANES = 16


class sc_scene_planes_args(C.Structure):
    """per-plane reflect-padded window gather operands (include/starcop_hip.h: sc_scene_planes_args)"""
    _fields_ = [("P", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("pad_top", C.c_int32), ("pad_left", C.c_int32),
                ("n", C.c_int32), ("win_h", C.c_int32), ("win_w", C.c_int32),
                ("src", C.c_void_p * SCENE_MAX_PLANES), ("row_stride", C.c_int64 * SCENE_MAX_PLANES),
                ("col_stride", C.c_int64 * SCENE_MAX_PLANES), ("ops", C.c_uint32 * SCENE_MAX_PLANES),
                ("fill_bits", C.c_uint32 * SCENE_MAX_PLANES), ("scale", C.c_float * SCENE_MAX_PLANES),
                ("clip_lo", C.c_float * SCENE_MAX_PLANES), ("clip_hi", C.c_float * SCENE_MAX_PLANES),
                ("win", C.c_void_p), ("win_host", C.c_void_p), ("out", C.c_void_p)]


PANEL_MAX, PANEL_MAX_CAT = 1024, 8
PANEL_F32, PANEL_I64, PANEL_U8 = 0, 1, 2                 # enum sc_panel_dtype
PANEL_BAND, PANEL_RGB, PANEL_CATEGORICAL = 0, 1, 2       # enum sc_panel_kind


class sc_panel(C.Structure):
    """one image panel of a validation figure (include/starcop_hip.h: sc_panel)"""
    _fields_ = [("src", C.c_void_p * 3), ("row_stride", C.c_int64), ("dtype", C.c_int32), ("kind", C.c_int32),
                ("H", C.c_int32), ("W", C.c_int32), ("scale", C.c_int32), ("dst_y", C.c_int32), ("dst_x", C.c_int32),
                ("autoscale", C.c_int32), ("n_cat", C.c_int32), ("reserved", C.c_int32),
                ("vmin", C.c_float), ("vmax", C.c_float), ("div", C.c_float),
                ("cat_value", C.c_float * PANEL_MAX_CAT), ("cat_rgb", (C.c_uint8 * 4) * PANEL_MAX_CAT)]


CSTATS_MAX_PLANES = 8


class sc_cstats_args(C.Structure):
    """per-component statistics operands (include/starcop_hip.h: sc_cstats_args)"""
    _fields_ = [("labels", C.c_void_p), ("counts", C.c_void_p),
                ("N", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("M", C.c_int32), ("P", C.c_int32), ("reserved", C.c_int32),
                ("plane", C.c_void_p * CSTATS_MAX_PLANES), ("plane_stride", C.c_int64 * CSTATS_MAX_PLANES),
                ("other", C.c_void_p), ("other_stride", C.c_int64),
                ("area", C.c_void_p), ("row_min", C.c_void_p), ("row_max", C.c_void_p), ("col_min", C.c_void_p),
                ("col_max", C.c_void_p), ("sum_row", C.c_void_p), ("sum_col", C.c_void_p), ("first_pixel", C.c_void_p),
                ("n_other", C.c_void_p), ("n_finite", C.c_void_p), ("sum", C.c_void_p), ("max", C.c_void_p), ("min", C.c_void_p),
                ("argmax", C.c_void_p)]


CRADIAL_MAX_BINS, CRADIAL_MAX_SIDE = 64, 32767


class sc_cradial_args(C.Structure):
    """per-component radial profile operands (include/starcop_hip.h: sc_cradial_args)"""
    _fields_ = [("labels", C.c_void_p), ("counts", C.c_void_p),
                ("N", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("M", C.c_int32), ("K", C.c_int32), ("reserved", C.c_int32),
                ("row_min", C.c_void_p), ("row_max", C.c_void_p), ("col_min", C.c_void_p), ("col_max", C.c_void_p),
                ("origin", C.c_void_p), ("plane", C.c_void_p), ("plane_stride", C.c_int64),
                ("edge2", C.c_int32 * CRADIAL_MAX_BINS),
                ("bin_count", C.c_void_p), ("bin_sum", C.c_void_p), ("d2_max", C.c_void_p), ("sum_rr", C.c_void_p),
                ("sum_cc", C.c_void_p), ("sum_rc", C.c_void_p)]


CQUANT_MAX_Q, CQUANT_SMALL_MAX = 8, 4096


class sc_cquant_args(C.Structure):
    """per-component order statistics operands (include/starcop_hip.h: sc_cquant_args)"""
    _fields_ = [("labels", C.c_void_p), ("counts", C.c_void_p),
                ("N", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("M", C.c_int32), ("Q", C.c_int32), ("reserved", C.c_int32),
                ("plane", C.c_void_p), ("plane_stride", C.c_int64), ("center", C.c_void_p),
                ("q", C.c_float * CQUANT_MAX_Q), ("n_finite", C.c_void_p), ("quantile", C.c_void_p)]


OUTLINE_COUNT, OUTLINE_TRACE,OUTLINE_RINGS, OUTLINE_SCATTER, OUTLINE_COMPACT = range(5)       # enum sc_outline_stage


class sc_outline_args(C.Structure):
    """component-outline operands (include/starcop_hip.h: sc_outline_args)"""
    _fields_ = [("labels", C.c_void_p), ("H", C.c_int32), ("W", C.c_int32), ("connectivity", C.c_int32), ("reserved", C.c_int32),
                ("E", C.c_int64), ("R", C.c_int64), ("V", C.c_int64), ("cnt", C.c_void_p), ("prefix", C.c_void_p),
                ("work", C.c_void_p), ("work_bytes", C.c_size_t), ("keys", C.c_void_p), ("stats", C.c_void_p),
                ("sorted_keys", C.c_void_p), ("ring_label", C.c_void_p), ("ring_area2", C.c_void_p), ("ring_len", C.c_void_p),
                ("ring_start", C.c_void_p), ("ordered", C.c_void_p), ("ordered_keep", C.c_void_p), ("keep_prefix", C.c_void_p),
                ("vertices", C.c_void_p), ("ring_offsets", C.c_void_p)]


class sc_rast_poly(C.Structure):
    """one polygon of a rasterize call (include/starcop_hip.h: sc_rast_poly)"""
    _fields_ = [("e0", C.c_int32), ("e1", C.c_int32), ("r0", C.c_int32), ("r1", C.c_int32), ("c0", C.c_int32), ("c1", C.c_int32),
                ("job0", C.c_int32), ("reserved", C.c_int32)]


class sc_rast_args(C.Structure):
    """polygon-rasterize operands (include/starcop_hip.h: sc_rast_args)"""
    _fields_ = [("edges", C.c_void_p), ("polys", C.c_void_p), ("polys_host", C.c_void_p), ("values", C.c_void_p), ("out", C.c_void_p),
                ("E", C.c_int64), ("P", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("reserved", C.c_int32)]


COG_MAX_BANDS = 4
COG_AVERAGE, COG_NEAREST, COG_MODE = 0, 1, 2             # enum sc_cog_resampling


class sc_cog_image(C.Structure):
    """a (nb, h, w) image read in place (include/starcop_hip.h: sc_cog_image)"""
    _fields_ = [("data", C.c_void_p), ("elem_bytes", C.c_int32), ("nb", C.c_int32), ("h", C.c_int32), ("w", C.c_int32),
                ("band_stride", C.c_int64), ("row_stride", C.c_int64), ("col_stride", C.c_int64),
                ("has_nodata", C.c_int32), ("nodata_bits", C.c_uint32)]


class sc_overview_args(C.Structure):
    """overview-pyramid operands (include/starcop_hip.h: sc_overview_args)"""
    _fields_ = [("src", sc_cog_image), ("resampling", C.c_int32), ("levels", C.c_int32), ("dst", C.c_void_p * 3)]


class sc_tiff_pack_args(C.Structure):
    """TIFF tile-packing operands (include/starcop_hip.h: sc_tiff_pack_args)"""
    _fields_ = [("src", sc_cog_image), ("bs", C.c_int32), ("predictor", C.c_int32), ("n_slots", C.c_int32), ("reserved", C.c_int32),
                ("slots", C.c_void_p), ("slots_host", C.c_void_p), ("out", C.c_void_p), ("out_bytes", C.c_size_t)]


EDT_FAR, EDT_WINDOW_MAX_R = 0x7FFFFFFF, 64               # SC_EDT_FAR, SC_EDT_WINDOW_MAX_R
EDT_WINDOW, EDT_ENVELOPE = 1, 2                          # enum sc_edt_row_pass


class sc_edt_args(C.Structure):
    """distance-transform operands (include/starcop_hip.h: sc_edt_args)"""
    _fields_ = [("mask", C.c_void_p), ("stride_n", C.c_int64), ("stride_h", C.c_int64), ("stride_w", C.c_int64),
                ("N", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("invert", C.c_int32),
                ("max_dist2", C.c_int32), ("thresh2", C.c_int32), ("variant", C.c_int32), ("negate", C.c_int32),
                ("pixel_size", C.c_double), ("dist2", C.c_void_p), ("dist", C.c_void_p), ("within", C.c_void_p)]


EDT_NEAREST_MAX_PLANES = 8                               # SC_EDT_NEAREST_MAX_PLANES


class sc_edt_nearest_args(C.Structure):
    """feature-transform operands (include/starcop_hip.h: sc_edt_nearest_args)"""
    _fields_ = [("mask", C.c_void_p), ("stride_n", C.c_int64), ("stride_h", C.c_int64), ("stride_w", C.c_int64),
                ("N", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("invert", C.c_int32),
                ("max_dist2", C.c_int32), ("variant", C.c_int32), ("n_planes", C.c_int32), ("reserved", C.c_int32),
                ("index", C.c_void_p), ("dist2", C.c_void_p), ("src", C.c_void_p * EDT_NEAREST_MAX_PLANES),
                ("src_stride", C.c_int64 * EDT_NEAREST_MAX_PLANES), ("dst", C.c_void_p * EDT_NEAREST_MAX_PLANES)]


_vp, _i, _f, _d, _sz =C.c_void_p, C.c_int, C.c_float, C.c_double, C.c_size_t

# name -> (restype, argtypes); every symbol include/starcop_hip.h declares
SIGNATURES = {
    "sc_last_error": (C.c_char_p, []),
    "sc_version": (_i, []),
    "sc_device_check": (_i, []),
    "sc_pack_weights": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "sc_packed_weight_floats": (_sz, [_i, _i, _i, _i, _i]),
    "sc_pack_work_items": (_sz, [_i, _i, _i, _i, _i, _i]),
    "sc_pack_weights_batch": (_i, [_vp, _vp, _i, C.c_uint32, _vp]),
    "sc_conv2d_mfma": (_i, [C.POINTER(sc_conv_args), _vp]),
    "sc_pw_stream_variant": (_i, [C.POINTER(sc_conv_args)]),
    "sc_conv1x1_ksplit": (_i, [C.POINTER(sc_conv_args), _vp]),
    "sc_wgrad_bx3_workspace_floats": (_sz, [_i, _i, _i, _i, _i]),
    "sc_conv3x3_wgrad_bx3": (_i, [C.POINTER(sc_wgrad_args), _vp]),
    "sc_pack_weights_bx3": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "sc_packed_weight_floats_bx3": (_sz, [_i, _i, _i, _i, _i]),
    "sc_conv3x3_bx3": (_i, [C.POINTER(sc_conv_args), _vp]),
    "sc_conv3_variant": (_i, [C.POINTER(sc_conv_args)]),
    "sc_thin16_variant": (_i, [C.POINTER(sc_conv_args)]),
    "sc_wgrad3_variant": (_i, [C.POINTER(sc_wgrad_args)]),
    "sc_wgrad_thin16_variant": (_i, [C.POINTER(sc_wgrad_args)]),
    "sc_wgrad_workspace_floats": (_sz, [_i, _i, _i, _i, _i, _i]),
    "sc_conv2d_wgrad_mfma": (_i, [C.POINTER(sc_wgrad_args), _vp]),
    "sc_dwconv3x3_fwd": (_i, [C.POINTER(sc_src), _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "sc_dwconv3x3_fwd_bn": (_i, [C.POINTER(sc_src), _vp, _vp, _i, _i, _i, _i, _i, _vp, C.POINTER(sc_bn_tail), _vp]),
    "sc_dwconv3x3_dgrad": (_i, [C.POINTER(sc_src), _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "sc_dwconv3x3_wgrad": (_i, [C.POINTER(sc_src), C.POINTER(sc_src), _vp, _i, _i, _i, _i, _i, _vp]),
    "sc_cast_f64_f32": (_i, [_vp, _vp, _sz, _vp]),
    "sc_cast_f64_f32_batch": (_i, [_vp, _i, _vp]),
    "sc_stem_conv_fwd": (_i, [C.POINTER(sc_src), _vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "sc_stem_fwd_kernel": (_i, [_i, _i, _i]),
    "sc_stem_wgrad_njb": (_i, [_i]),
    "sc_stem_wgrad_rows": (_i, [_i, _i, _i]),
    "sc_head_fwd_kernel": (_i, [_i, _i, _i, _i]),
    "sc_stem_wgrad_workspace_floats": (_sz, [_i, _i, _i, _i]),
    "sc_stem_conv_wgrad": (_i, [C.POINTER(sc_src), C.POINTER(sc_src), _vp, _sz, _vp, _i, _i, _i, _i, _vp]),
    "sc_head_conv_fwd": (_i, [C.POINTER(sc_src), _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "sc_head_conv_fwd_k": (_i, [C.POINTER(sc_src), _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "sc_head_conv_dgrad": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "sc_head_wgrad_workspace_floats": (_sz, [_i, _i, _i, _i]),
    "sc_head_conv_wgrad": (_i, [_vp, C.POINTER(sc_src), _vp, _sz, _vp, _vp, _i, _i, _i, _i, _vp]),
    "sc_head_conv_bwd": (_i, [_vp, C.POINTER(sc_src), _vp, _vp, _vp, _sz, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "sc_head_bwd_bn_rows": (_i, [_i, _i, _i]),
    "sc_stat_rows": (_i, [_i, _i, _i, _i]),
    "sc_bn_finalize": (_i, [_vp, _i, _d, _vp, _vp, _vp, _vp, _f, _f, _i, _vp, _i, _vp, _vp, _vp]),
    "sc_bn_finalize_form": (_i, [_i, _i, _i, _i]),
    "sc_bn_bwd_rows32_form": (_i, [_i, _i, _i]),
    "sc_ew_vec_form": (_i, [_i, _i]),
    "sc_bn_bwd_reduce": (_i, [_vp, _vp, _vp, _i, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "sc_bn_bwd_small": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sc_bn_bwd_finalize": (_i, [_vp, _i, _d, _vp, _vp, _vp, _vp, _i, _vp]),
    "sc_bn_bwd_finalize_rows32": (_i, [_vp, _i, _d, _vp, _vp, _vp, _vp, _i, _vp, _vp]),
    "sc_add_srcs": (_i, [C.POINTER(sc_src), C.POINTER(sc_src), _vp, _i, _i, _i, _vp]),
    "sc_stream_wait_stream": (_i, [_vp, _vp]),
    "sc_add_srcs_absmax": (_i, [C.POINTER(sc_src), C.POINTER(sc_src), _vp, _i, _i, _i, _vp, _vp]),
    "sc_apply_src": (_i, [C.POINTER(sc_src), _vp, _i, _i, _i, _vp]),
    "sc_downsum2x2": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "sc_fill_f64": (_i, [_vp, _d, _sz, _vp]),
    "sc_bce_logits_weighted": (_i, [_vp, _vp, _vp, _f, _sz, _vp, _vp, _vp, _vp]),
    "sc_adam_step": (_i, [_vp, _vp, _vp, _vp, _sz, _f, _f, _f, _f, _f, _f, _f, _f, _vp, _vp]),
    "sc_adam_prepare": (_i, [_vp, _vp, _f, _f, _vp, _vp]),
    "sc_threshold_masks": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _i, _i, _vp]),
    "sc_pred_classification": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "sc_mag1c_workspace_doubles": (_sz, [_i, _i, C.c_int64]),
    "sc_mag1c_groups": (_i, [C.POINTER(sc_mag1c_args), _vp]),
    "sc_mag1c_variant": (_i, [_i, _i, _i, _i, _i]),
    "sc_mag1c_pack": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp]),
    "sc_valid_mask": (_i, [_vp, _i, _i, _i, _i, _d, C.c_int64, _vp, _vp]),
    "sc_scatter": (_i, [_vp, _i, _vp, _sz, _vp, _i, _vp]),
    "sc_scatter_n": (_i, [_vp, _i, _vp, _vp, _sz, _vp, _i, _vp]),
    "sc_valid_mask_ne": (_i, [_vp, _i, _i, _i, _i, _d, C.c_int64, _vp, _vp]),
    "sc_mag1c_layout_columns": (_i, [_vp, _i, _i, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sc_mag1c_layout_ids_workspace_ints": (_sz, [C.c_int64, _i]),
    "sc_mag1c_layout_ids": (_i, [_vp, _vp, C.c_int64, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sc_trimmed_sum_workspace_bytes": (_sz, [_i]),
    "sc_trimmed_sums": (_i, [_vp, _i, _sz, _d, _vp, _vp, _sz, _vp]),
    "sc_band_ratio": (_i, [_vp, _vp, _vp, _i, _sz, _vp, _vp, _f, _f, _vp]),
    "sc_clip_scale": (_i, [_vp, _vp, _sz, _f, _f, _f, _f, _i, _vp]),
    "sc_mlr_workspace_bytes": (_sz, [_i, _sz, _i]),
    "sc_mlr_moments": (_i, [C.POINTER(sc_mlr_args), _vp, _sz, _vp]),
    "sc_mlr_solve": (_i, [C.POINTER(sc_mlr_args), _vp, _vp, _sz, _vp]),
    "sc_mlr_fit": (_i, [C.POINTER(sc_mlr_args), _vp, _vp, _sz, _vp]),
    "sc_mlr_predict": (_i, [C.POINTER(sc_mlr_args), _vp, _vp, _vp]),
    "sc_mlr_ratio": (_i, [C.POINTER(sc_mlr_args), _vp, _vp, _i, _i, _vp, _vp, _sz, _vp]),
    "sc_label_workspace_bytes": (_sz, [_i, _i, _i]),
    "sc_srf_bands": (_i, [C.POINTER(sc_srf_args), _vp]),
    "sc_resize_workspace_bytes": (_sz, [_i, _i, _i]),
    "sc_resize_aa": (_i, [C.POINTER(sc_resize_args), _vp]),
    "sc_window_stats_workspace_bytes": (_sz, [_i]),
    "sc_window_stats": (_i, [C.POINTER(sc_winstats_args), _vp, _sz, _vp]),
    "sc_glt_ortho": (_i, [C.POINTER(sc_ortho_args), _vp]),
    "sc_warp": (_i, [C.POINTER(sc_warp_args), _vp]),
    "sc_warp_area": (_i, [C.POINTER(sc_warp_area_args), _vp]),
    "sc_warp_area_variant": (_i, [C.POINTER(sc_warp_area_args)]),
    "sc_mosaic": (_i, [C.POINTER(sc_mosaic_args), _vp]),
    "sc_window_cut": (_i, [C.POINTER(sc_wcut_args), _vp]),
    "sc_scene_gather": (_i, [C.POINTER(sc_scene_args), _vp]),
    "sc_head_conv_fwd_k_mosaic": (_i, [C.POINTER(sc_src), _vp, _vp, _vp, _i, _i, C.c_int64, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "sc_scene_gather_planes": (_i, [C.POINTER(sc_scene_planes_args), _vp]),
    "sc_scene_core_counts": (_i, [_vp, C.c_int64, C.c_int64, _i, _i, C.c_uint32, _vp, _vp, _i, _vp, _vp]),
    "sc_head_conv_fwd_mosaic_prob": (_i, [C.POINTER(sc_src), _vp, _vp, _vp, C.c_int64, _vp, C.c_int64, _i, _i, _vp, C.c_int64, C.c_int64,
                                          C.c_uint32, _f, _vp, _vp, _i, _i, _i, _i, _vp]),
    "sc_connected_components": (_i, [_vp, _i, _vp, _vp, _vp, _sz, _i, _i, _i, _vp]),
    "sc_proposed_mask": (_i, [_vp, C.c_int64, _vp, C.c_int64, _f, _i, _vp, _vp, _sz, _i, _i, _i, _vp]),
    "sc_packed_weight_floats_thin16": (_sz, [_i, _i, _i]),
    "sc_pack_weights_thin16": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "sc_conv3x3_thin16": (_i, [C.POINTER(sc_conv_args), _vp]),
    "sc_packed_weight_floats_sp": (_sz, [_i, _i, _i]),
    "sc_pack_weights_sp": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "sc_sp_stat_rows": (_i, [_i, _i, _i, _i]),
    "sc_conv3x3_sp": (_i, [C.POINTER(sc_conv_args), _vp]),
    "sc_packed_weight_floats_spd": (_sz, [_i, _i, _i]),
    "sc_pack_weights_spd": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "sc_spd_vskip_ok": (_i, [_i, _i]),
    "sc_conv3x3_sp_dgrad": (_i, [C.POINTER(sc_conv_args), _vp]),
    "sc_sp_wgrad_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "sc_conv3x3_sp_wgrad": (_i, [C.POINTER(sc_wgrad_args), _vp, _sz, _vp]),
    "sc_wgrad_scatter_cols": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "sc_sp_variant": (_i, [C.POINTER(sc_conv_args)]),
    "sc_spd_variant": (_i, [C.POINTER(sc_conv_args)]),
    "sc_sp_wgrad_variant": (_i, [C.POINTER(sc_wgrad_args)]),
    "sc_binary_opening": (_i, [_vp, _f, _i, _vp, _vp, _i, _i, _i, _vp]),
    "sc_threshold_confusion": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _i, _i, _i, _vp]),
    "sc_gather_augment": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "sc_tile_window_sums": (_i, [_vp, _i, _i, _i, _vp, _vp, _i, _vp, _vp]),
    "sc_dwconv3x3_bwd_fused": (_i, [C.POINTER(sc_src), C.POINTER(sc_src), _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "sc_dw_variant": (_i, [_i, _i, _i, _i, _i, _i, _i]),
    "sc_wgrad_thin16_workspace_floats": (_sz, [_i, _i, _i, _i, _i]),
    "sc_conv3x3_wgrad_thin16": (_i, [C.POINTER(sc_wgrad_args), _vp]),
    "sc_conv2d_wgrad_mfma_deferred": (_i, [C.POINTER(sc_wgrad_args), C.POINTER(sc_wgrad_pending), _vp]),
    "sc_wgrad_reduce_batch": (_i, [_vp, _vp, _i, C.c_uint32, _vp]),
    "sc_packed_weight_floats_pw3": (_sz, [_i, _i, _i]),
    "sc_conv1x1_pw3": (_i, [C.POINTER(sc_conv_args), _vp]),
    "sc_conv1x1_pw3_variant": (_i, [_i, _i, _i, _i]),
    "sc_wgrad_pw3_workspace_floats": (_sz, [_i, _i, _i, _i, _i]),
    "sc_wgrad_pw3_variant": (_i, [_i, _i, _i, _i, _i]),
    "sc_conv1x1_wgrad_pw3": (_i, [C.POINTER(sc_wgrad_args), C.POINTER(sc_wgrad_pending), _vp]),
    "sc_irb_supported": (_i, [_i, _i, _i, _i, _i, _i]),
    "sc_irb_variant": (_i, [_i, _i, _i, _i]),
    "sc_irb_eval": (_i, [C.POINTER(sc_irb_args), _vp]),
    "sc_irt_supported": (_i, [_i, _i, _i, _i, _i]),
    "sc_irt_rows": (_i, [_i, _i, _i, _i, _i]),
    "sc_irt_bwd_rows": (_i, [_i, _i, _i, _i]),
    "sc_irt_bwd_workspace_floats": (_sz, [_i, _i, _i, _i, _i]),
    "sc_irt_geometry": (_i, [_i, _i, _i, _i, _i, _i, C.POINTER(_i)]),
    "sc_irt_expand_stats": (_i, [C.POINTER(sc_irt_args), _vp, _vp]),
    "sc_irt_fwd": (_i, [C.POINTER(sc_irt_args), _vp, _vp, _vp]),
    "sc_irt_bwd": (_i, [C.POINTER(sc_irt_args), C.POINTER(sc_src), _vp, _vp, _vp, _vp]),
    "sc_irt_xmoments": (_i, [C.POINTER(sc_irt_args), _vp, _vp]),
    "sc_irt_bwd_fix": (_i, [C.POINTER(sc_irt_args), _vp, _vp, _vp, _vp, _i, _vp]),
    "sc_irt_wgrad_finalize": (_i, [C.POINTER(sc_irt_args), _vp, _vp, _vp, _vp]),
    "sc_maxpool2x2": (_i, [C.POINTER(sc_src), _vp, _i, _i, _i, _i, _vp]),
    "sc_upsample_bilinear2x": (_i, [C.POINTER(sc_src), _vp, _i, _i, _i, _i, _vp]),
    "sc_maxpool2x2_bwd": (_i, [C.POINTER(sc_src), _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "sc_upsample_bilinear2x_bwd": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "sc_pwreg_param_floats": (_sz, [_i, _i, _i, _i]),
    "sc_pwreg_fwd": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "sc_reg_loss": (_i, [_vp, _vp, _sz, _i, _vp, _vp, _vp, _vp]),
    "sc_pwreg_sweep_blocks": (_i, [_i, _i, _i]),
    "sc_pwreg_train_sweep": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "sc_pwreg_finalize": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _d, _vp, _vp, _vp]),
    "sc_panel_minmax": (_i, [_vp, C.POINTER(sc_panel), _i, _vp, _vp]),
    "sc_render_panels": (_i, [_vp, C.POINTER(sc_panel), _i, _vp, _vp, _i, _i, _vp]),
    "sc_component_stats_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "sc_component_stats": (_i, [C.POINTER(sc_cstats_args), _vp, _sz, _vp]),
    "sc_component_radial_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "sc_component_radial": (_i, [C.POINTER(sc_cradial_args), _vp, _sz, _vp]),
    "sc_component_quantiles_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "sc_component_quantiles": (_i, [C.POINTER(sc_cquant_args), _vp, _sz, _vp]),
    "sc_component_outlines_workspace_bytes": (_sz, [_i, _i, C.c_int64]),
    "sc_component_outlines_rounds": (_i, [C.c_int64]),
    "sc_component_outlines": (_i, [C.POINTER(sc_outline_args), _i, _vp]),
    "sc_rasterize_polygons": (_i, [C.POINTER(sc_rast_args), _vp]),
    "sc_overview_reduce": (_i, [C.POINTER(sc_overview_args), _vp]),
    "sc_tiff_tile_flags": (_i, [C.POINTER(sc_cog_image), _i, _vp, _vp]),
    "sc_tiff_pack_tiles": (_i, [C.POINTER(sc_tiff_pack_args), _vp]),
    "sc_edt_workspace_bytes": (_sz, [_i, _i, _i]),
    "sc_edt": (_i, [C.POINTER(sc_edt_args), _vp, _sz, _vp]),
    "sc_edt_call_workspace_bytes": (_sz, [C.POINTER(sc_edt_args)]),
    "sc_edt_variant": (_i, [_i, _i, _i, _i]),
    "sc_edt_nearest_workspace_bytes": (_sz, [_i, _i, _i]),
    "sc_edt_nearest_call_workspace_bytes": (_sz, [C.POINTER(sc_edt_nearest_args)]),
    "sc_edt_nearest": (_i, [C.POINTER(sc_edt_nearest_args), _vp, _sz, _vp]),
    "sc_label_keep": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "sc_tiff_lzw_decode": (_i, [_vp, _sz, _vp, _sz, C.POINTER(C.c_size_t)]),
    "sc_tiff_unpredict": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp]),
}
REG_L1, REG_MSE, PWREG_G_FROM_MEMORY = 0, 1, 2       # enum sc_reg_loss_kind
PWREG_MAXC, PWREG_PART_DOUBLES, REG_LOSS_PARTS = 16, 273, 256
PACK_SPD = 8          # ... and of its data gradient sc_conv3x3_sp_dgrad
PACK_SP = 7            # sc_pack_desc.bx3 code of the phase-filter layout of sc_conv3x3_sp
PACK_PW3 = 6           # sc_pack_desc.bx3 code of the pointwise layout of sc_conv1x1_pw3
PACK_THIN16 = 5        # sc_pack_desc.bx3 code of the register layout of sc_conv3x3_thin16
TERMS_F16X2 = 4        # `terms` code of the two-fp16-term kernels (include/starcop_hip.h SC_TERMS_F16X2)
SE_CROSS = 0xBA        # the 3x3 cross of starcop/baselines.py:39-41 as sc_binary_opening's se_bits

_lib = None


def build(force=False):
    """Compile every HIP source for gfx950 into starcop_amd/libstarcop_hip.so (hipcc; no GPU needed)."""
    if force:
        subprocess.run(["make", "-C", CSRC, "clean"], check=True, stdout=subprocess.DEVNULL)
    r = subprocess.run(["make", "-C", CSRC, "-j", "4"], capture_output=True, text=True)
    if r.returncode != 0:
        raise StarcopHipError("building libstarcop_hip.so failed:\n" + r.stdout[-4000:] + r.stderr[-4000:])
    return LIB_PATH


def load():
    """dlopen the library and declare every entry point.  Raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("STARCOP_HIP_LIB", LIB_PATH)        # development knob: an experiment build of the same sources
    if not os.path.exists(path):
        raise StarcopHipError(
            f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C starcop_amd/csrc`).  starcop_amd has no CPU/torch fallback.")
    lib = C.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)     # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


_EXC = {-1: ValueError, -2: RuntimeError, -3: torch.linalg.LinAlgError, -4: RuntimeError}


def check(rc):
    """Map negative C status codes to the exception types the reference raises."""
    if rc != 0:
        msg = load().sc_last_error().decode("utf-8", "replace")
        raise _EXC.get(rc, StarcopHipError)(f"libstarcop_hip: {msg} (status {rc})")


_device_ok = {}


def require_device(t=None):
    """The product path runs on a gfx950 GPU only; anything else is a loud error."""
    if not torch.cuda.is_available():
        raise StarcopHipError("starcop_amd needs a ROCm GPU (gfx950); torch.cuda.is_available() is False")
    if t is not None and not t.is_cuda:
        raise StarcopHipError(f"starcop_amd kernels need device tensors, got a tensor on {t.device}")
    dev = torch.cuda.current_device()
    if dev not in _device_ok:
        check(load().sc_device_check())
        _device_ok[dev] = True


def tiff_lzw_decode(buf: bytes, n_out: int) -> bytes:
    """host: TIFF LZW stream -> at most n_out bytes (sc_tiff_lzw_decode)"""
    out = C.create_string_buffer(n_out)
    written = C.c_size_t(0)
    src = (C.c_char * len(buf)).from_buffer_copy(buf)
    if load().sc_tiff_lzw_decode(C.cast(src, C.c_void_p), len(buf), C.cast(out, C.c_void_p), n_out, C.byref(written)) != 0:
        raise ValueError("corrupt TIFF LZW stream")
    return out.raw[:written.value]


def tiff_unpredict(a, predictor, rows, cols, spp, bps, big_endian):
    """host: undo TIFF predictor 2 / 3 on a decoded block (uint8 numpy array) -> uint8 array of little-endian samples"""
    import numpy as np
    a = np.ascontiguousarray(a, dtype=np.uint8)
    out = np.empty_like(a)
    if load().sc_tiff_unpredict(a.ctypes.data_as(C.c_void_p), predictor, rows, cols, spp, bps, int(bool(big_endian)),
                                out.ctypes.data_as(C.c_void_p)) != 0:
        raise ValueError(f"TIFF predictor {predictor} with {bps}-byte samples is not supported")
    return out


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    """device pointer of a tensor (None -> NULL)."""
    if t is None:
        return None
    return C.c_void_p(t.data_ptr())


# out[] of sc_irt_geometry, in order (include/starcop_hip.h SC_IRT_GEO_FIELDS)
IRT_GEO_FIELDS = ("nks", "nch", "ngroups", "stats_grid", "pixel_blocks", "fwd_tiles", "fwd_per_cu", "fwd_grid", "bwd_tiles", "tiles_per_wg",
                  "bwd_rows", "mom_grid", "mom_ksteps", "fix_grid")


def irt_geometry(N, Cin, hidden, H, W, stride=2):
    """host: the launch geometry of the fused training block (sc_irt_geometry) as a dict; None for a block the library rejects"""
    out = (C.c_int * len(IRT_GEO_FIELDS))()
    if load().sc_irt_geometry(N, Cin, hidden, H, W, stride, out) != 0:
        return None
    return dict(zip(IRT_GEO_FIELDS, out))


def make_src(x, C_, mode=SRC_RAW, act=ACT_NONE, up=0, cst=None, aux=None):
    s = sc_src()
    s.x = x.data_ptr() if x is not None else None
    s.aux = aux.data_ptr() if aux is not None else None
    s.cst = cst.data_ptr() if cst is not None else None
    s.C, s.mode, s.act, s.up = int(C_), int(mode), int(act), int(up)
    return s
