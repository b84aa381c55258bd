"""ctypes binding of libstif_hip.so (the C ABI declared in include/stif.h).

The library is built in-tree (``make`` / ``__graft_entry__.build()``).  There is
no fallback: if the library is missing or fails to load, every op raises.
"""
from __future__ import annotations

import ctypes as C
import os

# STIF_HIP_LIB overrides the in-tree library (kernel experiments); the default is the in-tree build
LIB_PATH = os.environ.get("STIF_HIP_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libstif_hip.so")

MAXG = 16               # stif.h STIF_MAX_GROUPS: weight sets per launch
EPI_NONE, EPI_LRELU, EPI_RELU, EPI_RES, EPI_OFFMASK, EPI_LSTM = range(6)
PACK_PLAIN, PACK_OFFMASK, PACK_LSTM, PACK_WINO, PACK_WINO_OFFMASK, PACK_WINO_LSTM, PACK_DCNSEP, PACK_DCNPAIR = range(8)
PACK_F16X3 = 16          # OR'ed into a PACK_WINO* mode (stif.h STIF_PACK_F16X3)
CONV_F16X3 = 1           # stif_conv_args.flags
CONV_DYNAMIC = 2         # stif_conv_args.flags: dynamic tile schedule (sched counters)
DEC_REVOLUTIONS = 2      # stif_pack_dec_proj_ex lr_image bit (stif.h STIF_DEC_REVOLUTIONS)
PACK_DGRAD = 1           # stif_pack_conv_weight_dev flags: the data gradient's weight (stif.h STIF_PACK_DGRAD)
STATUS_PACK_RANGE = 16   # status bit of the device packer (stif.h STIF_STATUS_PACK_RANGE)

_P = C.c_void_p
_PA = _P * MAXG
_IB = C.c_int * (MAXG + 1)   # item_base: per-set item counts as a prefix array, all zeros = `nitems` per set


class ConvArgs(C.Structure):
    _fields_ = [
        ("in0", _PA), ("in1", _PA), ("w", _PA), ("bias", _PA), ("out", _PA), ("res", _PA), ("out2", _PA),
        ("in0_item", C.c_longlong), ("in1_item", C.c_longlong), ("out_item", C.c_longlong),
        ("res_item", C.c_longlong), ("out2_item", C.c_longlong),
        ("ngroups", C.c_int), ("nitems", C.c_int),
        ("H", C.c_int), ("W", C.c_int), ("C0", C.c_int),
        ("C1", C.c_int), ("in1_mode", C.c_int), ("in1_scale", C.c_float),
        ("Ho", C.c_int), ("Wo", C.c_int), ("cout", C.c_int), ("ks", C.c_int), ("stride", C.c_int),
        ("epi", C.c_int), ("flags", C.c_int), ("status", _P), ("sched", _P), ("item_base", _IB),
    ]


class DcnArgs(C.Structure):
    _fields_ = [
        ("inp", _PA), ("offmask", _PA), ("w", _PA), ("bias", _PA), ("out", _PA),
        ("in_item", C.c_longlong), ("om_item", C.c_longlong), ("out_item", C.c_longlong),
        ("ngroups", C.c_int), ("nitems", C.c_int), ("H", C.c_int), ("W", C.c_int), ("epi", C.c_int),
        ("flags", C.c_int), ("status", _P), ("item_base", _IB),
    ]


class DcnSepArgs(C.Structure):
    _fields_ = [
        ("fea", _PA), ("inp", _PA), ("w_om", _PA), ("b_om", _PA), ("w", _PA), ("bias", _PA), ("out", _PA),
        ("fea_item", C.c_longlong), ("in_item", C.c_longlong), ("out_item", C.c_longlong),
        ("ngroups", C.c_int), ("nitems", C.c_int), ("H", C.c_int), ("W", C.c_int), ("epi", C.c_int),
        ("flags", C.c_int), ("status", _P), ("item_base", _IB),
    ]


class ConvWgradArgs(C.Structure):
    """stif_conv_wgrad_args: x / gy NHWC maps with element strides between items, gw OIHW, gb or NULL."""
    _fields_ = [
        ("x", _P), ("gy", _P), ("gw", _P), ("gb", _P), ("x_item", C.c_longlong), ("gy_item", C.c_longlong),
        ("n", C.c_int), ("H", C.c_int), ("W", C.c_int), ("cin", C.c_int), ("cout", C.c_int),
        ("workspace", _P), ("workspace_bytes", C.c_size_t),
    ]


class ConvWgradCatArgs(C.Structure):
    """stif_conv_wgrad_cat_args: the weight gradient in 64 x 64 channel blocks -- one or two 64-channel x maps, gy with
    a pixel pitch of gy_channels floats of which the first cout count, gw [cout][64 nx][3][3]."""
    _fields_ = [
        ("x", _P * 2), ("gy", _P), ("gw", _P), ("gb", _P), ("x_item", C.c_longlong * 2), ("gy_item", C.c_longlong),
        ("n", C.c_int), ("H", C.c_int), ("W", C.c_int), ("nx", C.c_int), ("gy_channels", C.c_int), ("cout", C.c_int),
        ("workspace", _P), ("workspace_bytes", C.c_size_t),
    ]


class DcnBwdArgs(C.Structure):
    """stif_dcn_bwd_args: the backward of stif_dcn_nhwc -- NHWC maps with element strides between items, the OIHW weight
    as the state dict has it, any of g_in / g_om / g_w (with g_b) NULL for 'not computed'."""
    _fields_ = [
        ("inp", _P), ("offmask", _P), ("w", _P), ("gout", _P), ("out", _P),
        ("g_in", _P), ("g_om", _P), ("g_w", _P), ("g_b", _P),
        ("in_item", C.c_longlong), ("om_item", C.c_longlong), ("gout_item", C.c_longlong), ("out_item", C.c_longlong),
        ("gin_item", C.c_longlong), ("gom_item", C.c_longlong),
        ("n", C.c_int), ("H", C.c_int), ("W", C.c_int), ("epi", C.c_int),
        ("workspace", _P), ("workspace_bytes", C.c_size_t),
    ]


class DcnBwdContribArgs(C.Structure):
    """stif_dcn_bwd_contrib_args: stif_dcn_bwd_nhwc's data kernel with the g_in scatter stored as contribution
    sub-rows ``cm``, corner weights ``wgt`` and packed sort words ``words`` (g_om may be NULL)."""
    _fields_ = [
        ("inp", _P), ("offmask", _P), ("w", _P), ("gout", _P), ("out", _P), ("g_om", _P),
        ("cm", _P), ("wgt", _P), ("words", _P),
        ("in_item", C.c_longlong), ("om_item", C.c_longlong), ("gout_item", C.c_longlong), ("out_item", C.c_longlong),
        ("gom_item", C.c_longlong),
        ("n", C.c_int), ("H", C.c_int), ("W", C.c_int), ("epi", C.c_int),
    ]


class DecTables(C.Structure):
    _fields_ = [(n, _P) for n in ("near_y", "rel_y", "by0", "by1", "wy0", "wy1", "lin_y",
                                  "near_x", "rel_x", "bx0", "bx1", "wx0", "wx1", "lin_x", "hr_y", "hr_x")]


class DecImage(C.Structure):
    _fields_ = [("img", _P), ("ih", C.c_int), ("iw", C.c_int)] + [
        (n, _P) for n in ("by0", "by1", "wy0", "wy1", "bx0", "bx1", "wx0", "wx1")]


class DecWindow(C.Structure):
    """stif_dec_window: query rectangle, F rectangle (all zero = the query rectangle), stage-2 output
    addressing in elements (all zero = a dense [n, 3, hh, ww])."""
    _fields_ = [(n, C.c_int) for n in ("y0", "x0", "hh", "ww", "fy0", "fx0", "fh", "fw")] + [
        ("out_item", C.c_longlong), ("out_plane", C.c_longlong), ("out_pitch", C.c_int)]


class DecBlend(C.Structure):
    """stif_dec_blend: which of the local ensemble's four decodes a blending stage 2 is, whether it adds to the
    output or starts it, and the rel_y / rel_x tables of the four shifted queries its weight is computed from."""
    _fields_ = [("k", C.c_int), ("accumulate", C.c_int), ("rel_y", _P * 4), ("rel_x", _P * 4)]


class DecTimeField(C.Structure):
    """stif_dec_time: the query time of pixel (gy, gx) of item i is t[i * item + gy * row + gx * col] (strides in
    elements, >= 0, 0 broadcasts)."""
    _fields_ = [("t", _P), ("item", C.c_longlong), ("row", C.c_longlong), ("col", C.c_longlong)]


class DecPointList(C.Structure):
    """stif_dec_points: point p of item i is row y[i * y_item + p], column x[i * x_item + p] of the virtual grid at
    time t[i * t_item + p * t_point] (strides in elements, >= 0, 0 broadcasts); npts points per item."""
    _fields_ = [("y", _P), ("x", _P), ("t", _P), ("y_item", C.c_longlong), ("x_item", C.c_longlong),
                ("t_item", C.c_longlong), ("t_point", C.c_longlong), ("npts", C.c_int)]


SIREN_ROW_TILE = 64      # stif.h STIF_SIREN_ROW_TILE: rows per workgroup of the SIREN training kernels


class SirenArgs(C.Structure):
    """stif_siren_args: one SIREN MLP on a row-major input matrix, forward-for-training and backward."""
    _fields_ = [
        ("x", _P), ("x_stride", C.c_longlong),
        ("n", C.c_int), ("cin", C.c_int), ("nsine", C.c_int), ("cout", C.c_int), ("width", C.c_int * 4),
        ("w", _P * 5), ("b", _P * 5), ("y", _P), ("z", _P), ("g_y", _P), ("g_x", _P), ("gx_stride", C.c_longlong),
        ("g_w", _P * 5), ("g_b", _P * 5), ("workspace", _P), ("workspace_bytes", C.c_size_t),
    ]


DEC_TRAIN_TABLES = ("near_y", "near_x", "rel_y", "rel_x", "by0", "by1", "bx0", "bx1", "wy0", "wy1", "wx0", "wx1",
                    "lin_y", "lin_x", "near_y_first", "near_x_first", "by0_first", "by1_first", "bx0_first",
                    "bx1_first")


class DecTrainGeom(C.Structure):
    """stif_dec_train_geom: sizes, the LR maps and the per-axis tables of the decoder's input builders."""
    _fields_ = [(n, C.c_int) for n in ("B", "H", "W", "HH", "WW")] + [
        (n, _P) for n in ("feat", "frames", "t") + DEC_TRAIN_TABLES]


METRIC_Y, METRIC_SSIM, METRIC_FLOAT = 1, 2, 4  # stif_metric_args.flags (stif.h STIF_METRIC_*)
FSSIM_VOLUME, FSSIM_PLANAR = 0, 1               # stif_metric_float's mode (stif.h STIF_FSSIM_*)


class MetricArgs(C.Structure):
    """stif_metric_args: all-zero strides mean dense [n][3][H][W] planes / dense [n][H][W][3] bytes."""
    _fields_ = [
        ("pred", _P), ("pred_item", C.c_longlong), ("pred_plane", C.c_longlong), ("pred_pitch", C.c_longlong),
        ("gt_u8", _P), ("gt_item", C.c_longlong), ("gt_pitch", C.c_longlong),
        ("gt_f32", _P), ("gtf_item", C.c_longlong), ("gtf_plane", C.c_longlong), ("gtf_pitch", C.c_longlong),
        ("n", C.c_int), ("H", C.c_int), ("W", C.c_int), ("flags", C.c_int),
    ]


BATCH_HFLIP, BATCH_VFLIP, BATCH_ROT90 = 1, 2, 4   # stif_build_batch flags (stif.h STIF_BATCH_*)
GRAD_CHUNK, GRAD_MAX_SEGS = 1024, 1 << 20         # stif.h STIF_GRAD_CHUNK, STIF_GRAD_MAX_SEGS
RANK_SUM_MAX_RANKS = 64                           # stif.h STIF_RANK_SUM_MAX_RANKS
YUV_BT601, YUV_BT709 = 0, 1   # stif_yuv_format.matrix (stif.h STIF_YUV_*)


class YuvFormat(C.Structure):
    """stif_yuv_format: zero pitches / frame stride mean dense rows / the dense Y4M frame Y | U | V."""
    _fields_ = [(n, C.c_int) for n in ("width", "height", "sub_x", "sub_y", "depth", "matrix", "full_range")] + [
        ("pitch_y", C.c_longlong), ("pitch_c", C.c_longlong), ("frame_stride", C.c_longlong)]


EXPORTS = {
    # name: (restype, argtypes)
    "stif_yuv_to_rgb": (C.c_int, [C.POINTER(YuvFormat), _P, _P, _P, C.c_int, _P] + [C.c_longlong] * 3 + [_P]),
    "stif_rgb_to_yuv": (C.c_int, [C.POINTER(YuvFormat), _P] + [C.c_longlong] * 3 + [C.c_int, _P, _P, _P, _P]),
    "stif_scene_workspace_size": (C.c_size_t, [C.c_int] * 3),
    "stif_scene_sad": (C.c_int, [_P] + [C.c_longlong] * 3 + [C.c_int] * 3 + [_P, _P, C.c_size_t, _P]),
    "stif_metric_workspace_size": (C.c_size_t, [C.c_int] * 4),
    "stif_metric_psnr_ssim": (C.c_int, [C.POINTER(MetricArgs), _P, _P, C.c_size_t, _P]),
    "stif_metric_window": (C.c_int, [C.POINTER(C.c_double)]),
    "stif_metric_float_workspace_size": (C.c_size_t, [C.c_int] * 4),
    "stif_metric_float": (C.c_int, [C.POINTER(MetricArgs), C.c_int, _P, _P, C.c_size_t, _P]),
    "stif_conv2d_nhwc": (C.c_int, [C.POINTER(ConvArgs), _P]),
    "stif_conv3x3_wino": (C.c_int, [C.POINTER(ConvArgs), _P]),
    "stif_conv3x3_wgrad_workspace_size": (C.c_size_t, [C.c_int] * 5),
    "stif_conv3x3_wgrad": (C.c_int, [C.POINTER(ConvWgradArgs), _P]),
    "stif_pack_conv_weight_dev": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P]),
    "stif_conv3x3s2_wgrad_workspace_size": (C.c_size_t, [C.c_int] * 5),
    "stif_conv3x3s2_wgrad": (C.c_int, [C.POINTER(ConvWgradArgs), _P]),
    "stif_conv3x3s2_dgrad_workspace_size": (C.c_size_t, [C.c_int] * 3),
    "stif_conv3x3s2_dgrad": (C.c_int, [_P, _P, _P, C.c_longlong, C.c_longlong, C.c_int, C.c_int, C.c_int, _P,
                                       C.c_size_t, _P]),
    "stif_conv_first_wgrad_workspace_size": (C.c_size_t, [C.c_int] * 3),
    "stif_conv_first_wgrad": (C.c_int, [_P, _P, _P, _P, C.c_longlong, C.c_int, C.c_int, C.c_int, _P, C.c_size_t, _P]),
    "stif_pack_conv_plain_dev": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    "stif_conv3x3_wgrad_cat_workspace_size": (C.c_size_t, [C.c_int] * 6),
    "stif_conv3x3_wgrad_cat": (C.c_int, [C.POINTER(ConvWgradCatArgs), _P]),
    "stif_upsample2x_bwd_nhwc": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_longlong,
                                           C.c_longlong, _P]),
    "stif_pack_conv_block_dev": (C.c_int, [_P, _P] + [C.c_int] * 6 + [_P, _P, _P, _P]),
    "stif_conv1x1_wgrad_workspace_size": (C.c_size_t, [C.c_int] * 4),
    "stif_conv1x1_wgrad": (C.c_int, [C.POINTER(ConvWgradCatArgs), _P]),
    "stif_pack_conv1x1_dev": (C.c_int, [_P, _P] + [C.c_int] * 5 + [_P, _P, _P, _P]),
    "stif_lstm_gates_nhwc": (C.c_int, [_P] * 4 + [C.c_int] * 3 + [C.c_longlong] * 4 + [_P]),
    "stif_lstm_gates_bwd_nhwc": (C.c_int, [_P] * 6 + [C.c_int] * 3 + [C.c_longlong] * 6 + [_P]),
    "stif_upsample2x_nhwc": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_longlong,
                                       C.c_longlong, _P]),
    "stif_siren_fwd": (C.c_int, [C.POINTER(SirenArgs), _P]),
    "stif_siren_bwd_workspace_size": (C.c_size_t, [C.c_int] * 2),
    "stif_siren_wgrad_grid": (C.c_int, [C.c_int] * 3),
    "stif_siren_bwd": (C.c_int, [C.POINTER(SirenArgs), _P]),
    "stif_dec_x1_fwd": (C.c_int, [C.POINTER(DecTrainGeom), _P, _P]),
    "stif_dec_x1_bwd": (C.c_int, [C.POINTER(DecTrainGeom), _P, _P, _P]),
    "stif_dec_x2_fwd": (C.c_int, [C.POINTER(DecTrainGeom), _P, _P, _P]),
    "stif_dec_x2_bwd": (C.c_int, [C.POINTER(DecTrainGeom), _P, _P, _P, _P]),
    "stif_dec_x3_fwd": (C.c_int, [C.POINTER(DecTrainGeom), _P, _P, _P, _P]),
    "stif_dec_x3_bwd": (C.c_int, [C.POINTER(DecTrainGeom)] + [_P] * 7),
    "stif_conv_first": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P]),
    "stif_dcn_nhwc": (C.c_int, [C.POINTER(DcnArgs), _P]),
    "stif_dcn_sep_nhwc": (C.c_int, [C.POINTER(DcnSepArgs), _P]),
    "stif_dcn_bwd_workspace_size": (C.c_size_t, [C.c_int] * 3),
    "stif_dcn_bwd_nhwc": (C.c_int, [C.POINTER(DcnBwdArgs), _P]),
    "stif_dcn_bwd_contrib": (C.c_int, [C.POINTER(DcnBwdContribArgs), _P]),
    "stif_dec_x3_bwd_contrib": (C.c_int, [C.POINTER(DecTrainGeom)] + [_P] * 9),
    "stif_segsum": (C.c_int, [_P, _P, C.c_longlong, C.c_int, C.c_int, _P, _P, _P, C.c_longlong, C.c_longlong, C.c_int,
                              _P]),
    "stif_grad_pack": (C.c_int, [_P, C.c_int, _P, C.c_longlong, _P]),
    "stif_rank_sum": (C.c_int, [_P, C.c_longlong, C.c_int, _P, C.c_longlong, _P]),
    "stif_dcn_offmask_nhwc": (C.c_int, [_P, _P, C.c_longlong, C.c_longlong, C.c_int, C.c_int, C.c_int, _P]),
    "stif_dcn_v2_workspace_size": (C.c_size_t, [C.c_int] * 14),
    "stif_dcn_v2_forward": (C.c_int, [_P] * 6 + [C.c_int] * 14 + [_P, C.c_size_t, _P]),
    "stif_dcn_v2_backward_workspace_size": (C.c_size_t, [C.c_int] * 14),
    "stif_dcn_v2_backward": (C.c_int, [_P] * 11 + [C.c_int] * 14 + [_P, C.c_size_t, _P]),
    "stif_dec_pack_lr": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P]),
    "stif_dec_stage1": (C.c_int, [_P, _P, C.POINTER(DecTables), C.POINTER(DecImage), _P, _P, _P] + [C.c_int] * 5
                        + [_P]),
    "stif_dec_stage2": (C.c_int, [_P, _P, _P, _P, C.POINTER(DecTables), C.POINTER(DecImage), _P, _P]
                        + [C.c_int] * 5 + [_P]),
    "stif_dec_stage1_ex": (C.c_int, [_P, _P, C.POINTER(DecTables), C.POINTER(DecImage), _P, _P, _P]
                           + [C.c_int] * 6 + [_P, _P]),
    "stif_dec_stage2_ex": (C.c_int, [_P, _P, _P, _P, C.POINTER(DecTables), C.POINTER(DecImage), _P, _P]
                           + [C.c_int] * 6 + [_P, _P]),
    "stif_dec_stage1_win": (C.c_int, [_P, _P, C.POINTER(DecTables), C.POINTER(DecImage), _P, _P, _P]
                            + [C.c_int] * 6 + [_P, _P, C.POINTER(DecWindow)]),
    "stif_dec_bounds": (C.c_int, [_P, C.POINTER(DecTables), _P, C.c_int, C.c_int, C.c_int, _P, C.POINTER(DecWindow)]),
    "stif_dec_stage2_win": (C.c_int, [_P, _P, _P, _P, C.POINTER(DecTables), C.POINTER(DecImage), _P, _P]
                            + [C.c_int] * 6 + [_P, _P, C.POINTER(DecWindow)]),
    "stif_dec_flow_win": (C.c_int, [_P, _P, C.POINTER(DecTables), C.POINTER(DecImage), _P, _P, _P]
                          + [C.c_int] * 6 + [_P, _P, C.POINTER(DecWindow)]),
    "stif_dec_stage2_blend_win": (C.c_int, [_P, _P, _P, _P, C.POINTER(DecTables), C.POINTER(DecImage), _P, _P]
                                  + [C.c_int] * 6 + [_P, _P, C.POINTER(DecBlend), C.POINTER(DecWindow)]),
    "stif_dec_stage1_tf": (C.c_int, [_P, _P, C.POINTER(DecTables), C.POINTER(DecImage), C.POINTER(DecTimeField), _P, _P]
                           + [C.c_int] * 6 + [_P, _P, C.POINTER(DecWindow)]),
    "stif_dec_stage2_tf": (C.c_int, [_P, _P, _P, _P, C.POINTER(DecTables), C.POINTER(DecImage),
                                     C.POINTER(DecTimeField), _P] + [C.c_int] * 6 + [_P, _P, C.POINTER(DecWindow)]),
    "stif_dec_stage1_pts": (C.c_int, [_P, _P, C.POINTER(DecTables), C.POINTER(DecPointList), _P, _P]
                            + [C.c_int] * 6 + [_P, _P]),
    "stif_dec_corners_pts": (C.c_int, [_P, C.POINTER(DecTables), C.POINTER(DecPointList), _P, _P, _P]
                             + [C.c_int] * 3 + [_P, _P]),
    "stif_dec_stage2_pts": (C.c_int, [_P, _P, _P, _P, C.POINTER(DecTables), C.POINTER(DecPointList), _P]
                            + [C.c_int] * 6 + [_P, _P]),
    "stif_dec_remap_pts": (C.c_int, [C.POINTER(DecTables), C.POINTER(DecPointList), _P, _P] + [C.c_int] * 3 + [_P, _P]),
    "stif_dec_flow_pts": (C.c_int, [_P, _P, C.POINTER(DecTables), C.POINTER(DecPointList), _P, _P]
                          + [C.c_int] * 6 + [_P, _P]),
    "stif_dec_stage2_blend_pts": (C.c_int, [_P, _P, _P, _P, C.POINTER(DecTables), C.POINTER(DecPointList), _P]
                                  + [C.c_int] * 6 + [_P, _P, C.POINTER(DecBlend)]),
    "stif_dec_blend4": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, _P]),
    "stif_upsample_image": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "stif_resize_frames": (C.c_int, [_P, _P] + [C.c_int] * 5 + [_P, _P, C.c_int, C.c_int, _P, _P, C.c_int, C.c_int,
                                                                 _P]),
    "stif_frames_to_u8": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P]),
    "stif_build_batch": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, C.c_int, C.c_uint, _P]),
    "stif_pack_dec_proj_ex": (C.c_int, [_P, _P, _P, _P, C.c_int, _P, _P]),
    "stif_conv_weight_floats": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "stif_conv_bias_floats": (C.c_size_t, [C.c_int, C.c_int]),
    "stif_pack_conv_weight": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "stif_dec_proj_floats": (C.c_size_t, []),
    "stif_pack_dec_proj": (C.c_int, [_P] * 6),
    "stif_dec_mlp_floats": (C.c_size_t, []),
    "stif_pack_dec_mlp": (C.c_int, [C.POINTER(_P), C.POINTER(_P), C.POINTER(_P), _P]),
    "stif_pack_dec_mlp_ex": (C.c_int, [C.POINTER(_P), C.POINTER(_P), C.POINTER(_P), _P, C.c_int]),
    "stif_last_error": (C.c_char_p, []),
    "stif_version": (C.c_char_p, []),
}

_lib = None


E_INVALID, E_LAUNCH, E_WORKSPACE, E_RANGE = 1, 2, 3, 4   # stif.h STIF_E_*


class StifError(RuntimeError):
    """Raised for any non-zero status of the C ABI (the reference surfaces AT_ERROR as RuntimeError)."""

    def __init__(self, msg, code=None):
        super().__init__(msg)
        self.code = code


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise StifError(f"{LIB_PATH} not built; run `make` (or __graft_entry__.build())")
        h = C.CDLL(LIB_PATH)
        for name, (res, args) in EXPORTS.items():
            fn = getattr(h, name)
            fn.restype = res
            fn.argtypes = args
        _lib = h
    return _lib


def check(rc: int, what: str):
    if rc != 0:
        msg = lib().stif_last_error().decode(errors="replace")
        raise StifError(f"{what} failed (code {rc}): {msg}", rc)
