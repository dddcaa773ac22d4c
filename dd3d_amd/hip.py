"""ctypes binding of libdd3d_hip.so (C ABI declared in include/dd3d_hip.h).

The library is the ONLY compute path of this package: importing ``lib()`` raises if the shared object
has not been built (``python -c "import __graft_entry__ as g; g.build()"``) -- there is no eager / CPU
fallback anywhere in ``dd3d_amd``.
"""
import ctypes as C
import os

import numpy as np

# DD3D_HIP_LIB: alternate build of the same ABI (A/B measurements of two kernel versions on one box, tests/tools/ab_lib.sh)
_LIB_PATH = os.environ.get("DD3D_HIP_LIB") or os.path.join(os.path.dirname(__file__), "lib", "libdd3d_hip.so")
_lib = None

MAX_LEVELS = 8
MATH_F32, MATH_BF16X3, MATH_BF16X2, MATH_BF16, MATH_F16X2 = 0, 1, 2, 3, 4
MATH_PLANES = {MATH_F32: 0, MATH_BF16X3: 3, MATH_BF16X2: 2, MATH_BF16: 1, MATH_F16X2: 2}  # 16-bit terms per value (dd3d_math_planes)
ABI_VERSION = 7
STATUS_F16_OVERFLOW = 1
CAND_FIELDS = 22
DET_FIELDS = 32

TILE_128x128, TILE_128x64, TILE_64x64, TILE_128x32, TILE_64x128, TILE_256x128, TILE_128x128_W4, TILE_64x64_W4, TILE_128x64_W4, \
    TILE_128x64_K2, TILE_64x128_K2, TILE_64x64_W4K2, TILE_256x128_T42, TILE_128x256_T24, TILE_256x256_W8, TILE_128x32_W4, \
    TILE_192x256_W8 = range(17)
TILE_SHAPES = {TILE_128x128: (128, 128), TILE_128x64: (128, 64), TILE_64x64: (64, 64), TILE_128x32: (128, 32),
               TILE_64x128: (64, 128), TILE_256x128: (256, 128), TILE_128x128_W4: (128, 128), TILE_64x64_W4: (64, 64),
               TILE_128x64_W4: (128, 64), TILE_128x64_K2: (128, 64), TILE_64x128_K2: (64, 128), TILE_64x64_W4K2: (64, 64),
               TILE_256x128_T42: (256, 128), TILE_128x256_T24: (128, 256), TILE_256x256_W8: (256, 256), TILE_128x32_W4: (128, 32),
               TILE_192x256_W8: (192, 256)}
TILE_NAMES = {TILE_128x128: "128x128", TILE_128x64: "128x64", TILE_64x64: "64x64", TILE_128x32: "128x32", TILE_64x128: "64x128",
              TILE_256x128: "256x128", TILE_128x128_W4: "128x128w4", TILE_64x64_W4: "64x64w4", TILE_128x64_W4: "128x64w4", TILE_128x64_K2: "128x64k2",
              TILE_64x128_K2: "64x128k2", TILE_64x64_W4K2: "64x64w4k2", TILE_256x128_T42: "256x128t42", TILE_128x256_T24: "128x256t24",
              TILE_256x256_W8: "256x256w8", TILE_128x32_W4: "128x32w4", TILE_192x256_W8: "192x256w8"}

# numpy mirror of `dd3d_conv_seg` (120 bytes) -- arrays of it are uploaded to the device as raw bytes.
CONV_SEG_DTYPE = np.dtype(
    [("in_", "<u8"), ("w", "<u8"), ("scale", "<u8"), ("bias", "<u8"), ("lo", "<u8"), ("res", "<u8"), ("out", "<u8"),
     ("B", "<i4"), ("H", "<i4"), ("W", "<i4"), ("Ho", "<i4"), ("Wo", "<i4"), ("in_pitch", "<i4"), ("out_pitch", "<i4"),
     ("res_pitch", "<i4"), ("M", "<i4"), ("res_mode", "<i4"), ("in_planes", "<u8"), ("n_limit", "<i4"),
     ("reserved", "<i4"), ("out_planes", "<u8")]
)
assert CONV_SEG_DTYPE.itemsize == 120


class ConvLaunch(C.Structure):
    """`dd3d_conv_launch`."""
    _fields_ = [
        ("segs", C.c_void_p), ("tiles", C.c_void_p), ("workspace", C.c_void_p), ("nsegs", C.c_int32), ("ntiles", C.c_int32),
        ("KH", C.c_int32), ("KW", C.c_int32), ("stride", C.c_int32), ("pad", C.c_int32), ("Cin", C.c_int32), ("N", C.c_int32),
        ("Kpad", C.c_int32), ("Npad", C.c_int32), ("relu", C.c_int32), ("splitk", C.c_int32), ("math_mode", C.c_int32),
        ("tile_cfg", C.c_int32), ("zero_page", C.c_void_p), ("tile_counters", C.c_void_p), ("seg0_host", C.c_void_p), ("in_relu", C.c_int32),
        ("in_planes", C.c_int32), ("out_plane_scale", C.c_float), ("status", C.c_void_p), ("amax", C.c_void_p)
    ]


class SmallcArgs(C.Structure):
    """`dd3d_smallc_args`."""
    _fields_ = [
        ("in_", C.c_void_p), ("out", C.c_void_p), ("w3", C.c_void_p), ("scale", C.c_void_p), ("bias", C.c_void_p), ("lo", C.c_void_p),
        ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("Ho", C.c_int32), ("Wo", C.c_int32), ("in_pitch", C.c_int32),
        ("out_pitch", C.c_int32), ("Cin", C.c_int32), ("KH", C.c_int32), ("KW", C.c_int32), ("stride", C.c_int32), ("pad", C.c_int32),
        ("N", C.c_int32), ("relu", C.c_int32)
    ]


class StemArgs(C.Structure):
    """`dd3d_stem_args`."""
    _fields_ = [
        ("src", C.c_void_p), ("sizes", C.c_void_p), ("mean", C.c_float * 3), ("stdv", C.c_float * 3), ("w1", C.c_void_p), ("scale1", C.c_void_p),
        ("bias1", C.c_void_p), ("w2", C.c_void_p), ("scale2", C.c_void_p), ("bias2", C.c_void_p), ("w3", C.c_void_p), ("scale3", C.c_void_p),
        ("bias3", C.c_void_p), ("out", C.c_void_p), ("out_planes", C.c_void_p), ("B", C.c_int32), ("Hp", C.c_int32), ("Wp", C.c_int32),
        ("out_pitch", C.c_int32), ("plane_scale", C.c_float), ("status", C.c_void_p), ("K", C.c_void_p), ("inv_K", C.c_void_p),
        ("zero_f32", C.c_void_p), ("zero_count", C.c_int32)
    ]


class StemKeepArgs(C.Structure):
    """`dd3d_stem_keep_args`."""
    _fields_ = [("stem", StemArgs), ("keep_base", C.c_void_p), ("keep_level0", C.c_void_p), ("keep_base_pitch", C.c_int32), ("keep_level0_pitch", C.c_int32)]


class ResizeArgs(C.Structure):
    """`dd3d_resize_args`."""
    _fields_ = [
        ("src", C.c_void_p), ("dst", C.c_void_p), ("tmp", C.c_void_p), ("C", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
        ("new_h", C.c_int32), ("new_w", C.c_int32), ("src_plane", C.c_int64), ("dst_plane", C.c_int64), ("src_row", C.c_int32),
        ("dst_row", C.c_int32), ("lo_w", C.c_void_p), ("cnt_w", C.c_void_p), ("kk_w", C.c_void_p), ("lo_h", C.c_void_p),
        ("cnt_h", C.c_void_p), ("kk_h", C.c_void_p), ("ksize_w", C.c_int32), ("ksize_h", C.c_int32)
    ]


class SelectArgs(C.Structure):
    """`dd3d_select_args`."""
    _fields_ = [
        ("cls", C.c_void_p * MAX_LEVELS), ("box2d", C.c_void_p * MAX_LEVELS), ("box3d", C.c_void_p * MAX_LEVELS),
        ("H", C.c_int32 * MAX_LEVELS), ("W", C.c_int32 * MAX_LEVELS), ("stride", C.c_int32 * MAX_LEVELS),
        ("cls_pitch", C.c_int32), ("b2d_pitch", C.c_int32), ("b3d_pitch", C.c_int32), ("num_levels", C.c_int32),
        ("B", C.c_int32), ("num_classes", C.c_int32), ("class_agnostic_3d", C.c_int32), ("loc_offset_half", C.c_int32),
        ("thresh_with_ctr", C.c_int32), ("topk", C.c_int32), ("attr_off", C.c_int32), ("num_attr", C.c_int32),
        ("speed_off", C.c_int32), ("pre_nms_thresh", C.c_float), ("min_depth", C.c_float),
        ("max_depth", C.c_float), ("focal_factor", C.c_float), ("scale_depth_by_focal", C.c_int32), ("allocentric", C.c_int32),
        ("depth_is_distance", C.c_int32), ("inv_K", C.c_void_p), ("canon_sizes", C.c_void_p), ("scratch_idx", C.c_void_p),
        ("scratch_score", C.c_void_p), ("scratch_off", C.c_int64 * MAX_LEVELS), ("scratch_img_stride", C.c_int64),
        ("cand", C.c_void_p), ("counts", C.c_void_p), ("npass", C.c_void_p), ("slot_off", C.c_int32 * (MAX_LEVELS + 1))
    ]


class NmsArgs(C.Structure):
    """`dd3d_nms_args`."""
    _fields_ = [
        ("cand", C.c_void_p), ("counts", C.c_void_p), ("G", C.c_int32), ("num_levels", C.c_int32), ("topk", C.c_int32),
        ("do_nms", C.c_int32), ("use_score3d", C.c_int32), ("nms_thresh", C.c_float), ("post_topk", C.c_int32),
        ("do_postprocess", C.c_int32), ("out_size", C.c_void_p), ("sort_idx", C.c_void_p), ("sbox", C.c_void_p),
        ("scls", C.c_void_p), ("mask", C.c_void_p), ("nvalid", C.c_void_p), ("det", C.c_void_p), ("det_count", C.c_void_p),
        ("det_cap", C.c_int32), ("slot_off", C.c_int32 * (MAX_LEVELS + 1)), ("img_first", C.c_int32), ("img_per_rec", C.c_int32),
        ("rec_stride", C.c_int64)
    ]


class BevArgs(C.Structure):
    """`dd3d_bev_args`."""
    _fields_ = [
        ("det_in", C.c_void_p), ("count_in", C.c_void_p), ("inv_K", C.c_void_p), ("pose", C.c_void_p), ("group", C.c_void_p),
        ("out_size", C.c_void_p), ("G", C.c_int32), ("det_cap", C.c_int32), ("num_classes", C.c_int32),
        ("iou_thresh", C.c_float), ("max_dets", C.c_int32), ("write_global", C.c_int32),
        ("do_postprocess", C.c_int32), ("work", C.c_void_p), ("sbox", C.c_void_p), ("mask", C.c_void_p), ("meta", C.c_void_p),
        ("det_out", C.c_void_p), ("count_out", C.c_void_p), ("img_first", C.c_int32), ("img_per_rec", C.c_int32), ("rec_stride", C.c_int64)
    ]


class KittiMatchArgs(C.Structure):
    """`dd3d_kitti_match_args`."""
    _fields_ = [
        ("ov", C.c_void_p), ("ov_off", C.c_void_p), ("dt_begin", C.c_void_p), ("gt_begin", C.c_void_p), ("dt_score", C.c_void_p),
        ("ign_dt", C.c_void_p), ("ign_gt", C.c_void_p), ("min_overlap", C.c_void_p), ("n_ov", C.c_int64), ("n_img", C.c_int32),
        ("n_dt", C.c_int32), ("n_gt", C.c_int32), ("n_cd", C.c_int32), ("n_o", C.c_int32), ("max_dt", C.c_int32), ("max_gt", C.c_int32)
    ]


KITTI_MAX_DT_PER_IMAGE, KITTI_MAX_GT_PER_IMAGE, KITTI_MAX_OVERLAPS, KITTI_MAX_THRESHOLDS = 8192, 1024, 8, 256

NUSC_MAX_PRED_PER_SEGMENT, NUSC_MAX_GT_PER_SEGMENT, NUSC_MAX_THRESHOLDS = 500, 4096, 8


class NuscMatchArgs(C.Structure):
    """`dd3d_nusc_match_args`."""
    _fields_ = [
        ("pred_xy", C.c_void_p), ("gt_xy", C.c_void_p), ("pred_begin", C.c_void_p), ("gt_begin", C.c_void_p), ("pred_begin_host", C.c_void_p),
        ("gt_begin_host", C.c_void_p), ("n_seg", C.c_int32), ("n_pred", C.c_int32), ("n_gt", C.c_int32), ("n_thr", C.c_int32),
        ("thr", C.c_double * NUSC_MAX_THRESHOLDS)
    ]

LOSS_GT_FIELDS, LOSS_MAX_GT, LOSS_BOX3D_FIELDS, LOSS_TERMS, LOSS_OUT = 28, 512, 19, 16, 16
LOSS_BLOCK = 256  # targets per block of dd3d_loss_terms: one partial row per block


class LossArgs(C.Structure):
    """`dd3d_loss_args`."""
    _fields_ = [
        ("cls", C.c_void_p * MAX_LEVELS), ("box2d", C.c_void_p * MAX_LEVELS), ("box3d", C.c_void_p * MAX_LEVELS), ("locations", C.c_void_p),
        ("gt_off", C.c_void_p), ("gt", C.c_void_p), ("inv_K", C.c_void_p), ("canon_sizes", C.c_void_p), ("labels", C.c_void_p),
        ("target_inds", C.c_void_p), ("box2d_reg", C.c_void_p), ("ctr_target", C.c_void_p), ("box3d_t", C.c_void_p), ("attributes", C.c_void_p),
        ("speeds", C.c_void_p), ("flags", C.c_void_p), ("partials", C.c_void_p), ("out", C.c_void_p), ("num_pos", C.c_void_p),
        ("H", C.c_int32 * MAX_LEVELS), ("W", C.c_int32 * MAX_LEVELS), ("loc_off", C.c_int32 * (MAX_LEVELS + 1)),
        ("soi_lo", C.c_float * MAX_LEVELS), ("soi_hi", C.c_float * MAX_LEVELS), ("radius", C.c_float * MAX_LEVELS),
        ("num_levels", C.c_int32), ("B", C.c_int32), ("num_classes", C.c_int32), ("max_gt", C.c_int32), ("n_partials", C.c_int32),
        ("cls_pitch", C.c_int32), ("b2d_pitch", C.c_int32), ("b3d_pitch", C.c_int32), ("attr_off", C.c_int32), ("num_attr", C.c_int32),
        ("speed_off", C.c_int32), ("center_sample", C.c_int32), ("class_agnostic_3d", C.c_int32), ("scale_depth_by_focal", C.c_int32),
        ("allocentric", C.c_int32), ("depth_is_distance", C.c_int32), ("min_depth", C.c_float), ("max_depth", C.c_float),
        ("focal_factor", C.c_float), ("focal_alpha", C.c_float), ("focal_gamma", C.c_float), ("smooth_l1_beta", C.c_float),
        ("conf3d_temperature", C.c_float), ("weight_box3d", C.c_float), ("weight_conf3d", C.c_float), ("weight_attr", C.c_float),
        ("weight_speed", C.c_float)
    ]


LOSS_GRAD_DENOMS = 4


class LossGradArgs(C.Structure):
    """`dd3d_loss_grad_args`."""
    _fields_ = [
        ("d_cls", C.c_void_p * MAX_LEVELS), ("d_box2d", C.c_void_p * MAX_LEVELS), ("d_box3d", C.c_void_p * MAX_LEVELS),
        ("upstream", C.c_void_p), ("denoms", C.c_void_p)
    ]


DDL_ROW, DDL_MAX_BLOCKS = 12, 1024
DDL_QUADS_PER_BLOCK = 256  # dd3d_dense_depth_loss: a block of 256 threads reads 256 four-pixel groups per sweep


def dense_depth_loss_blocks(B, Hp, Wp):
    """Blocks (= partial rows) of one dd3d_dense_depth_loss launch on a B x Hp x Wp canvas."""
    quads = B * Hp * (Wp // 4)
    return min((quads + DDL_QUADS_PER_BLOCK - 1) // DDL_QUADS_PER_BLOCK, DDL_MAX_BLOCKS)


class DenseDepthLossArgs(C.Structure):
    """`dd3d_dense_depth_loss_args`."""
    _fields_ = [
        ("raw", C.c_void_p * MAX_LEVELS), ("gt", C.c_void_p), ("inv_K", C.c_void_p), ("partials", C.c_void_p), ("out", C.c_void_p),
        ("count", C.c_void_p), ("h", C.c_int32 * MAX_LEVELS), ("w", C.c_int32 * MAX_LEVELS), ("stride", C.c_int32 * MAX_LEVELS),
        ("divisor", C.c_float * MAX_LEVELS), ("num_levels", C.c_int32), ("B", C.c_int32), ("Hp", C.c_int32), ("Wp", C.c_int32),
        ("pitch", C.c_int32), ("offset_half", C.c_int32), ("n_partials", C.c_int32), ("focal_factor", C.c_float), ("min_depth", C.c_float),
        ("max_depth", C.c_float), ("beta", C.c_float), ("loss_weight", C.c_float)
    ]


DDG_ROW = 4  # floats per slab row of dd3d_dense_depth_loss_backward: the four corner sums of one sub-tile of a cell


class DenseDepthGradArgs(C.Structure):
    """`dd3d_dense_depth_grad_args`."""
    _fields_ = [("d_raw", C.c_void_p * MAX_LEVELS), ("upstream", C.c_void_p), ("slab", C.c_void_p), ("n_slab", C.c_int64)]


def dense_depth_grad_rows(args):
    """Slab rows one dd3d_dense_depth_loss_backward call on the filled-in DenseDepthLossArgs `args` writes (the library's own count: one
    row per level, image, cell and sub-tile); raises like `check` when the gradient cannot run on these args."""
    n = lib().dd3d_dense_depth_grad_rows(C.byref(args))
    if n < 0:
        raise RuntimeError(f"libdd3d_hip dense_depth_grad_rows failed: {lib().dd3d_last_error().decode()}")
    return int(n)


PG_MAX_SLOTS, PG_MAX_N, PG_UNIT = 8, 256, 64
PG_ACT_F32, PG_ACT_F16X2, PG_ACT_BF16X3 = 0, 1, 2
PG_TARGET_SLICES = 48  # csrc/predictor_grads.hip::PG_TARGET_SLICES


class PredGradArgs(C.Structure):
    """`dd3d_pred_grad_args`."""
    _fields_ = [
        ("act", C.c_void_p * MAX_LEVELS), ("g", C.c_void_p * MAX_LEVELS), ("map", C.c_void_p * MAX_LEVELS), ("w", C.c_void_p * MAX_LEVELS),
        ("bias", C.c_void_p * MAX_LEVELS), ("scale", C.c_void_p * MAX_LEVELS), ("da", C.c_void_p * MAX_LEVELS), ("lo", C.c_void_p),
        ("slot", C.c_void_p), ("part", C.c_void_p), ("qpart", C.c_void_p), ("dw_level", C.c_void_p), ("dw", C.c_void_p), ("db", C.c_void_p),
        ("q", C.c_void_p), ("r", C.c_void_p), ("dscale", C.c_void_p), ("doffset", C.c_void_p), ("H", C.c_int32 * MAX_LEVELS),
        ("W", C.c_int32 * MAX_LEVELS), ("num_levels", C.c_int32), ("B", C.c_int32), ("Cin", C.c_int32), ("n", C.c_int32),
        ("g_pitch", C.c_int32), ("act_mode", C.c_int32), ("act_pitch", C.c_int32), ("n_slices", C.c_int32), ("plane_scale", C.c_float)
    ]


def pred_grad_slices(B, level_hw):
    """Rows of `part` / `qpart` one dd3d_predictor_wgrad call needs (the rule of dd3d_predictor_grad_slices, for plans built without a device)."""
    units = [B * h * ((w + PG_UNIT - 1) // PG_UNIT) for h, w in level_hw]
    ups = max(1, (sum(units) + PG_TARGET_SLICES - 1) // PG_TARGET_SLICES)
    return sum((u + ups - 1) // ups for u in units)


TG_MAX_C, TG_UNIT, TG_MIN_UNITS_PER_SLICE, TG_SLAB_BYTES, TG_MIN_TILES = 256, 64, 4, 160 << 20, 512


class TowerGradArgs(C.Structure):
    """`dd3d_tower_grad_args`."""
    _fields_ = [
        ("x", C.c_void_p * MAX_LEVELS), ("y", C.c_void_p * MAX_LEVELS), ("g", C.c_void_p * MAX_LEVELS), ("scale", C.c_void_p * MAX_LEVELS),
        ("da_add", C.c_void_p * MAX_LEVELS), ("da", C.c_void_p * MAX_LEVELS), ("w", C.c_void_p), ("part", C.c_void_p), ("qpart", C.c_void_p),
        ("dw_level", C.c_void_p), ("dw", C.c_void_p), ("q", C.c_void_p), ("r", C.c_void_p), ("H", C.c_int32 * MAX_LEVELS),
        ("W", C.c_int32 * MAX_LEVELS), ("num_levels", C.c_int32), ("B", C.c_int32), ("Cin", C.c_int32), ("Cout", C.c_int32),
        ("g_pitch", C.c_int32), ("x_mode", C.c_int32), ("x_pitch", C.c_int32), ("y_mode", C.c_int32), ("y_pitch", C.c_int32),
        ("n_slices", C.c_int32), ("dgrad_rows", C.c_int32), ("x_plane_scale", C.c_float), ("y_plane_scale", C.c_float)
    ]


def tower_grad_slices(B, level_hw, Cin, Cout):
    """Rows of `part` / `qpart` one dd3d_tower_wgrad call needs (the rule of dd3d_tower_grad_slices, for plans built without a device):
    at least TG_MIN_UNITS_PER_SLICE 64-pixel units per slice, more once the slab would pass TG_SLAB_BYTES."""
    units = [B * h * ((w + TG_UNIT - 1) // TG_UNIT) for h, w in level_hw]
    max_slices = max(1, TG_SLAB_BYTES // (Cout * 9 * Cin * 4))
    ups = max(TG_MIN_UNITS_PER_SLICE, (sum(units) + max_slices - 1) // max_slices)
    return sum((u + ups - 1) // ups for u in units)


FG_MAX_CIN, FG_MAX_COUT, FG_UNIT, FG_MIN_UNITS_PER_SLICE, FG_SLAB_BYTES, FG_MIN_TILES = 1024, 256, 64, 4, 160 << 20, 512


class FpnGradArgs(C.Structure):
    """`dd3d_fpn_grad_args`."""
    _fields_ = [
        ("x", C.c_void_p * MAX_LEVELS), ("g", C.c_void_p * MAX_LEVELS), ("w", C.c_void_p * MAX_LEVELS), ("scale", C.c_void_p * MAX_LEVELS),
        ("mask", C.c_void_p * MAX_LEVELS), ("add", C.c_void_p * MAX_LEVELS), ("pool", C.c_void_p * MAX_LEVELS), ("da", C.c_void_p * MAX_LEVELS),
        ("part", C.c_void_p), ("qpart", C.c_void_p), ("dw_level", C.c_void_p), ("dw", C.c_void_p), ("q", C.c_void_p), ("r", C.c_void_p),
        ("H", C.c_int32 * MAX_LEVELS), ("W", C.c_int32 * MAX_LEVELS), ("pool_H", C.c_int32 * MAX_LEVELS), ("pool_W", C.c_int32 * MAX_LEVELS),
        ("num_levels", C.c_int32), ("B", C.c_int32), ("Cin", C.c_int32), ("Cout", C.c_int32), ("g_pitch", C.c_int32), ("ksize", C.c_int32),
        ("stride", C.c_int32), ("in_relu", C.c_int32), ("x_mode", C.c_int32), ("x_pitch", C.c_int32), ("mask_mode", C.c_int32),
        ("mask_pitch", C.c_int32), ("n_slices", C.c_int32), ("dgrad_rows", C.c_int32), ("x_plane_scale", C.c_float), ("mask_plane_scale", C.c_float)
    ]


def fpn_grad_slices(B, level_hw, Cin, Cout, ksize, stride):
    """Rows of `part` / `qpart` one dd3d_fpn_wgrad call needs (the rule of dd3d_fpn_grad_slices, for plans built without a device):
    the largest level's count.  `level_hw`: the INPUT sizes; a unit is 64 (stride 2: 32) output pixels of a row."""
    unit = FG_UNIT // 2 if stride == 2 else FG_UNIT
    max_slices = max(1, FG_SLAB_BYTES // (Cout * ksize * ksize * Cin * 4))
    n = 0
    for h, w in level_hw:
        ho, wo = (h + stride - 1) // stride, (w + stride - 1) // stride
        units = B * ho * ((wo + unit - 1) // unit)
        ups = max(FG_MIN_UNITS_PER_SLICE, (units + max_slices - 1) // max_slices)
        n = max(n, (units + ups - 1) // ups)
    return n


BG_MAX_CIN, BG_MAX_COUT, BG_UNIT, BG_MIN_UNITS_PER_SLICE, BG_MIN_TILES, BG_MAX_PIXELS = 1280, 512, 64, 4, 512, 1 << 26


class BackboneGradArgs(C.Structure):
    """`dd3d_backbone_grad_args`."""
    _fields_ = [
        ("x", C.c_void_p), ("y", C.c_void_p), ("g", C.c_void_p), ("w", C.c_void_p), ("scale", C.c_void_p), ("add", C.c_void_p),
        ("res_g", C.c_void_p), ("res_y", C.c_void_p), ("da", C.c_void_p), ("part", C.c_void_p), ("qpart", C.c_void_p), ("dw_level", C.c_void_p),
        ("dw", C.c_void_p), ("q", C.c_void_p), ("r", C.c_void_p), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("Cin", C.c_int32),
        ("Cout", C.c_int32), ("ksize", C.c_int32), ("stride", C.c_int32), ("g_pitch", C.c_int32), ("add_pitch", C.c_int32),
        ("res_pitch", C.c_int32), ("da_pitch", C.c_int32), ("x_mode", C.c_int32), ("x_pitch", C.c_int32), ("y_mode", C.c_int32),
        ("y_pitch", C.c_int32), ("res_y_mode", C.c_int32), ("res_y_pitch", C.c_int32), ("n_slices", C.c_int32), ("dgrad_rows", C.c_int32),
        ("dgrad_group", C.c_int32), ("x_plane_scale", C.c_float), ("y_plane_scale", C.c_float), ("res_y_plane_scale", C.c_float)
    ]


class PoolGradArgs(C.Structure):
    """`dd3d_pool_grad_args`."""
    _fields_ = [
        ("x", C.c_void_p), ("g", C.c_void_p), ("res_g", C.c_void_p), ("res_y", C.c_void_p), ("add", C.c_void_p), ("da", C.c_void_p),
        ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32), ("x_mode", C.c_int32), ("x_pitch", C.c_int32),
        ("res_y_mode", C.c_int32), ("res_y_pitch", C.c_int32), ("g_pitch", C.c_int32), ("res_pitch", C.c_int32), ("add_pitch", C.c_int32),
        ("da_pitch", C.c_int32), ("x_plane_scale", C.c_float), ("res_y_plane_scale", C.c_float)
    ]


def backbone_grad_slices(B, H, W, Cin, Cout, ksize, stride):
    """Rows of `part` / `qpart` one dd3d_backbone_wgrad call needs (the rule of dd3d_backbone_grad_slices, for plans built without a
    device).  H, W: the INPUT's sizes; a unit is 64 (stride 2: 32) output pixels of a row; the slab stays within TG_SLAB_BYTES."""
    unit = BG_UNIT // 2 if stride == 2 else BG_UNIT
    max_slices = max(1, TG_SLAB_BYTES // (Cout * ksize * ksize * Cin * 4))
    ho, wo = (H + stride - 1) // stride, (W + stride - 1) // stride
    units = B * ho * ((wo + unit - 1) // unit)
    ups = max(BG_MIN_UNITS_PER_SLICE, (units + max_slices - 1) // max_slices)
    return (units + ups - 1) // ups


VG_MAX_CIN, VG_MAX_COUT, EG_MAX_RSPLIT = 2144, 1024, 64


class EseGradArgs(C.Structure):
    """`dd3d_ese_grad_args`."""
    _fields_ = [
        ("xt", C.c_void_p), ("g", C.c_void_p), ("fc_w", C.c_void_p), ("fc_b", C.c_void_p), ("part", C.c_void_p), ("m", C.c_void_p), ("z", C.c_void_p),
        ("s", C.c_void_p), ("dz", C.c_void_p), ("u", C.c_void_p), ("g_xt", C.c_void_p), ("d_fc_w", C.c_void_p), ("d_fc_b", C.c_void_p),
        ("B", C.c_int32), ("HW", C.c_int32), ("C", C.c_int32), ("rsplit", C.c_int32), ("xt_mode", C.c_int32), ("xt_pitch", C.c_int32),
        ("g_pitch", C.c_int32), ("gxt_pitch", C.c_int32), ("xt_plane_scale", C.c_float), ("reserved", C.c_int32)
    ]


class Pool3GradArgs(C.Structure):
    """`dd3d_pool3_grad_args`."""
    _fields_ = [
        ("x", C.c_void_p), ("g", C.c_void_p), ("add", C.c_void_p), ("da", C.c_void_p), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
        ("C", C.c_int32), ("x_mode", C.c_int32), ("x_pitch", C.c_int32), ("g_pitch", C.c_int32), ("add_pitch", C.c_int32), ("da_pitch", C.c_int32),
        ("x_plane_scale", C.c_float)
    ]


def pool3_out(n):
    """Output size of MaxPool2d(3, 2, ceil_mode=True) on n >= 3 rows (dd3d_maxpool3x3s2_ceil_nhwc's rule): ceil((n - 3) / 2) + 1, minus one
    when the last window would start outside the map."""
    o = (n - 3 + 1) // 2 + 1
    return o - 1 if (o - 1) * 2 >= n else o


def ese_grad_rsplit(HW):
    """Row splits of one dd3d_ese_backward call: the forward gate's rule (a split per 256 rows, at most EG_MAX_RSPLIT)."""
    return max(1, min(EG_MAX_RSPLIT, HW // 256))


SG_UNIT, SG_TARGET_SLICES, SG_MIN_UNITS_PER_SLICE, SG_MAX_UNITS_PER_SLICE = 64, 512, 8, 64
STEM_GRAD_SHAPES = ((7, 1, 4, 16), (3, 1, 16, 16), (3, 2, 16, 32))  # (ksize, stride, Cin, Cout) of base_layer, level0.0, level1.0
VOVNET_STEM_GRAD_SHAPE = (3, 2, 4, 64)  # (ksize, stride, Cin, Cout) of the VoVNet-V2 stem_1 (dd3d_vovnet_stem_wgrad)


class StemGradArgs(C.Structure):
    """`dd3d_stem_grad_args`."""
    _fields_ = [
        ("x", C.c_void_p), ("y", C.c_void_p), ("g", C.c_void_p), ("w", C.c_void_p), ("scale", C.c_void_p), ("da", C.c_void_p),
        ("part", C.c_void_p), ("qpart", C.c_void_p), ("dw_level", C.c_void_p), ("dw", C.c_void_p), ("q", C.c_void_p), ("r", C.c_void_p),
        ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("Cin", C.c_int32), ("Cout", C.c_int32), ("ksize", C.c_int32),
        ("stride", C.c_int32), ("x_pitch", C.c_int32), ("g_pitch", C.c_int32), ("da_pitch", C.c_int32), ("y_mode", C.c_int32),
        ("y_pitch", C.c_int32), ("n_slices", C.c_int32), ("wgrad_blocks", C.c_int32), ("y_plane_scale", C.c_float)
    ]


def stem_grad_slices(B, H, W, Cin, Cout, ksize, stride):
    """Rows of `part` / `qpart` one dd3d_stem_wgrad call needs (the rule of dd3d_stem_grad_slices, for plans built without a device).
    H, W: the INPUT's sizes; a unit is up to 64 output pixels of a row; about SG_TARGET_SLICES slices of 8 to 64 units, more units once the
    slab would pass TG_SLAB_BYTES."""
    ho, wo = (H + stride - 1) // stride, (W + stride - 1) // stride
    units = B * ho * ((wo + SG_UNIT - 1) // SG_UNIT)
    ups = min(max((units + SG_TARGET_SLICES - 1) // SG_TARGET_SLICES, SG_MIN_UNITS_PER_SLICE), SG_MAX_UNITS_PER_SLICE)
    max_slices = TG_SLAB_BYTES // (Cout * ksize * ksize * Cin * 4)
    if ups * max_slices < units:
        ups = (units + max_slices - 1) // max_slices
    return (units + ups - 1) // ups


def vovnet_stem_grad_slices(B, H, W):
    """Rows of `part` / `qpart` one dd3d_vovnet_stem_wgrad call needs (the rule of dd3d_vovnet_stem_grad_slices -- stem_grad_slices' at
    VOVNET_STEM_GRAD_SHAPE --, for plans built without a device).  H, W: the INPUT's sizes."""
    ksize, stride, Cin, Cout = VOVNET_STEM_GRAD_SHAPE
    return stem_grad_slices(B, H, W, Cin, Cout, ksize, stride)


BN_MAX_SEGS, BN_MAX_C, BN_SLICE, BN_STAT_ROWS = 24, 256, 64, 7
BN_ROW_MU, BN_ROW_VAR, BN_ROW_S, BN_ROW_T, BN_ROW_RSTD, BN_ROW_RUN_MEAN, BN_ROW_RUN_VAR = range(7)
BN_MOMENTUM = 0.1  # nn.BatchNorm2d's default, which the reference's get_norm("BN") uses


class TowerBnArgs(C.Structure):
    """`dd3d_tower_bn_args`."""
    _fields_ = [
        ("c", C.c_void_p * BN_MAX_SEGS), ("gamma", C.c_void_p * BN_MAX_SEGS), ("beta", C.c_void_p * BN_MAX_SEGS), ("run_mean", C.c_void_p * BN_MAX_SEGS),
        ("run_var", C.c_void_p * BN_MAX_SEGS), ("stats", C.c_void_p * BN_MAX_SEGS), ("y", C.c_void_p * BN_MAX_SEGS), ("g", C.c_void_p * BN_MAX_SEGS),
        ("qp", C.c_void_p * BN_MAX_SEGS), ("gc", C.c_void_p * BN_MAX_SEGS), ("part", C.c_void_p), ("status", C.c_void_p), ("N", C.c_int32 * BN_MAX_SEGS),
        ("num_segs", C.c_int32), ("C", C.c_int32), ("c_pitch", C.c_int32), ("g_pitch", C.c_int32), ("math_mode", C.c_int32), ("y_mode", C.c_int32),
        ("y_pitch", C.c_int32), ("n_slices", C.c_int32), ("eps", C.c_float), ("momentum", C.c_float), ("plane_scale", C.c_float), ("reserved", C.c_int32)
    ]


class FpnBnArgs(C.Structure):
    """`dd3d_fpn_bn_args`."""
    _fields_ = [
        ("bn", TowerBnArgs), ("y32", C.c_void_p * BN_MAX_SEGS), ("up", C.c_int32 * BN_MAX_SEGS), ("B", C.c_int32 * BN_MAX_SEGS),
        ("H", C.c_int32 * BN_MAX_SEGS), ("W", C.c_int32 * BN_MAX_SEGS), ("y32_pitch", C.c_int32), ("reserved", C.c_int32)
    ]


BBN_MIN_C, BBN_MAX_C = 16, 512  # the widths of csrc/backbone_bn.hip: 16, multiples of 32 up to 256, multiples of 256 up to 512
BBN_RELU, BBN_LINEAR, BBN_RESIDUAL = range(3)


class BackboneBnArgs(C.Structure):
    """`dd3d_backbone_bn_args`."""
    _fields_ = [
        ("bn", TowerBnArgs), ("y32", C.c_void_p * BN_MAX_SEGS), ("res", C.c_void_p * BN_MAX_SEGS), ("act", C.c_int32), ("res_mode", C.c_int32),
        ("res_pitch", C.c_int32), ("y32_pitch", C.c_int32), ("res_plane_scale", C.c_float), ("reserved", C.c_int32)
    ]


def backbone_bn_width_ok(Cc):
    """The rule of dd3d_backbone_bn_*: C = 16, a multiple of 32 up to 256, or a multiple of 256 up to 512."""
    return Cc == BBN_MIN_C or (Cc >= 32 and Cc % 32 == 0 and Cc <= 256) or (Cc > 0 and Cc % 256 == 0 and Cc <= BBN_MAX_C)


def bn_slices(pixels):
    """Rows of `part` one dd3d_bn_batch_stats / dd3d_bn_backward_reduce call needs for segments of `pixels` pixels each (the rule of
    dd3d_bn_slices, for plans built without a device)."""
    return sum((n + BN_SLICE - 1) // BN_SLICE for n in pixels)


EXPORTS = [
    "dd3d_abi_version", "dd3d_last_error", "dd3d_arch", "dd3d_build_flags", "dd3d_conv_tile_shape", "dd3d_conv_row_rings", "dd3d_conv2d_igemm_f32",
    "dd3d_preprocess_u8_nhwc4", "dd3d_maxpool2x2_nhwc", "dd3d_maxpool3x3s2_ceil_nhwc", "dd3d_ese_nhwc", "dd3d_upsample2x_add_nhwc", "dd3d_fcos_select_decode",
    "dd3d_invert_intrinsics", "dd3d_nms_finalize", "dd3d_bev_nms_aggregate", "dd3d_conv2d_smallc_supported", "dd3d_conv2d_smallc_bf16x3", "dd3d_rotate_iou_eval", "dd3d_d3_box_overlap", "dd3d_image_box_overlap", "dd3d_aligned_bilinear_scale", "dd3d_resize_bilinear_u8",
    "dd3d_format_boxes3d", "dd3d_math_planes", "dd3d_split_planes", "dd3d_maxpool2x2_planes", "dd3d_maxpool2x2_planes_in", "dd3d_upsample2x_add_planes", "dd3d_ese_fused", "dd3d_stem_fused_f16x2", "dd3d_stem_fused_keep_f16x2", "dd3d_fold_range_flags", "dd3d_pack_readback",
    "dd3d_kitti_tp_scores", "dd3d_kitti_pr_counts", "dd3d_nusc_center_match", "dd3d_loss_assign", "dd3d_loss_terms", "dd3d_loss_layout",
    "dd3d_dense_depth_loss", "dd3d_dense_depth_loss_layout", "dd3d_loss_backward", "dd3d_loss_grad_layout",
    "dd3d_dense_depth_loss_backward", "dd3d_dense_depth_grad_rows", "dd3d_dense_depth_grad_layout",
    "dd3d_predictor_wgrad", "dd3d_predictor_dgrad", "dd3d_predictor_grad_slices", "dd3d_pred_grad_layout",
    "dd3d_tower_wgrad", "dd3d_tower_dgrad", "dd3d_tower_grad_slices", "dd3d_tower_grad_layout",
    "dd3d_fpn_wgrad", "dd3d_fpn_dgrad", "dd3d_fpn_grad_slices", "dd3d_fpn_grad_layout",
    "dd3d_backbone_wgrad", "dd3d_backbone_dgrad", "dd3d_backbone_grad_slices", "dd3d_maxpool2x2_backward", "dd3d_backbone_grad_layout",
    "dd3d_stem_wgrad", "dd3d_stem_dgrad", "dd3d_stem_grad_slices", "dd3d_stem_grad_layout",
    "dd3d_vovnet_stem_wgrad", "dd3d_vovnet_stem_grad_slices",
    "dd3d_vovnet_conv_wgrad", "dd3d_vovnet_conv_dgrad", "dd3d_vovnet_conv_grad_slices", "dd3d_vovnet_add", "dd3d_ese_backward", "dd3d_maxpool3x3s2_ceil_backward",
    "dd3d_vovnet_grad_layout",
    "dd3d_bn_batch_stats", "dd3d_bn_apply_relu_split", "dd3d_bn_backward_reduce", "dd3d_bn_backward_apply", "dd3d_bn_slices", "dd3d_tower_bn_layout",
    "dd3d_bn_apply_topdown_split", "dd3d_bn_backward_reduce_linear", "dd3d_bn_backward_apply_linear", "dd3d_fpn_bn_layout",
    "dd3d_backbone_bn_batch_stats", "dd3d_backbone_bn_apply", "dd3d_backbone_bn_backward_reduce", "dd3d_backbone_bn_backward_apply",
    "dd3d_backbone_bn_backward_reduce_linear", "dd3d_backbone_bn_backward_apply_linear", "dd3d_backbone_bn_slices", "dd3d_backbone_bn_layout"
]


class HipLibraryMissing(RuntimeError):
    pass


def lib_path():
    return _LIB_PATH


def build_flags():
    """Build-time knobs of the loaded library ("" = the product build)."""
    return lib().dd3d_build_flags().decode()


def lib():
    """Load (once) and return the ctypes handle.  Raises HipLibraryMissing if the .so is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise HipLibraryMissing(
            f"{_LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'`. "
            "dd3d_amd has no CPU / eager fallback."
        )
    L = C.CDLL(_LIB_PATH)
    L.dd3d_abi_version.restype = C.c_int
    L.dd3d_last_error.restype = C.c_char_p
    L.dd3d_arch.restype = C.c_char_p
    if hasattr(L, "dd3d_build_flags"):
        L.dd3d_build_flags.restype = C.c_char_p
    L.dd3d_conv_tile_shape.argtypes = [C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.dd3d_conv_row_rings.argtypes = [C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.dd3d_conv2d_igemm_f32.argtypes = [C.POINTER(ConvLaunch), C.c_void_p]
    L.dd3d_preprocess_u8_nhwc4.argtypes = [
        C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_float),
        C.c_void_p
    ]
    L.dd3d_maxpool2x2_nhwc.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int32] * 6 + [C.c_void_p]
    L.dd3d_upsample2x_add_nhwc.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int32] * 6 + [C.c_void_p]
    L.dd3d_maxpool3x3s2_ceil_nhwc.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int32] * 6 + [C.c_void_p]
    L.dd3d_ese_nhwc.argtypes = [C.c_void_p] * 7 + [C.c_int32] * 7 + [C.c_void_p]
    L.dd3d_fcos_select_decode.argtypes = [C.POINTER(SelectArgs), C.c_void_p]
    L.dd3d_invert_intrinsics.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    L.dd3d_nms_finalize.argtypes = [C.POINTER(NmsArgs), C.c_void_p]
    L.dd3d_bev_nms_aggregate.argtypes = [C.POINTER(BevArgs), C.c_void_p]
    L.dd3d_conv2d_smallc_supported.argtypes = [C.c_int32] * 6
    L.dd3d_conv2d_smallc_bf16x3.argtypes = [C.POINTER(SmallcArgs), C.c_void_p]
    L.dd3d_stem_fused_f16x2.argtypes = [C.POINTER(StemArgs), C.c_void_p]
    L.dd3d_stem_fused_keep_f16x2.argtypes = [C.POINTER(StemKeepArgs), C.c_void_p]
    L.dd3d_fold_range_flags.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_void_p, C.c_void_p]
    L.dd3d_pack_readback.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p]
    L.dd3d_rotate_iou_eval.argtypes = [C.c_void_p] * 3 + [C.c_int32] * 3 + [C.c_void_p]
    L.dd3d_d3_box_overlap.argtypes = [C.c_void_p] * 3 + [C.c_int32] * 4 + [C.c_void_p]
    L.dd3d_image_box_overlap.argtypes = [C.c_void_p] * 3 + [C.c_int32] * 3 + [C.c_void_p]
    L.dd3d_aligned_bilinear_scale.argtypes = [C.c_void_p] * 3 + [C.c_int32] * 6 + [C.c_float, C.c_void_p]
    L.dd3d_resize_bilinear_u8.argtypes = [C.POINTER(ResizeArgs), C.c_void_p]
    L.dd3d_format_boxes3d.argtypes = [C.c_void_p] * 4 + [C.c_int32, C.c_void_p]
    L.dd3d_math_planes.argtypes = [C.c_int32]
    L.dd3d_maxpool2x2_planes.argtypes = [C.c_void_p] * 3 + [C.c_int32] * 7 + [C.c_float, C.c_void_p, C.c_void_p]
    L.dd3d_maxpool2x2_planes_in.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int32] * 5 + [C.c_void_p]
    L.dd3d_upsample2x_add_planes.argtypes = [C.c_void_p] * 3 + [C.c_int32] * 7 + [C.c_float, C.c_void_p, C.c_void_p]
    L.dd3d_ese_fused.argtypes = [C.c_void_p] * 9 + [C.c_int32] * 8 + [C.c_float, C.c_void_p, C.c_void_p]
    L.dd3d_split_planes.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int32] * 5 + [C.c_float, C.c_void_p, C.c_void_p]
    L.dd3d_kitti_tp_scores.argtypes = [C.POINTER(KittiMatchArgs), C.c_void_p, C.c_void_p]
    L.dd3d_kitti_pr_counts.argtypes = [C.POINTER(KittiMatchArgs), C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    L.dd3d_nusc_center_match.argtypes = [C.POINTER(NuscMatchArgs), C.c_void_p, C.c_void_p]
    L.dd3d_loss_assign.argtypes = [C.POINTER(LossArgs), C.c_void_p]
    L.dd3d_loss_terms.argtypes = [C.POINTER(LossArgs), C.c_void_p]
    L.dd3d_loss_layout.argtypes = [C.c_void_p, C.c_int32]
    L.dd3d_loss_backward.argtypes = [C.POINTER(LossArgs), C.POINTER(LossGradArgs), C.c_void_p]
    L.dd3d_loss_grad_layout.argtypes = [C.c_void_p, C.c_int32]
    L.dd3d_dense_depth_loss.argtypes = [C.POINTER(DenseDepthLossArgs), C.c_void_p]
    L.dd3d_dense_depth_loss_layout.argtypes = [C.c_void_p, C.c_int32]
    L.dd3d_dense_depth_loss_backward.argtypes = [C.POINTER(DenseDepthLossArgs), C.POINTER(DenseDepthGradArgs), C.c_void_p]
    L.dd3d_dense_depth_grad_rows.argtypes = [C.POINTER(DenseDepthLossArgs)]
    L.dd3d_dense_depth_grad_rows.restype = C.c_int64
    L.dd3d_dense_depth_grad_layout.argtypes = [C.c_void_p, C.c_int32]
    L.dd3d_predictor_wgrad.argtypes = [C.POINTER(PredGradArgs), C.c_void_p]
    L.dd3d_predictor_dgrad.argtypes = [C.POINTER(PredGradArgs), C.c_void_p]
    L.dd3d_predictor_grad_slices.argtypes = [C.POINTER(PredGradArgs)]
    L.dd3d_predictor_grad_slices.restype = C.c_int64
    L.dd3d_pred_grad_layout.argtypes = [C.c_void_p, C.c_int32]
    L.dd3d_tower_wgrad.argtypes = [C.POINTER(TowerGradArgs), C.c_void_p]
    L.dd3d_tower_dgrad.argtypes = [C.POINTER(TowerGradArgs), C.c_void_p]
    L.dd3d_tower_grad_slices.argtypes = [C.POINTER(TowerGradArgs)]
    L.dd3d_tower_grad_slices.restype = C.c_int64
    L.dd3d_tower_grad_layout.argtypes = [C.c_void_p, C.c_int32]
    L.dd3d_fpn_wgrad.argtypes = [C.POINTER(FpnGradArgs), C.c_void_p]
    L.dd3d_fpn_dgrad.argtypes = [C.POINTER(FpnGradArgs), C.c_void_p]
    L.dd3d_fpn_grad_slices.argtypes = [C.POINTER(FpnGradArgs)]
    L.dd3d_fpn_grad_slices.restype = C.c_int64
    L.dd3d_fpn_grad_layout.argtypes = [C.c_void_p, C.c_int32]
    L.dd3d_backbone_wgrad.argtypes = [C.POINTER(BackboneGradArgs), C.c_void_p]
    L.dd3d_backbone_dgrad.argtypes = [C.POINTER(BackboneGradArgs), C.c_void_p]
    L.dd3d_backbone_grad_slices.argtypes = [C.POINTER(BackboneGradArgs)]
    L.dd3d_backbone_grad_slices.restype = C.c_int64
    L.dd3d_maxpool2x2_backward.argtypes = [C.POINTER(PoolGradArgs), C.c_void_p]
    L.dd3d_backbone_grad_layout.argtypes = [C.c_void_p, C.c_int32]
    L.dd3d_stem_wgrad.argtypes = [C.POINTER(StemGradArgs), C.c_void_p]
    L.dd3d_stem_dgrad.argtypes = [C.POINTER(StemGradArgs), C.c_void_p]
    L.dd3d_stem_grad_slices.argtypes = [C.POINTER(StemGradArgs)]
    L.dd3d_stem_grad_slices.restype = C.c_int64
    L.dd3d_stem_grad_layout.argtypes = [C.c_void_p, C.c_int32]
    L.dd3d_vovnet_stem_wgrad.argtypes = [C.POINTER(StemGradArgs), C.c_void_p]
    L.dd3d_vovnet_stem_grad_slices.argtypes = [C.POINTER(StemGradArgs)]
    L.dd3d_vovnet_stem_grad_slices.restype = C.c_int64
    L.dd3d_vovnet_conv_wgrad.argtypes = [C.POINTER(BackboneGradArgs), C.c_void_p]
    L.dd3d_vovnet_conv_dgrad.argtypes = [C.POINTER(BackboneGradArgs), C.c_void_p]
    L.dd3d_vovnet_conv_grad_slices.argtypes = [C.POINTER(BackboneGradArgs)]
    L.dd3d_vovnet_add.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_int32] * 4 + [C.c_void_p]
    L.dd3d_vovnet_conv_grad_slices.restype = C.c_int64
    L.dd3d_ese_backward.argtypes = [C.POINTER(EseGradArgs), C.c_void_p]
    L.dd3d_maxpool3x3s2_ceil_backward.argtypes = [C.POINTER(Pool3GradArgs), C.c_void_p]
    L.dd3d_vovnet_grad_layout.argtypes = [C.c_void_p, C.c_int32]
    for name in ("dd3d_bn_batch_stats", "dd3d_bn_apply_relu_split", "dd3d_bn_backward_reduce", "dd3d_bn_backward_apply"):
        getattr(L, name).argtypes = [C.POINTER(TowerBnArgs), C.c_void_p]
    L.dd3d_bn_slices.argtypes = [C.POINTER(TowerBnArgs)]
    L.dd3d_bn_slices.restype = C.c_int64
    L.dd3d_tower_bn_layout.argtypes = [C.c_void_p, C.c_int32]
    L.dd3d_bn_apply_topdown_split.argtypes = [C.POINTER(FpnBnArgs), C.c_void_p]
    for name in ("dd3d_bn_backward_reduce_linear", "dd3d_bn_backward_apply_linear"):
        getattr(L, name).argtypes = [C.POINTER(TowerBnArgs), C.c_void_p]
    L.dd3d_fpn_bn_layout.argtypes = [C.c_void_p, C.c_int32]
    for name in ("dd3d_backbone_bn_batch_stats", "dd3d_backbone_bn_backward_reduce", "dd3d_backbone_bn_backward_apply",
                 "dd3d_backbone_bn_backward_reduce_linear", "dd3d_backbone_bn_backward_apply_linear"):
        getattr(L, name).argtypes = [C.POINTER(TowerBnArgs), C.c_void_p]
    L.dd3d_backbone_bn_apply.argtypes = [C.POINTER(BackboneBnArgs), C.c_void_p]
    L.dd3d_backbone_bn_slices.argtypes = [C.POINTER(TowerBnArgs)]
    L.dd3d_backbone_bn_slices.restype = C.c_int64
    L.dd3d_backbone_bn_layout.argtypes = [C.c_void_p, C.c_int32]
    for name in EXPORTS:
        getattr(L, name)  # AttributeError if the .so is stale
    assert L.dd3d_abi_version() == ABI_VERSION, "libdd3d_hip.so ABI version mismatch; rebuild"
    # A library compiled with build-time knobs (-DDD3D_...: ring depths, schedules, store forms -- A/B variants of tests/tools) says so;
    # it is only accepted when the caller chose it (DD3D_HIP_LIB names it, or DD3D_ALLOW_VARIANT_LIB=1), never as the default library.
    flags = L.dd3d_build_flags().decode()
    if flags and not (os.environ.get("DD3D_HIP_LIB") or os.environ.get("DD3D_ALLOW_VARIANT_LIB") == "1"):
        raise HipLibraryMissing(f"{_LIB_PATH} was built with non-default knobs ({flags}): rebuild it with __graft_entry__.build(force=True), "
                                "or select a variant explicitly with DD3D_HIP_LIB / DD3D_ALLOW_VARIANT_LIB=1")
    _lib = L
    return L


def check(rc, what=""):
    if rc != 0:
        raise RuntimeError(f"libdd3d_hip {what} failed (rc={rc}): {lib().dd3d_last_error().decode()}")


def current_stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
