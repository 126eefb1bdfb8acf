"""ctypes binding of libmcamd.so (include/mcamd.h).

The product path has no CPU or PyTorch fallback: if the HIP library cannot be
loaded this raises, and every wrapper raises `McamdError` on a non-zero return.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmcamd.so")


class McamdError(RuntimeError):
    pass


class ConvGeom(C.Structure):
    _fields_ = [("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("ksize", C.c_int32),
                ("cin", C.c_int32), ("cout", C.c_int32), ("x_ld", C.c_int32), ("x_choff", C.c_int32),
                ("stem", C.c_int32), ("pad", C.c_int32), ("x_wrap", C.c_int32), ("x_f8", C.c_int32), ("x_f8_wexp", C.c_int32)]


class ConvEpilogue(C.Structure):
    _fields_ = [("mode", C.c_int32), ("y_ld", C.c_int32), ("y_choff", C.c_int32),
                ("y", C.c_void_p), ("bias", C.c_void_p), ("stats", C.c_void_p),
                ("stats_rows", C.c_int32), ("stats_ld", C.c_int32),
                ("scale", C.c_void_p), ("shift", C.c_void_p), ("slope", C.c_float), ("overflow", C.c_void_p),
                ("dst_mode", C.c_int32), ("y2", C.c_void_p), ("y2_ld", C.c_int32), ("y2_choff", C.c_int32),
                ("concurrent", C.c_int32)]


class ActDesc(C.Structure):
    _fields_ = [("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32),
                ("y", C.c_void_p), ("y_ld", C.c_int32), ("y_choff", C.c_int32),
                ("scale", C.c_void_p), ("shift", C.c_void_p), ("slope", C.c_float), ("mode", C.c_int32),
                ("dst", C.c_void_p), ("dst_ld", C.c_int32), ("dst_choff", C.c_int32),
                ("dst2", C.c_void_p), ("dst2_ld", C.c_int32), ("dst2_choff", C.c_int32),
                ("y_dtype", C.c_int32), ("planes", C.c_int32), ("dst_plane", C.c_int32), ("dst2_plane", C.c_int32),
                ("dst_pad", C.c_int32), ("dst2_pad", C.c_int32), ("border", C.c_void_p), ("planes2", C.c_int32),
                ("pool_act", C.c_void_p), ("pool_act_ld", C.c_int32), ("pool_act_pad", C.c_int32),
                ("dst_q8", C.c_void_p), ("dst2_q8", C.c_void_p)]


class ChanMap(C.Structure):
    _fields_ = [("rows", C.c_void_p), ("cols", C.c_void_p)]


class PackJob(C.Structure):
    _fields_ = [("w", C.c_void_p), ("mask", C.c_void_p), ("dst_fwd", C.c_void_p), ("dst_dgrad", C.c_void_p),
                ("rows", C.c_void_p), ("cols", C.c_void_p),
                ("first_tile", C.c_int64), ("cout", C.c_int32), ("cin", C.c_int32), ("ksize", C.c_int32),
                ("split", C.c_int32), ("f8_wexp", C.c_int32)]


class ActBwdDesc(C.Structure):
    _fields_ = [("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32),
                ("y", C.c_void_p), ("y_ld", C.c_int32), ("y_choff", C.c_int32),
                ("scale", C.c_void_p), ("shift", C.c_void_p), ("mean", C.c_void_p), ("invstd", C.c_void_p),
                ("slope", C.c_float), ("mode", C.c_int32),
                ("g", C.c_void_p), ("g_ld", C.c_int32), ("g_choff", C.c_int32),
                ("g2", C.c_void_p), ("g2_ld", C.c_int32), ("g2_choff", C.c_int32),
                ("dy", C.c_void_p), ("dy_ld", C.c_int32), ("dy_choff", C.c_int32),
                ("dgamma", C.c_void_p), ("dbeta", C.c_void_p), ("grad_scale", C.c_float),
                ("dy_keep", C.c_void_p), ("chan_perm", C.c_void_p), ("y_dtype", C.c_int32),
                ("overflow", C.c_void_p), ("dy_pad", C.c_int32), ("skip_dead_param_grads", C.c_int32),
                ("act", C.c_void_p), ("act_ld", C.c_int32), ("act_choff", C.c_int32), ("act_pad", C.c_int32),
                ("pool_out", C.c_void_p), ("pool_out_ld", C.c_int32), ("pool_out_choff", C.c_int32),
                ("pool_out_pad", C.c_int32),
                ("sums", C.c_void_p), ("sums_rows", C.c_int32), ("sums_ld", C.c_int32)]


class DgradSums(C.Structure):
    """mcamd_dgrad_sums (include/mcamd.h)."""
    _fields_ = [("slab", C.c_void_p), ("rows", C.c_int32), ("ld", C.c_int32),
                ("act", C.c_void_p), ("act_ld", C.c_int32), ("act_choff", C.c_int32), ("act_pad", C.c_int32),
                ("scale", C.c_void_p), ("shift", C.c_void_p), ("mean", C.c_void_p), ("invstd", C.c_void_p),
                ("slope", C.c_float), ("y", C.c_void_p), ("y_ld", C.c_int32), ("y_choff", C.c_int32),
                ("ch_lo", C.c_int32), ("C", C.c_int32)]


class BnConv1x1Instance(C.Structure):
    """mcamd_bn_conv1x1_instance (include/mcamd.h)."""
    _fields_ = [(n, C.c_int32) for n in ("bn", "cb", "threads", "rows", "num_mtiles", "grid", "lds_bytes")]


class ActInstance(C.Structure):
    """mcamd_act_instance (include/mcamd.h)."""
    _fields_ = [("mode", C.c_int32), ("fixed", C.c_int32), ("y32", C.c_int32), ("planes", C.c_int32),
                ("planes2", C.c_int32), ("q8", C.c_int32), ("items", C.c_int64), ("grid", C.c_int32)]


class SplitkInfo(C.Structure):
    """mcamd_splitk_info (include/mcamd.h)."""
    _fields_ = [("slices", C.c_int32), ("bm", C.c_int32), ("bn", C.c_int32), ("bk", C.c_int32),
                ("chunks", C.c_int32), ("tiles", C.c_int32), ("workspace_bytes", C.c_int64),
                ("stages", C.c_int32), ("mtiles", C.c_int32), ("ntiles", C.c_int32),
                ("finish_rows", C.c_int32), ("finish_cols", C.c_int32)]


class FoldDesc(C.Structure):
    _fields_ = [("w", C.c_void_p), ("mask", C.c_void_p), ("rows", C.c_void_p), ("cols", C.c_void_p),
                ("beta", C.c_void_p), ("slope", C.c_float),
                ("n", C.c_int32), ("cin_t", C.c_int32), ("cin_k", C.c_int32), ("cin_aug", C.c_int32), ("ksize", C.c_int32)]


class StemBlockDesc(C.Structure):
    _fields_ = [("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("x", C.c_void_p), ("wp", C.c_void_p), ("gamma", C.c_void_p), ("beta", C.c_void_p),
                ("running_mean", C.c_void_p), ("running_var", C.c_void_p),
                ("momentum", C.c_float), ("eps", C.c_float), ("training", C.c_int32),
                ("scale", C.c_void_p), ("shift", C.c_void_p), ("save_mean", C.c_void_p), ("save_invstd", C.c_void_p),
                ("slope", C.c_float),
                ("dst", C.c_void_p), ("dst_ld", C.c_int32), ("dst_choff", C.c_int32),
                ("g", C.c_void_p), ("g_ld", C.c_int32), ("g_choff", C.c_int32),
                ("mask", C.c_void_p), ("grad_scale", C.c_float),
                ("dw", C.c_void_p), ("dgamma", C.c_void_p), ("dbeta", C.c_void_p), ("cout", C.c_int32), ("planes", C.c_int32),
                ("x_lo", C.c_void_p), ("wp_lo", C.c_void_p)]


class RegionDesc(C.Structure):
    _fields_ = [("output", C.c_void_p), ("target", C.c_void_p),
                ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("num_anchors", C.c_int32), ("num_classes", C.c_int32),
                ("max_boxes", C.c_int32), ("anchors", C.c_float * 16),
                ("coord_scale", C.c_float), ("noobject_scale", C.c_float), ("object_scale", C.c_float),
                ("class_scale", C.c_float), ("thresh", C.c_float)]


class DistillDesc(C.Structure):
    """mcamd_distill_desc (include/mcamd.h)."""
    _fields_ = [("student", C.c_void_p), ("teacher", C.c_void_p),
                ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("num_anchors", C.c_int32), ("num_classes", C.c_int32),
                ("obj_scale", C.c_float), ("box_scale", C.c_float), ("cls_scale", C.c_float), ("temperature", C.c_float)]


class DetectDesc(C.Structure):
    """mcamd_detect_desc (include/mcamd.h)."""
    _fields_ = [("output", C.c_void_p),
                ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("num_anchors", C.c_int32), ("num_classes", C.c_int32),
                ("anchors", C.c_float * 16), ("conf_thresh", C.c_float), ("nms_thresh", C.c_float)]


class VocMatchDesc(C.Structure):
    """mcamd_voc_match_desc (include/mcamd.h)."""
    _fields_ = [("rows", C.c_void_p), ("probs", C.c_void_p), ("nkept", C.c_void_p),
                ("B", C.c_int32), ("N", C.c_int32), ("C", C.c_int32), ("G", C.c_int32),
                ("conf_thresh", C.c_float), ("first_image", C.c_int32), ("ovthresh", C.c_double),
                ("gt_box", C.c_void_p), ("gt_cls", C.c_void_p), ("gt_difficult", C.c_void_p), ("gt_count", C.c_void_p),
                ("image_size", C.c_void_p),
                ("keys", C.c_void_p), ("flags", C.c_void_p), ("capacity", C.c_int64), ("counters", C.c_void_p)]


class FoldJob(C.Structure):
    _fields_ = [("d", FoldDesc), ("waug", C.c_void_p), ("first_block", C.c_int64)]


class AugmentDesc(C.Structure):
    """mcamd_augment_desc (include/mcamd.h)."""
    _fields_ = [("src_off", C.c_int64), ("tmp_off", C.c_int64),
                ("src_w", C.c_int32), ("src_h", C.c_int32), ("crop_x", C.c_int32), ("crop_y", C.c_int32),
                ("crop_w", C.c_int32), ("crop_h", C.c_int32), ("flip", C.c_int32),
                ("hk", C.c_int32), ("vk", C.c_int32), ("hcoef_off", C.c_int32), ("vcoef_off", C.c_int32),
                ("lut_off", C.c_int32)]


class AugmentBatch(C.Structure):
    """mcamd_augment_batch (include/mcamd.h)."""
    _fields_ = [("desc", C.c_void_p), ("desc_dev", C.c_void_p),
                ("src", C.c_void_p), ("src_bytes", C.c_int64),
                ("coef", C.c_void_p), ("coef_elems", C.c_int64),
                ("lut", C.c_void_p), ("lut_bytes", C.c_int64),
                ("tmp", C.c_void_p), ("tmp_bytes", C.c_int64),
                ("out", C.c_void_p), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32)]


class WzSeg(C.Structure):
    """mcamd_wz_seg (include/mcamd.h)."""
    _fields_ = [("w", C.c_void_p), ("mask", C.c_void_p), ("n", C.c_int64), ("word0", C.c_int64), ("val0", C.c_int64),
                ("kept", C.c_int64), ("cout", C.c_int32), ("kind", C.c_int32), ("exp0", C.c_int32), ("dense", C.c_int32),
                ("block0", C.c_int32), ("shift0", C.c_int32)]


class HzSeg(C.Structure):
    """mcamd_hz_seg (include/mcamd.h)."""
    _fields_ = [("sym0", C.c_int64), ("nsym", C.c_int64), ("nbits", C.c_int64), ("word0", C.c_int64), ("chunk0", C.c_int64),
                ("popc_bits", C.c_int64), ("block0", C.c_int32), ("A", C.c_int32)]


class WsSeg(C.Structure):
    """mcamd_ws_seg (include/mcamd.h)."""
    _fields_ = [("w", C.c_void_p), ("mask", C.c_void_p), ("codes", C.c_void_p), ("n", C.c_int64), ("part0", C.c_int64),
                ("K", C.c_int32), ("cb0", C.c_int32), ("slab0", C.c_int32), ("reserved", C.c_int32)]


class TaylorSeg(C.Structure):
    """mcamd_taylor_seg (include/mcamd.h)."""
    _fields_ = [("w", C.c_void_p), ("g", C.c_void_p), ("bias", C.c_void_p), ("gbias", C.c_void_p), ("acc_w", C.c_void_p),
                ("acc_b", C.c_void_p), ("acc_f", C.c_void_p), ("wg0", C.c_int64), ("kind", C.c_int32), ("cout", C.c_int32),
                ("cin", C.c_int32), ("khw", C.c_int32)]


class GproxSeg(C.Structure):
    """mcamd_gprox_seg (include/mcamd.h)."""
    _fields_ = [("w", C.c_void_p), ("nz", C.c_void_p), ("wg0", C.c_int64), ("kind", C.c_int32), ("cout", C.c_int32),
                ("cin", C.c_int32), ("khw", C.c_int32)]


EPI_RAW_F16, EPI_NCHW_F32, EPI_PAD_F16, EPI_RAW_F32 = 0, 1, 2, 3
DST_PLAIN, DST_POOL, DST_REORG = 0, 1, 2
WGRAD_GENERIC, WGRAD_STEM, WGRAD_WIN, WGRAD_NINE, WGRAD_NINE_WIDE = 0, 1, 2, 3, 4      # mcamd_conv_wgrad_plan_info: family
WFIN_ROW, WFIN_VEC, WFIN_GENERIC = 0, 1, 2                                             # ... and finish kernel
WGRAD_PLAN_INFO_N = 13
WGRAD_BSPARSE_PLAN_N = 8                                                               # mcamd_conv_wgrad_bsparse_plan
STEM_PLAN_FWD, STEM_PLAN_FWD_PLANES, STEM_PLAN_STATS, STEM_PLAN_GRAM, STEM_PLAN_BWD = 0, 1, 2, 3, 4    # mcamd_stem_block_plan_info
STEM_PLAN_INFO_N = 20
WZ_FP32, WZ_FP16, WZ_FP8, WZ_CODE, WZ_W4 = 0, 1, 2, 4, 5                               # mcamd_wz_seg.kind (WZ_W4: | taps << 8)
WZ_F_BN, WZ_F_BITS = 1, 2                                                              # record flags of a .mcz file
WZ_BLOCK_WORDS = 64
HZ_MAXLEN, HZ_CHUNK, HZ_GROUP = 12, 1024, 64                                            # MCAMD_HZ_*
WS_SLAB = 4096                                                                         # MCAMD_WS_SLAB
TAYLOR_CONV, TAYLOR_GATE = 0, 1                                                        # mcamd_taylor_seg.kind
GPROX_BLOCK, GPROX_GATE = 0, 1                                                         # mcamd_gprox_seg.kind

# name -> (restype, argtypes); the complete list of symbols include/mcamd.h declares.
_P, _I32, _I64, _F, _SZ = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_size_t
SIGNATURES = {
    "mcamd_version": (C.c_int, []),
    "mcamd_arch": (C.c_char_p, []),
    "mcamd_last_error": (C.c_char_p, []),
    "mcamd_reload_config": (None, []),
    "mcamd_conv_stats_rows": (_I32, [C.POINTER(ConvGeom)]),
    "mcamd_conv_stats_rows_mode": (_I32, [C.POINTER(ConvGeom), _I32]),
    "mcamd_conv_fwd_f8_ok": (_I32, [C.POINTER(ConvGeom)]),
    "mcamd_conv_tile_info": (C.c_int, [C.POINTER(ConvGeom), _I32, C.POINTER(_I32)]),
    "mcamd_conv_route_info": (C.c_int, [C.POINTER(ConvGeom), _I32, _I32, _I32, _I32, C.POINTER(_I32)]),
    "mcamd_packed_elems_fwd": (_I64, [C.POINTER(ConvGeom)]),
    "mcamd_packed_elems_dgrad": (_I64, [C.POINTER(ConvGeom)]),
    "mcamd_pack_weights": (C.c_int, [C.POINTER(ConvGeom), _P, _P, C.POINTER(ChanMap), _P, _P, _P]),
    "mcamd_pack_weights_many": (C.c_int, [_P, _I32, _I64, _P]),
    "mcamd_conv_fwd": (C.c_int, [C.POINTER(ConvGeom), _P, _P, C.POINTER(ConvEpilogue), _P]),
    "mcamd_conv_fwd_sparse24_ok": (_I32, [C.POINTER(ConvGeom)]),
    "mcamd_sparse24_elems": (C.c_int, [C.POINTER(ConvGeom), C.POINTER(_I64)]),
    "mcamd_conv_fwd_sparse24_info": (C.c_int, [C.POINTER(ConvGeom), C.POINTER(_I32)]),
    "mcamd_pack_sparse24": (C.c_int, [C.POINTER(ConvGeom), _P, _P, _P, _P, _P]),
    "mcamd_conv_fwd_sparse24": (C.c_int, [C.POINTER(ConvGeom), _P, _P, _P, C.POINTER(ConvEpilogue), _P]),
    "mcamd_conv_fwd_bsparse_ok": (_I32, [C.POINTER(ConvGeom)]),
    "mcamd_bsparse_elems": (C.c_int, [C.POINTER(ConvGeom), C.POINTER(_I64)]),
    "mcamd_bsparse_lists": (C.c_int, [C.POINTER(ConvGeom), _P, _P, _P, _P]),
    "mcamd_conv_fwd_bsparse": (C.c_int, [C.POINTER(ConvGeom), _P, _P, _P, _P, C.POINTER(ConvEpilogue), _P]),
    "mcamd_conv_fwd_bsparse_info": (C.c_int, [C.POINTER(ConvGeom), C.POINTER(_I32)]),
    "mcamd_conv_bsparse_train_ok": (_I32, [C.POINTER(ConvGeom), _I32]),
    "mcamd_conv_bsparse_train_info": (C.c_int, [C.POINTER(ConvGeom), _I32, C.POINTER(_I32)]),
    "mcamd_conv_bsparse_raw_stats_rows": (_I32, [C.POINTER(ConvGeom), _I32]),
    "mcamd_bsparse_elems_dgrad": (C.c_int, [C.POINTER(ConvGeom), C.POINTER(_I64)]),
    "mcamd_bsparse_lists_dgrad": (C.c_int, [C.POINTER(ConvGeom), _P, _P, _P, _P]),
    "mcamd_conv_fwd_bsparse_raw": (C.c_int, [C.POINTER(ConvGeom), _P, _P, _P, _P, C.POINTER(ConvEpilogue), _P]),
    "mcamd_conv_dgrad_bsparse": (C.c_int, [C.POINTER(ConvGeom), _P, _I32, _I32, _P, _P, _P, C.POINTER(ConvEpilogue), _P]),
    "mcamd_conv_fwd_splitk_info": (C.c_int, [C.POINTER(ConvGeom), _I32, _I32, _I32, C.POINTER(SplitkInfo)]),
    "mcamd_conv_fwd_splitk": (C.c_int, [C.POINTER(ConvGeom), _P, _P, C.POINTER(ConvEpilogue), _I32, _P, _SZ, _P]),
    "mcamd_conv_fwd_q8_ok": (_I32, [C.POINTER(ConvGeom)]),
    "mcamd_q8_elems": (C.c_int, [C.POINTER(ConvGeom), C.POINTER(_I64)]),
    "mcamd_pack_q8": (C.c_int, [C.POINTER(ConvGeom), _P, _P, _P, _P, _P]),
    "mcamd_conv_fwd_q8": (C.c_int, [C.POINTER(ConvGeom), _P, _P, _P, C.POINTER(ConvEpilogue), _I32, _I32, _P]),
    "mcamd_conv_fwd_q8_info": (C.c_int, [C.POINTER(ConvGeom), _I32, C.POINTER(_I32)]),
    "mcamd_conv_fwd_q8_splitk_info": (C.c_int, [C.POINTER(ConvGeom), _I32, _I32, C.POINTER(SplitkInfo)]),
    "mcamd_conv_fwd_q8_splitk": (C.c_int, [C.POINTER(ConvGeom), _P, _P, _P, C.POINTER(ConvEpilogue), _I32, _I32, _I32, _P, _SZ, _P]),
    "mcamd_conv_fwd_q8_bsparse_ok": (_I32, [C.POINTER(ConvGeom)]),
    "mcamd_q8_bsparse_elems": (C.c_int, [C.POINTER(ConvGeom), C.POINTER(_I64)]),
    "mcamd_q8_bsparse_lists": (C.c_int, [C.POINTER(ConvGeom), _P, _P, _P, _P]),
    "mcamd_conv_fwd_q8_bsparse": (C.c_int, [C.POINTER(ConvGeom), _P, _P, _P, _P, _P, C.POINTER(ConvEpilogue), _I32, _I32, _P]),
    "mcamd_conv_fwd_q8_bsparse_info": (C.c_int, [C.POINTER(ConvGeom), C.POINTER(_I32)]),
    "mcamd_conv_fwd_q8_slim_ok": (_I32, [C.POINTER(ConvGeom)]),
    "mcamd_q8_slim_elems": (C.c_int, [C.POINTER(ConvGeom), C.POINTER(_I64)]),
    "mcamd_pack_q8_slim": (C.c_int, [C.POINTER(ConvGeom), _P, _P, _P, _P, _P]),
    "mcamd_conv_fwd_q8_slim": (C.c_int, [C.POINTER(ConvGeom), _P, _P, _P, C.POINTER(ConvEpilogue), _P, _I32, _I32, _I32, _P]),
    "mcamd_conv_fwd_q8_sparse24_ok": (_I32, [C.POINTER(ConvGeom)]),
    "mcamd_q8_sparse24_elems": (C.c_int, [C.POINTER(ConvGeom), C.POINTER(_I64)]),
    "mcamd_pack_q8_sparse24": (C.c_int, [C.POINTER(ConvGeom), _P, _P, _P, _P, _P, _P]),
    "mcamd_conv_fwd_q8_sparse24": (C.c_int, [C.POINTER(ConvGeom), _P, _P, _P, _P, C.POINTER(ConvEpilogue), _I32, _I32, _P]),
    "mcamd_conv_fwd_q8_w4_ok": (_I32, [C.POINTER(ConvGeom)]),
    "mcamd_q8_w4_elems": (C.c_int, [C.POINTER(ConvGeom), C.POINTER(_I64)]),
    "mcamd_pack_q8_w4": (C.c_int, [C.POINTER(ConvGeom), _P, _P, _P, _P, _P, _P]),
    "mcamd_unpack_q8_w4": (C.c_int, [C.POINTER(ConvGeom), _P, _P, _P, _P]),
    "mcamd_conv_fwd_q8_w4": (C.c_int, [C.POINTER(ConvGeom), _P, _P, _P, _P, C.POINTER(ConvEpilogue), _I32, _I32, _P]),
    "mcamd_conv_fwd_q8_w4_info": (C.c_int, [C.POINTER(ConvGeom), C.POINTER(_I32)]),
    "mcamd_conv_fwd_q8_w4_raw": (C.c_int, [C.POINTER(ConvGeom), _P, _P, _P, _P, C.POINTER(ConvEpilogue), _P]),
    "mcamd_fakequant_q8_w4": (C.c_int, [C.POINTER(ConvGeom), _P, _P, _P, _P, _P]),
    "mcamd_cast_q8": (C.c_int, [_P, _I64, _I32, _I32, _I32, _P, _I32, _I32, _P]),
    "mcamd_conv_fwd_q8_stats_rows": (_I32, [C.POINTER(ConvGeom)]),
    "mcamd_fakequant_q8": (C.c_int, [C.POINTER(ConvGeom), _P, _P, _P, _P, _P]),
    "mcamd_cast_q8_train": (C.c_int, [_P, _I64, _I32, _I32, _I32, _P, _I32, _I32, _P]),
    "mcamd_conv_dgrad": (C.c_int, [C.POINTER(ConvGeom), _P, _I32, _I32, _P, C.POINTER(ConvEpilogue), _P]),
    "mcamd_conv_dgrad_sums_rows": (_I32, [C.POINTER(ConvGeom), _I32]),
    "mcamd_conv_dgrad_sums": (C.c_int, [C.POINTER(ConvGeom), _P, _I32, _I32, _P, C.POINTER(ConvEpilogue), C.POINTER(DgradSums), _P]),
    "mcamd_conv_wgrad_workspace_bytes": (_SZ, [C.POINTER(ConvGeom)]),
    "mcamd_conv_wgrad": (C.c_int, [C.POINTER(ConvGeom), _P, _P, _I32, _I32, _P, C.POINTER(ChanMap), _F, _P, _P, _P, _SZ, _P]),
    "mcamd_conv_wgrad_plan_info": (C.c_int, [C.POINTER(ConvGeom), _I32, C.POINTER(_I32)]),
    "mcamd_wgrad_generic_instances": (_I32, [C.POINTER(_I32), _I32]),
    "mcamd_conv_wgrad_bsparse_ok": (_I32, [C.POINTER(ConvGeom)]),
    "mcamd_wgrad_bsparse_elems": (C.c_int, [C.POINTER(ConvGeom), C.POINTER(_I64)]),
    "mcamd_wgrad_bsparse_lists": (C.c_int, [C.POINTER(ConvGeom), _P, _P, _P, _P, _P]),
    "mcamd_conv_wgrad_bsparse_plan": (C.c_int, [C.POINTER(ConvGeom), _I32, C.POINTER(_I64)]),
    "mcamd_conv_wgrad_bsparse": (C.c_int, [C.POINTER(ConvGeom), _P, _P, _I32, _I32, _P, _P, _P, _I32, _I32, _F, _P, _P, _P, _SZ, _P]),
    "mcamd_conv_bwd1x1_ok": (_I32, [C.POINTER(ConvGeom), C.POINTER(C.c_char_p)]),
    "mcamd_conv_bwd1x1_sums_rows": (_I32, [C.POINTER(ConvGeom)]),
    "mcamd_conv_bwd1x1_wgrad_splits": (_I32, [C.POINTER(ConvGeom)]),
    "mcamd_conv_bwd1x1_workspace_bytes": (_SZ, [C.POINTER(ConvGeom)]),
    "mcamd_conv_bwd1x1": (C.c_int, [C.POINTER(ConvGeom), _P, _P, _I32, _I32, _P, _P, _I32, _I32, _P, C.POINTER(DgradSums), _P, _F,
                                    _P, _P, _P, _SZ, _P]),
    "mcamd_bn_coeffs": (C.c_int, [_P, _I32, _I32, _I32, _I64, _P, _P, _P, _P, _F, _F, _I32, _P, _P, _P, _P, _P, _P]),
    "mcamd_bn_coeffs_ex": (C.c_int, [_P, _I32, _I32, _I32, _I64, _P, _P, _P, _P, _F, _F, _I32, _P, _P, _P, _P, _P, _I32, _P]),
    "mcamd_fold_weights": (C.c_int, [C.POINTER(FoldDesc), _P, _P]),
    "mcamd_fold_weights_many": (C.c_int, [_P, _I32, _I64, _P]),
    "mcamd_unfold_wgrad": (C.c_int, [C.POINTER(FoldDesc), _P, _P, _P, _P, _I32, _P]),
    "mcamd_bn_act_fwd": (C.c_int, [C.POINTER(ActDesc), _P]),
    "mcamd_bn_act_fwd_instance": (C.c_int, [C.POINTER(ActDesc), C.POINTER(ActInstance)]),
    "mcamd_bn_act_conv1x1_ok": (_I32, [C.POINTER(ActDesc), C.POINTER(ConvGeom)]),
    "mcamd_bn_act_conv1x1_stats_rows": (_I32, [C.POINTER(ActDesc), C.POINTER(ConvGeom)]),
    "mcamd_bn_act_conv1x1_info": (C.c_int, [C.POINTER(ActDesc), C.POINTER(ConvGeom), C.POINTER(BnConv1x1Instance)]),
    "mcamd_bn_act_conv1x1_fwd": (C.c_int, [C.POINTER(ActDesc), C.POINTER(ConvGeom), _P, C.POINTER(ConvEpilogue), _P]),
    "mcamd_bn_act_bwd_workspace_bytes": (_SZ, [C.POINTER(ActBwdDesc)]),
    "mcamd_bn_act_bwd": (C.c_int, [C.POINTER(ActBwdDesc), _P, _SZ, _P]),
    "mcamd_stem_block_workspace_bytes": (_SZ, []),
    "mcamd_stem_block_fwd": (C.c_int, [C.POINTER(StemBlockDesc), _P, _SZ, _P]),
    "mcamd_stem_block_bwd": (C.c_int, [C.POINTER(StemBlockDesc), _P, _SZ, _P]),
    "mcamd_stem_block_stats_rows": (_I32, [C.POINTER(StemBlockDesc)]),
    "mcamd_stem_block_stats": (C.c_int, [C.POINTER(StemBlockDesc), _P, _I32, _I32, _P]),
    "mcamd_stem_block_plan_info": (C.c_int, [C.POINTER(StemBlockDesc), C.POINTER(_I32)]),
    "mcamd_nchw_f32_to_nhwc4_split": (C.c_int, [_P, _I32, _I32, _I32, _P, _P, _P]),
    "mcamd_pack_stem_split": (C.c_int, [_P, _P, _I32, _P, _P, _P]),
    "mcamd_nchw_f32_to_padded_nhwc_f16": (C.c_int, [_P, _I32, _I32, _I32, _I32, _F, _P, _I32, _I32, _P, _P]),
    "mcamd_nchw_f32_to_padded_nhwc_f16_pad": (C.c_int, [_P, _I32, _I32, _I32, _I32, _F, _P, _I32, _I32, _I32, _P, _P]),
    "mcamd_nchw_f32_to_padded_nhwc_f16_split": (C.c_int, [_P, _I32, _I32, _I32, _I32, _P, _I32, _I32, _I32, _P]),
    "mcamd_stem_conv_f32_stats_rows": (_I32, []),
    "mcamd_stem_conv_f32": (C.c_int, [_P, _I32, _I32, _I32, _P, _P, _I32, _P, _P, _I32, _P, _I32, _I32, _P]),
    "mcamd_region_loss_workspace_bytes": (_SZ, [_I32]),
    "mcamd_region_loss": (C.c_int, [C.POINTER(RegionDesc), _P, _P, _P, _P, _SZ, _P]),
    "mcamd_distill_loss_workspace_bytes": (_SZ, [_I32, _I32]),
    "mcamd_distill_loss": (C.c_int, [C.POINTER(DistillDesc), _P, _P, _P, _SZ, _P]),
    "mcamd_region_decode": (C.c_int, [C.POINTER(DetectDesc), _P, _P, _P]),
    "mcamd_nms": (C.c_int, [_P, _P, _I32, _I32, _F, _P, _P, _P]),
    "mcamd_detect": (C.c_int, [C.POINTER(DetectDesc), _P, _P, _P, _P, _P, _P]),
    "mcamd_voc_match": (C.c_int, [C.POINTER(VocMatchDesc), _P]),
    "mcamd_voc_ap": (C.c_int, [_P, _P, _P, _I64, _P, _I32, _P, _P, _P, _P]),
    "mcamd_augment": (C.c_int, [C.POINTER(AugmentBatch), _P]),
    "mcamd_augment_tables": (C.c_int, [_P, _P, _P, _I32, _I32, _I32, _P, _I64, _P, _I64, _P]),
    "mcamd_plan_begin": (C.c_int, [C.POINTER(_P), _I32]),
    "mcamd_plan_mark": (_I32, []),
    "mcamd_plan_end": (_P, []),
    "mcamd_plan_segments": (_I32, [_P]),
    "mcamd_plan_launches": (_I32, [_P]),
    "mcamd_plan_run": (C.c_int, [_P, _I32, _I32, C.POINTER(_P), _I32]),
    "mcamd_plan_destroy": (None, [_P]),
    "mcamd_stream_wait": (C.c_int, [_P, _P]),
    "mcamd_memset_zero": (C.c_int, [_P, _SZ, _P]),
    "mcamd_step_flags": (C.c_int, [_P, _I32, _P, _P, _P, _P, _P]),
    "mcamd_kth_magnitude_workspace_bytes": (_SZ, []),
    "mcamd_kth_magnitude": (C.c_int, [C.POINTER(_P), C.POINTER(_I64), _I32, _I64, _P, _P, _SZ, _P]),
    "mcamd_magnitude_mask": (C.c_int, [_P, _I64, _P, _P, _P]),
    "mcamd_filter_scores_workspace_bytes": (_SZ, [_I32]),
    "mcamd_filter_scores": (C.c_int, [_P, _I32, _I32, _I32, _I32, _P, _P, _SZ, _P]),
    "mcamd_filter_mean_square": (C.c_int, [_P, _I32, _I32, _I32, _I32, _P, _P, _SZ, _P]),
    "mcamd_filter_mask": (C.c_int, [_P, _I32, _I64, _P, _P]),
    "mcamd_count_zeros": (C.c_int, [_P, _I64, _P, _P]),
    "mcamd_masked_residual": (C.c_int, [_P, _P, _I64, _P, _P]),
    "mcamd_nm_mask": (C.c_int, [_P, _P, _I32, _I32, _I32, _I32, _I32, _P, _P]),
    "mcamd_nm_violations": (C.c_int, [_P, _I32, _I32, _I32, _P, _P]),
    "mcamd_block_scores": (C.c_int, [_P, _P, _I32, _I32, _I32, _P, _P]),
    "mcamd_block_mask": (C.c_int, [_P, _P, _I32, _I32, _I32, _P, _P]),
    "mcamd_wz_workspace_bytes": (_SZ, [_I64, _I32]),
    "mcamd_wz_pack": (C.c_int, [_P, _P, _I32, _P, _I64, _P, _P, _I64, _P, _I64, _P, _SZ, _P]),
    "mcamd_wz_unpack": (C.c_int, [_P, _P, _I32, _P, _I64, _P, _I64, _P, _I64, _P, _SZ, _P]),
    "mcamd_wz_pack_w4": (C.c_int, [_P, _P, _I32, _P, _I64, _P, _P, _I64, _P, _I64, _P, _SZ, _P, _P, _I64]),
    "mcamd_wz_unpack_w4": (C.c_int, [_P, _P, _I32, _P, _I64, _P, _I64, _P, _I64, _P, _SZ, _P, _P, _I64]),
    "mcamd_hz_workspace_bytes": (_SZ, [_I64, _I32]),
    "mcamd_hz_histogram": (C.c_int, [_P, _P, _I32, _P, _I64, _P, _P, _P, _SZ, _P]),
    "mcamd_hz_encode": (C.c_int, [_P, _P, _I32, _P, _I64, _P, _P, _I64, _P, _I64, _P, _SZ, _P]),
    "mcamd_hz_decode": (C.c_int, [_P, _P, _I32, _P, _P, _I64, _P, _I64, _P, _I64, _P, _P]),
    "mcamd_ws_workspace_bytes": (_SZ, [_I64, _I64, _I32]),
    "mcamd_ws_init": (C.c_int, [_P, _P, _I32, _P, _I64, _P, _SZ, _P]),
    "mcamd_ws_iterate": (C.c_int, [_P, _P, _I32, _P, _I64, _P, _P, _P, _SZ, _P]),
    "mcamd_ws_assign": (C.c_int, [_P, _P, _I32, _P, _I64, _P]),
    "mcamd_ws_project": (C.c_int, [_P, _P, _I32, _P, _I64, _P, _P, _P, _SZ, _P]),
    "mcamd_ws_expand": (C.c_int, [_P, _P, _I32, _P, _I64, _P]),
    "mcamd_taylor_seg_workgroups": (_I64, [C.POINTER(TaylorSeg)]),
    "mcamd_taylor_accum": (C.c_int, [_P, _P, _I32, _P, _P, _P]),
    "mcamd_gprox_seg_workgroups": (_I64, [C.POINTER(GproxSeg)]),
    "mcamd_group_prox": (C.c_int, [_P, _P, _I32, C.c_double, _F, _P, _P]),
}

_lib = None


def lib():
    """The loaded library; raises McamdError when it is absent (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise McamdError(
                "libmcamd.so is missing (%s). Build it with `python -m modelcompression_amd.build`; "
                "modelcompression_amd has no CPU/PyTorch fallback for its compute path." % LIB_PATH)
        # torch first: PyTorch-ROCm ships its own libamdhip64 and must be the HIP runtime of this process.  Loaded
        # the other way round, libmcamd.so binds /opt/rocm's copy and its launches go to a second runtime that
        # never saw torch's device / streams ("no ROCm-capable device is detected").
        import torch  # noqa: F401
        h = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(h, name)          # AttributeError here = header/library mismatch
            fn.restype = res
            fn.argtypes = args
        _lib = h
    return _lib


def reload_config():
    """Have the library re-read its MCAMD_* switches (they are cached at first use; tests that change one call this)."""
    lib().mcamd_reload_config()


def check(rc, what=""):
    if rc != 0:
        msg = lib().mcamd_last_error().decode()
        raise McamdError("%s failed (%d): %s" % (what or "mcamd call", rc, msg))


def ptr(t):
    """Device pointer of a torch tensor (or None)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
