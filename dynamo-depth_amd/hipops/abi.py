"""ctypes mirror of include/dynamo_hip.h (the C ABI of libdynamo_hip.so).

Only plain pointers / ints / floats cross this boundary -- no torch types.  Tensors are handed over
as `tensor.data_ptr()`; the caller (hipops.functions) validates dtype / contiguity / device first.
"""
import ctypes as C

DD_MAX_SCALES = 4
DD_NUM_SRC = 2
DD_ABI_VERSION = 2
DD_MODE_RIGID, DD_MODE_FLOW, DD_MODE_FLOW_MASK = 0, 1, 2
DD_PARTIAL_STRIDE = 40
DD_SUMS_STRIDE = 8
DD_OBJECTS_ROW = 22         # 32-bit words per row of dd_objects' table
DD_TRACKS_LINK = 6          # 32-bit words per row of dd_tracks_link's links
DD_TRACKS_MAX_OBJECTS = 1024
DD_DTYPE_F32, DD_DTYPE_F16, DD_DTYPE_BF16 = 0, 1, 2         # `dtype` of the element-typed (_t) entry points

_fp = C.c_void_p        # device (or, for the host-math test library, host) float*


class DDPhotoScale(C.Structure):
    _fields_ = [
        ("shift", C.c_int), ("h", C.c_int), ("w", C.c_int),
        ("w_photo", C.c_float), ("w_cons", C.c_float),
        ("disp", _fp),
        ("flow", _fp * DD_NUM_SRC),
        ("mask", _fp * DD_NUM_SRC),
        ("noise", _fp),
        ("g_disp", _fp),
        ("g_flow", _fp * DD_NUM_SRC),
        ("g_mask", _fp * DD_NUM_SRC),
        ("out_color", _fp * DD_NUM_SRC),
        ("out_sample", _fp * DD_NUM_SRC),
        ("out_depth", _fp),
        ("out_idsel", _fp),
        ("out_resid", _fp * DD_NUM_SRC),
        ("out_delta", _fp * DD_NUM_SRC),
    ]


class DDPhotoArgs(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int),
        ("B", C.c_int), ("H", C.c_int), ("W", C.c_int),
        ("num_scales", C.c_int), ("mode", C.c_int), ("automask", C.c_int), ("want_grad", C.c_int),
        ("min_depth", C.c_float), ("max_depth", C.c_float), ("ssim_weight", C.c_float),
        ("eps", C.c_float), ("disp_thr", C.c_float),
        ("target", _fp),
        ("source", _fp * DD_NUM_SRC),
        ("source_packed", _fp * DD_NUM_SRC),
        ("K", _fp), ("inv_K", _fp),
        ("T", _fp * DD_NUM_SRC),
        ("ts", _fp * DD_NUM_SRC),
        ("g_T", _fp * DD_NUM_SRC),
        ("sums", _fp),
        ("workspace", _fp),
        ("scale", DDPhotoScale * DD_MAX_SCALES),
    ]


DD_NUM_TERMS = 7
DD_MAX_RES = 128
TERM_NAMES = ("p_photo", "d_smooth", "d_ground", "c_smooth", "c_consistency", "m_sparsity", "m_smooth")   # options.py g_* order


class DDAssembleArgs(C.Structure):
    _fields_ = [
        ("n", C.c_int), ("num_scales", C.c_int),
        ("coef", C.c_float * DD_NUM_TERMS),
        ("norm", C.c_float * DD_MAX_RES),
        ("term_of", C.c_int8 * DD_MAX_RES),
        ("scale_of", C.c_int8 * DD_MAX_RES),
    ]


DD_VIS_MAX_TILES = 16
DD_VIS_KINDS = {"img": 0, "ref_img": 1, "disp": 2, "mask": 3, "ego_flow": 4, "ind_flow": 5, "comp_flow": 6, "samp_flow": 7}     # DD_VIS_*

DD_REG_SMOOTH = 5
DD_REG_RES_STRIDE = 16


class DDRegSmooth(C.Structure):
    _fields_ = [("inp", _fp), ("g_inp", _fp), ("C", C.c_int), ("normalise", C.c_int), ("weight", C.c_float)]


class DDRegScale(C.Structure):
    _fields_ = [
        ("h", C.c_int), ("w", C.c_int),
        ("img", _fp),
        ("smooth", DDRegSmooth * DD_REG_SMOOTH),
        ("delta", _fp * DD_NUM_SRC), ("delta_sum", _fp * DD_NUM_SRC), ("prob", _fp * DD_NUM_SRC), ("g_prob", _fp * DD_NUM_SRC),
        ("w_sparsity", C.c_float * DD_NUM_SRC),
        ("disp", _fp), ("g_disp", _fp), ("inv_K", _fp), ("rand_idx", _fp), ("plane", _fp),
        ("w_ground", C.c_float),
    ]


class DDRegArgs(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int), ("B", C.c_int), ("num_scales", C.c_int),
        ("np_per_it", C.c_int), ("max_it", C.c_int),
        ("tol", C.c_float), ("g_prior", C.c_float), ("min_depth", C.c_float), ("max_depth", C.c_float),
        ("res", _fp), ("workspace", _fp),
        ("scale", DDRegScale * DD_MAX_SCALES),
    ]


class DDJpegHeader(C.Structure):
    """include/dynamo_hip.h DDJpegHeader."""
    _fields_ = [("data_offset", C.c_int32), ("data_end", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("restart_interval", C.c_int32),
                ("ncomp", C.c_int32), ("h", C.c_int32 * 3), ("v", C.c_int32 * 3), ("tq", C.c_int32 * 3), ("td", C.c_int32 * 3), ("ta", C.c_int32 * 3),
                ("reserved", C.c_int32 * 3), ("qt", (C.c_uint16 * 64) * 4), ("bits", (C.c_uint8 * 16) * 4), ("vals", (C.c_uint8 * 256) * 4)]


def ptr(t):
    """Raw address of a tensor's storage (None -> NULL)."""
    return None if t is None else C.c_void_p(t.data_ptr())


_i, _f, _d, _v, _z, _ll = C.c_int, C.c_float, C.c_double, C.c_void_p, C.c_size_t, C.c_longlong

# name -> (restype, argtypes): one entry per prototype of include/dynamo_hip.h, the only list of entry points on the Python side
# (tests/test_abi.py holds it against the header, argument by argument)
SIGNATURES = {
    "dd_photo_loss": (_i, [C.POINTER(DDPhotoArgs), _v]),
    "dd_photo_workspace_bytes": (_z, [C.POINTER(DDPhotoArgs)]),
    "dd_photo_timing": (_i, [_i]),
    "dd_photo_timing_read": (_i, [C.POINTER(C.c_float), C.POINTER(_i), _i]),
    "dd_photo_loss_part": (_i, [C.POINTER(DDPhotoArgs), _v, _i]),
    "dd_smooth_loss": (_i, [_v, _v, _i, _i, _i, _i, _i, _f, _v, _v, _v, _v]),
    "dd_smooth_workspace_bytes": (_z, [_i, _i, _i, _i]),
    "dd_ground_loss": (_i, [_v, _v, _v, _i, _i, _i, _i, _i, _f, _f, _f, _f, _f, _v, _v, _v, _v, _v]),
    "dd_ground_workspace_bytes": (_z, [_i, _i, _i, _i]),
    "dd_resize_workspace_bytes": (_z, [_i, _i, _i, _i, _i]),
    "dd_resize_bicubic": (_i, [_v, _i, _i, _i, _v, _v, _i, _i, _v, _v, _i, _v, _v, _i, _v, _z, _v]),
    "dd_ground_candidates": (_i, [_v, _v, _v, _i, _i, _i, _i, _i, _f, _f, _f, _v, _v]),
    "dd_ground_select": (_i, [_v, _v, _v, _i, _i, _i, _i, _f, _f, _f, _f, _f, _v, _v, _v, _v, _v, _v]),
    "dd_ground_plane": (_i, [_v, _v, _i, _i, _i, _i, _i, _f, _f, _v, _v, _v, _v]),
    "dd_assemble_losses": (_i, [_v, C.POINTER(DDAssembleArgs), _v, _v, _v]),
    "dd_reg_losses_finish": (_i, [C.POINTER(DDRegArgs), C.POINTER(DDAssembleArgs), _v, _v, _v]),
    "dd_fused_loss": (_i, [C.POINTER(DDPhotoArgs), C.POINTER(DDRegArgs), C.POINTER(DDAssembleArgs), _v, _v, _v]),
    "dd_fused_loss_part": (_i, [C.POINTER(DDPhotoArgs), C.POINTER(DDRegArgs), C.POINTER(DDAssembleArgs), _v, _v, _v, _i]),
    "dd_fused_loss_supported": (_i, [C.POINTER(DDPhotoArgs), C.POINTER(DDRegArgs)]),
    "dd_reg_workspace_bytes": (_z, [C.POINTER(DDRegArgs)]),
    "dd_jpeg_workspace_bytes": (_z, [_i, _i, _i, _i, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "dd_jpeg_decode": (_i, [_v, _ll, _v, _i, _i, _i, _i, C.POINTER(C.c_int), C.POINTER(C.c_int), _v, _v, _z, _v]),
    "dd_backproject": (_i, [_v, _v, _i, _i, _i, _v, _v]),
    "dd_backproject_bwd": (_i, [_v, _v, _i, _i, _i, _v, _v]),
    "dd_project3d": (_i, [_v, _v, _v, _i, _i, _i, _f, _v, _v, _v]),
    "dd_project3d_bwd": (_i, [_v, _v, _v, _v, _v, _i, _i, _i, _f, _v, _v, _v, _v]),
    "dd_project3d_workspace_bytes": (_z, [_i, _i, _i]),
    "dd_ssim": (_i, [_v, _v, _i, _i, _i, _i, _v, _v]),
    "dd_ssim_bwd": (_i, [_v, _v, _v, _i, _i, _i, _i, _v, _v, _v]),
    "dd_disp_to_depth": (_i, [_v, _z, _f, _f, _v, _v, _v]),
    "dd_pose_matrix": (_i, [_v, _v, _i, _i, _v, _v]),
    "dd_pose_matrix_bwd": (_i, [_v, _v, _v, _i, _i, _v, _v, _v]),
    "dd_channel_sum_workspace_bytes": (_z, [_i]),
    "dd_dwconv3x3_workspace_bytes": (_z, [_i, _i, _i]),
    "dd_conv3x3_cout1_bwd_data": (_i, [_v, _v, _i, _i, _i, _i, _i, _v, _v]),
    "dd_prepare_frames": (_i, [_v, _v, _v, _i, _i, _i, _i, _v, _v, _v, _v]),
    "dd_prepare_frames_workspace_bytes": (_z, [_i, _i]),
    "dd_pyramid_down2": (_i, [_v, _i, _i, _i, _v, _v]),
    "dd_pack_rgb": (_i, [_v, _i, _i, _i, _v, _v]),
    "dd_depth_metrics": (_i, [_v, _i, _i, _i, _v, _v, _i, _v, C.POINTER(_d), _f, _f, _v, _v, _v, _z, _v]),
    "dd_depth_metrics_workspace_bytes": (_z, [_i, _i]),
    "dd_depth_metrics_masked": (_i, [_v, _i, _i, _i, _v, _v, _i, _v, C.POINTER(_d), _f, _f, _v, _i, _i, _v, _v, _v, _v, _z, _v]),
    "dd_depth_metrics_masked_workspace_bytes": (_z, [_i, _i]),
    "dd_depth_metrics_accumulate": (_i, [_v, _v, _i, _v, _v, _v]),
    "dd_odom_snippet_count": (_i, [_i, _i]),
    "dd_odom_snippets": (_i, [_v, _v, _i, _i, _v, _v, _v]),
    "dd_motion_pr": (_i, [_v, _i, _i, _i, _v, _v, _i, _i, _v, _i, _i, _v, _v]),
    "dd_fill_contours": (_i, [_v, _i, _v, _i, _i, _i, _i, _v, _v]),
    "dd_lidar_depth_points_workspace_bytes": (_z, [_i, _i, _i, _i]),
    "dd_lidar_depth_points": (_i, [_v, _ll, C.POINTER(C.c_int32), _i, _v, _i, _i, _i, _v, _v, _v, _v, _z, _v]),
    "dd_lidar_pose_points_workspace_bytes": (_z, [_i, _ll]),
    "dd_lidar_pose_points": (_i, [_v, _ll, C.POINTER(C.c_int32), _i, _v, _v, _v, _v, _z, _v]),
    "dd_box_fit": (_i, [_v, _i, _v, _v, _i, _v, _v, _i, _v, _v, _v]),
    "dd_range_image_points_workspace_bytes": (_z, [_i, _ll]),
    "dd_range_image_points": (_i, [_v, _v, _v, _v, _ll, _ll, _ll, C.POINTER(C.c_int32), _i, _v, _v, _v, _v, _v, _v, _z, _v]),
    "dd_undistort": (_i, [_v, _i, _i, _i, C.POINTER(_d), _v, _v]),
    "dd_resize_area": (_i, [_v, _i, _i, _i, _v, _i, _i, _v, _v, _v, _i, _v, _v, _v, _i, _v]),
    "dd_vis_frame": (_i, [_v, _v, _v, _v, _v, _v, _v, _v, _f, _f, _i, _i, C.POINTER(C.c_int), _i, _i, _i, _v, _f, _f, _f, _f, _i, _i, _v, _v, _v, _v]),
    "dd_vis_flow_tiles": (_i, [_v, _v, C.POINTER(C.c_int), _i, _i, _i, _i, _i, _i, _f, _i, _v, _v]),
    "dd_export_depth": (_i, [_v, _v, _v, _i, _i, _i, _i, _i, _f, _f, _f, _v, _f, _f, _v, _v, _v, _v]),
    "dd_export_plane_u8": (_i, [_v, _i, _i, _i, _i, _i, _v, _v]),
    "dd_export_cloud_workspace_bytes": (_z, [_i, _i, _i, _i]),
    "dd_export_cloud": (_i, [_v, _v, _v, _v, _v, _v, _i, _i, _i, _i, _i, _f, _f, _f, _f, _f, _f, _f, _f, _f, _i, _v, _v, _v, _z, _v]),
    "dd_objects_workspace_bytes": (_z, [_i, _i, _i, _i]),
    "dd_objects": (_i, [_v, _v, _v, _v, _v, _v, _v, _i, _i, _i, _f, _f, _f, _f, _f, _f, _f, _i, _i, _i, _v, _v, _v, _v, _z, _v]),
    "dd_export_labels_u16": (_i, [_v, _i, _i, _i, _i, _i, _v, _v]),
    "dd_tracks_link": (_i, [_v, _v, _v, _v, _v, _v, _v, _i, _i, _i, _f, _f, _f, _f, _f, _f, _i, _v, _v, _v]),
    "dd_bn_workspace_bytes": (_z, [_i]),
    "dd_bn_act_fwd_t": (_i, [_v, _v, _ll, _i, _v, _v, _f, _f, _v, _v, _v, _v, _i, _v, _i, _v, _z, _v]),
    "dd_bn_act_bwd_t": (_i, [_v, _v, _v, _ll, _i, _v, _v, _v, _v, _i, _v, _v, _v, _v, _i, _v, _z, _v]),
    "dd_channel_sum_nhwc_t": (_i, [_v, _ll, _i, _v, _i, _v, _v]),
    "dd_reflect_pad1_nhwc_t": (_i, [_v, _i, _i, _i, _i, _v, _i, _v]),
    "dd_reflect_pad1_nhwc_bwd_t": (_i, [_v, _i, _i, _i, _i, _v, _i, _v]),
    "dd_up_cat_pad_t": (_i, [_v, _v, _i, _i, _i, _i, _i, _i, _i, _v, _i, _v]),
    "dd_up_cat_pad_bwd_t": (_i, [_v, _v, _i, _i, _i, _i, _i, _i, _i, _v, _v, _i, _v]),
    "dd_layer_norm_workspace_bytes": (_z, [_i]),
    "dd_layer_scale_workspace_bytes": (_z, [_i, _i]),
    "dd_layer_norm_fwd_t": (_i, [_v, _ll, _i, _v, _v, _f, _v, _v, _v, _i, _v]),
    "dd_layer_norm_bwd_t": (_i, [_v, _v, _v, _v, _v, _ll, _i, _v, _v, _v, _z, _i, _v]),
    "dd_layer_scale_bwd_t": (_i, [_v, _v, _v, _i, _i, _i, _v, _v, _v, _z, _i, _v]),
    "dd_layer_scale_fwd_t": (_i, [_v, _v, _v, _i, _i, _i, _v, _i, _v]),
    "dd_dwconv3x3_nhwc_t": (_i, [_v, _v, _i, _i, _i, _i, _i, _v, _i, _v]),
    "dd_dwconv3x3_nhwc_bwd_data_t": (_i, [_v, _v, _i, _i, _i, _i, _i, _v, _i, _v]),
    "dd_dwconv3x3_nhwc_bwd_weight_t": (_i, [_v, _v, _i, _i, _i, _i, _i, _v, _v, _z, _i, _v]),
    "dd_redu_supported": (_i, [_i, _i]),
    "dd_redu_workspace_bytes": (_z, [_ll, _i, _i]),
    "dd_redu_fwd": (_i, [_v, _v, _v, _v, _ll, _i, _i, _v, _v]),
    "dd_redu_bwd_data": (_i, [_v, _v, _ll, _i, _i, _v, _v, _v]),
    "dd_redu_bwd_weight": (_i, [_v, _v, _v, _ll, _i, _i, _v, _v, _v, _z, _v]),
    "dd_conv_head_supported": (_i, [_i]),
    "dd_conv_head_workspace_bytes": (_z, [_i, _i, _i, _i]),
    "dd_conv_head_fwd": (_i, [_v, _v, _ll, _ll, _ll, _v, _i, _i, _i, _i, _v, _v]),
    "dd_conv_head_bwd_weight": (_i, [_v, _v, _i, _i, _i, _i, _v, _v, _v, _z, _v]),
    "dd_conv_small_supported": (_i, [_i, _i, _i]),
    "dd_conv_small_workspace_bytes": (_z, [_i, _i, _i]),
    "dd_conv_small_fwd": (_i, [_v, _v, _ll, _ll, _ll, _ll, _v, _i, _i, _i, _i, _i, _i, _v, _v, _z, _v]),
    "dd_conv_small_bwd_data": (_i, [_v, _v, _ll, _ll, _ll, _ll, _i, _i, _i, _i, _i, _i, _v, _v, _z, _v]),
    "dd_conv_small_bwd_weight": (_i, [_v, _v, _i, _i, _i, _i, _i, _i, _v, _v, _v, _z, _v]),
    "dd_conv3x3_mfma_supported": (_i, [_i, _i]),
    "dd_conv3x3_mfma_pack_bytes": (_z, [_i, _i]),
    "dd_conv3x3_mfma_pack": (_i, [_v, _ll, _ll, _ll, _ll, _i, _i, _v, _v, _v]),
    "dd_conv3x3_mfma_pack_many_job_words": (_i, []),
    "dd_conv3x3_mfma_pack_many_blocks": (_i, [_i, _i, _i, _i]),
    "dd_conv3x3_mfma_pack_many": (_i, [_v, _v, _i, _v]),
    "dd_conv3x3_mfma": (_i, [_v, _v, _v, _i, _i, _i, _i, _i, _i, _v, _v]),
    "dd_conv3x3_mfma_n": (_i, [_v, _v, _v, _i, _i, _i, _i, _i, _i, _i, _v, _v]),
    "dd_conv3x3_mfma_flat_supported": (_i, [_i, _i, _i, _i, _i]),
    "dd_conv3x3_mfma_flat_workspace_bytes": (_z, [_i, _i, _i, _i, _i]),
    "dd_conv3x3_mfma_flat": (_i, [_v, _v, _v, _i, _i, _i, _i, _i, _v, _v, _z, _v]),
    "dd_conv3x3_mfma_flat_n": (_i, [_v, _v, _v, _i, _i, _i, _i, _i, _i, _v, _v, _z, _v]),
    "dd_conv3x3_mfma_wgrad_workspace_bytes": (_z, [_i, _i, _i, _i, _i]),
    "dd_conv3x3_mfma_bwd_weight": (_i, [_v, _v, _i, _i, _i, _i, _i, _i, _v, _v, _z, _v]),
    "dd_conv3x3_mfma_bwd_weight_n": (_i, [_v, _v, _i, _i, _i, _i, _i, _i, _i, _v, _v, _z, _v]),
    "dd_conv3x3_half_supported": (_i, [_i, _i]),
    "dd_conv3x3_half_pack_bytes": (_z, [_i, _i]),
    "dd_conv3x3_half_pack": (_i, [_v, _ll, _ll, _ll, _ll, _i, _i, _i, _v, _v, _v]),
    "dd_conv3x3_half": (_i, [_v, _v, _v, _i, _i, _i, _i, _i, _i, _i, _v, _v]),
    "dd_conv3x3_half_wgrad_workspace_bytes": (_z, [_i, _i, _i, _i, _i]),
    "dd_conv3x3_half_bwd_weight": (_i, [_v, _v, _i, _i, _i, _i, _i, _i, _i, _v, _v, _z, _v]),
    "dd_pw_gemm_pack_bytes": (_z, [_i, _i]),
    "dd_mlp_pack": (_i, [_v, _ll, _ll, _v, _ll, _ll, _i, _i, _v, _v, _v, _v, _v, _v]),
    "dd_mlp_fwd_supported": (_i, [_i]),
    "dd_mlp_fwd": (_i, [_v, _v, _v, _v, _v, _i, _i, _v, _v]),
    "dd_mlp_fwd_splits": (_i, [_i, _i]),
    "dd_mlp_fwd_workspace_bytes": (_z, [_i, _i, _i]),
    "dd_mlp_fwd_n": (_i, [_v, _v, _v, _v, _v, _i, _i, _i, _i, _v, _v, _z, _v]),
    "dd_pw_gemm": (_i, [_v, _v, _v, _i, _i, _i, _i, _v, _v]),
    "dd_gelu_pair": (_i, [_v, _v, _v, _z, _v]),
    "dd_mlp_train_pack": (_i, [_v, _ll, _ll, _v, _ll, _ll, _i, _i, _v, _v, _v, _v, _v]),
    "dd_mlp_train_pack_narrow": (_i, [_v, _ll, _ll, _v, _ll, _ll, _i, _i, _v, _v, _v, _v, _v]),
    "dd_mlp_train_fwd": (_i, [_v, _v, _v, _v, _v, _i, _i, _i, _i, _v, _v, _v, _v, _z, _v]),
    "dd_mlp_train_bwd_workspace_bytes": (_z, [_i, _i, _i]),
    "dd_mlp_train_bwd": (_i, [_v, _v, _v, _v, _i, _i, _i, _i, _v, _v, _v, _z, _v]),
    "dd_linear_wgrad_supported": (_i, [_i, _i, _i]),
    "dd_linear_wgrad_workspace_bytes": (_z, [_i, _i, _i]),
    "dd_linear_wgrad": (_i, [_v, _v, _i, _i, _i, _v, _v, _v, _z, _v]),
    "dd_linear_wgrad_n": (_i, [_v, _v, _i, _i, _i, _i, _v, _v, _v, _z, _v]),
    "dd_adam_chunk": (_i, []),
    "dd_adam_multi": (_i, [_v, _i, _v, _i, _v, _d, _d, _d, _d, _d, _v, _v, _v]),
    "dd_error_string": (C.c_char_p, [_i]),
    "dd_abi_version": (_i, []),
}
EXPORTED = tuple(SIGNATURES)


def declare(lib):
    """Attaches restype/argtypes for every entry point of include/dynamo_hip.h and returns their names.  A library that lacks some
    of them (a stale build) gets the others set, then an AttributeError that names every missing one."""
    missing = []
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is None:
            missing.append(name)
            continue
        fn.restype = res
        fn.argtypes = args
    if missing:
        raise AttributeError("no symbol " + ", ".join(missing))
    return EXPORTED


def fill_photo_args(*, B, H, W, mode, automask, want_grad, min_depth, max_depth, ssim_weight, eps, disp_thr,
                    target, source, K, inv_K, T, ts, g_T, sums, workspace, scales, source_packed=None):
    """Builds a DDPhotoArgs from tensors.  `scales` is a list of dicts with the DDPhotoScale field names
    (tensors or None; per-frame entries as 2-lists)."""
    a = DDPhotoArgs()
    a.abi_version = DD_ABI_VERSION
    a.B, a.H, a.W = B, H, W
    a.num_scales = len(scales)
    a.mode, a.automask, a.want_grad = mode, int(bool(automask)), int(bool(want_grad))
    a.min_depth, a.max_depth, a.ssim_weight, a.eps, a.disp_thr = min_depth, max_depth, ssim_weight, eps, disp_thr
    a.target = ptr(target)
    a.K, a.inv_K = ptr(K), ptr(inv_K)
    a.sums, a.workspace = ptr(sums), ptr(workspace)
    for f in range(DD_NUM_SRC):
        a.source[f] = ptr(source[f])
        a.source_packed[f] = ptr(source_packed[f]) if source_packed is not None else None
        a.T[f] = ptr(T[f])
        a.ts[f] = ptr(ts[f]) if ts is not None else None
        a.g_T[f] = ptr(g_T[f]) if g_T is not None else None
    for s, d in enumerate(scales):
        sc = a.scale[s]
        sc.shift, sc.h, sc.w = d["shift"], d["h"], d["w"]
        sc.w_photo, sc.w_cons = d.get("w_photo", 0.0), d.get("w_cons", 0.0)
        for name in ("disp", "noise", "g_disp", "out_depth", "out_idsel"):
            setattr(sc, name, ptr(d.get(name)))
        for name in ("flow", "mask", "g_flow", "g_mask", "out_color", "out_sample", "out_resid", "out_delta"):
            pair = d.get(name) or (None, None)
            arr = getattr(sc, name)
            for f in range(DD_NUM_SRC):
                arr[f] = ptr(pair[f])
    return a
