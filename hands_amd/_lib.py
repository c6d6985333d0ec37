"""ctypes binding of ``libhands_hip.so`` (declared in include/hands_hip.h).

The product path has no CPU fallback: if the shared library is missing or cannot be loaded,
:func:`lib` raises and every op of :mod:`hands_amd` fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HANDS_HIP_LIB") or os.path.join(_HERE, "libhands_hip.so")   # HANDS_HIP_LIB: developer A/B builds only

c_float_p = C.c_void_p  # raw device pointers travel as integers


class ConvDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "B", "H", "W", "Cin", "Ho", "Wo", "Cout", "KH", "KW", "stride", "pad",
        "in_pix_stride", "out_pix_stride", "res_pix_stride", "Kpad", "act")]


ACT_NONE, ACT_RELU, ACT_GELU, ACT_LEAKY_RELU = 0, 1, 2, 3


class ManoConsts(C.Structure):
    _fields_ = [("pose_mean", C.c_void_p), ("J_template", C.c_void_p), ("J_shapedirs", C.c_void_p),
                ("lbs_weights", C.c_void_p), ("tip_ids", C.c_void_p)]


class ManoOut(C.Structure):
    _fields_ = [("vertices", C.c_void_p), ("joints3d", C.c_void_p), ("v3d_cam", C.c_void_p),
                ("j3d_cam", C.c_void_p), ("j2d_norm", C.c_void_p), ("cam_t", C.c_void_p)]


class ManoSide(C.Structure):
    _fields_ = [("consts", ManoConsts), ("blend_w", C.c_void_p), ("blend_bias", C.c_void_p), ("rot", C.c_void_p),
                ("betas", C.c_void_p), ("cam_wp", C.c_void_p), ("out", ManoOut)]


class PackedDims(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("Cin", "Cout", "Cout_pad", "Kpad")]


class EvalIn(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "pred_j3d_r", "pred_j3d_l", "gt_j3d_r", "gt_j3d_l", "pred_j2d_r", "pred_j2d_l", "gt_j2d_r", "gt_j2d_l",
        "is_valid", "right_valid", "left_valid", "joints_valid_r", "joints_valid_l")]


class EvalOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "mpjpe_ra_h", "mpjpe_pa_ra_r", "mpjpe_pa_ra_l", "mpjpe_pa_ra_h", "mrrpe_rl", "pix_err_r", "pix_err_l")]


class EvalMaskedOut(C.Structure):
    """hands_eval_masked_out (include/hands_hip.h): the nine values of the egoexo branch of eval_mpjpe_pa_ra."""
    _fields_ = [(n, C.c_void_p) for n in (
        "rao_r", "rao_l", "rao_h", "abs_r", "abs_l", "abs_h", "pa_ra_r", "pa_ra_l", "pa_ra_h")]


class MeshEvalIn(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "pred_v3d_r", "pred_v3d_l", "gt_v3d_r", "gt_v3d_l", "pred_j3d_r", "pred_j3d_l", "gt_j3d_r", "gt_j3d_l",
        "is_valid", "right_valid", "left_valid")]


MESH_MAX_V, MESH_NQ = 1024, 10            # HANDS_MESH_MAX_V, HANDS_MESH_NQ
# hands_mesh_eval_out: quantity q of hand s (r, l, h) is pointer 3 * q + s
MESH_QUANTITIES = ("mpvpe_ra", "f5_ra", "f15_ra", "auc_ra_v", "auc_ra_j", "mpvpe_pa", "f5_pa", "f15_pa", "auc_pa_v", "auc_pa_j")


class MeshEvalOut(C.Structure):
    _fields_ = [(f"{q}_{s}", C.c_void_p) for q in MESH_QUANTITIES for s in "rlh"]


SURF_MAX_F, SURF_CHUNK, SURF_NQ = 4096, 512, 4     # HANDS_SURF_MAX_F, HANDS_SURF_CHUNK, HANDS_SURF_NQ
SIGNED_CHUNK = 256                                 # HANDS_SIGNED_CHUNK
SURF_QUANTITIES = ("p2s_ra", "p2s_pa", "chamfer_ra", "chamfer_pa")


class SurfEvalOut(C.Structure):
    """hands_surf_eval_out (include/hands_hip.h): quantity q of hand s (r, l, h) is pointer 3 * q + s."""
    _fields_ = [(f"{q}_{s}", C.c_void_p) for q in SURF_QUANTITIES for s in "rlh"]


ACCEL_NQ = 3                                       # HANDS_ACCEL_NQ
ACCEL_QUANTITIES = ("acc", "acc_j", "acc_abs")


class AccelEvalOut(C.Structure):
    """hands_accel_eval_out (include/hands_hip.h): quantity q of hand s (r, l, h) is pointer 3 * q + s."""
    _fields_ = [(f"{q}_{s}", C.c_void_p) for q in ACCEL_QUANTITIES for s in "rlh"]


class SmoothSide(C.Structure):
    """hands_smooth_side (include/hands_hip.h): one hand of a hands_smooth_mano_f32 call; valid and state may be NULL."""
    _fields_ = [(n, C.c_void_p) for n in ("pose", "beta", "cam", "valid", "pose_out", "beta_out", "cam_out", "state")]


SMOOTH_SHAPE_MODES = {"filter": 0, "mean": 1, "none": 2}     # HANDS_SMOOTH_SHAPE_*


class SmoothCfg(C.Structure):
    """hands_smooth_cfg (include/hands_hip.h): index 0 rotations, 1 shape, 2 camera."""
    _fields_ = [("min_cutoff", C.c_double * 3), ("beta", C.c_double * 3), ("d_cutoff", C.c_double * 3), ("shape_mode", C.c_int)]


class ManoFitConsts(C.Structure):
    """hands_mano_fit_consts (include/hands_hip.h): the three joint constants of ManoConsts and the tip pack."""
    _fields_ = [(n, C.c_void_p) for n in ("pose_mean", "J_template", "J_shapedirs", "tip_v_template", "tip_shapedirs",
                                          "tip_lbs_weights", "tip_posedirs")]


class ManoFitSide(C.Structure):
    """hands_mano_fit_side (include/hands_hip.h): one hand of a hands_mano_fit_f32 call; weights, valid and init_* may be NULL."""
    _fields_ = [("consts", ManoFitConsts)] + [(n, C.c_void_p) for n in (
        "joints", "weights", "valid", "init_pose", "init_beta", "init_transl", "pose", "beta", "transl", "rmse", "steps")]


class FitCfg(C.Structure):
    """hands_fit_cfg (include/hands_hip.h)."""
    _fields_ = [("iters", C.c_int), ("lambda_beta", C.c_double), ("lambda_pose", C.c_double), ("mu0", C.c_double)]


class ManoFit2DSide(C.Structure):
    """hands_mano_fit2d_side (include/hands_hip.h): one hand of a hands_mano_fit2d_f32 call; weights, valid and init_* may be NULL."""
    _fields_ = [("consts", ManoFitConsts)] + [(n, C.c_void_p) for n in (
        "kp2d", "weights", "valid", "init_pose", "init_beta", "init_transl", "pose", "beta", "transl", "rmse", "steps", "start",
        "j3d", "j2d")]


class Fit2DCfg(C.Structure):
    """hands_fit2d_cfg (include/hands_hip.h)."""
    _fields_ = [("iters_rigid", C.c_int), ("iters", C.c_int), ("lambda_beta", C.c_double), ("lambda_pose", C.c_double),
                ("mu0", C.c_double), ("robust_sigma", C.c_double), ("z_min", C.c_double), ("fit_shape", C.c_int),
                ("prior_to_init", C.c_int)]


class ManoFitVertsConsts(C.Structure):
    """hands_mano_fit_verts_consts (include/hands_hip.h): the three joint constants and the full vertex constants."""
    _fields_ = [(n, C.c_void_p) for n in ("pose_mean", "J_template", "J_shapedirs", "v_template", "shapedirs", "lbs_weights",
                                          "posedirs_vm")]


class ManoFitVertsSide(C.Structure):
    """hands_mano_fit_verts_side (include/hands_hip.h): one hand of a hands_mano_fit_verts_f32 call; weights, valid and init_* may
    be NULL."""
    _fields_ = [("consts", ManoFitVertsConsts)] + [(n, C.c_void_p) for n in (
        "verts", "weights", "valid", "init_pose", "init_beta", "init_transl", "pose", "beta", "transl", "rmse", "steps", "j3d")]


class ManoFitSurfConsts(C.Structure):
    """hands_mano_fit_surf_consts (include/hands_hip.h): hands_mano_fit_verts_consts and the face list (1538,3) int32."""
    _fields_ = [(n, C.c_void_p) for n in ("pose_mean", "J_template", "J_shapedirs", "v_template", "shapedirs", "lbs_weights",
                                          "posedirs_vm", "faces")]


class ManoFitSurfSide(C.Structure):
    """hands_mano_fit_surf_side (include/hands_hip.h): one hand of a hands_mano_fit_surf_f32 call; weights, valid, init_* and
    normals may be NULL."""
    _fields_ = [("consts", ManoFitSurfConsts)] + [(n, C.c_void_p) for n in (
        "points", "weights", "valid", "init_pose", "init_beta", "init_transl", "pose", "beta", "transl", "rmse", "steps", "j3d",
        "verts", "face_idx", "bary", "normals")]


class FitSurfCfg(C.Structure):
    """hands_fit_surf_cfg (include/hands_hip.h)."""
    _fields_ = [("iters", C.c_int), ("lambda_beta", C.c_double), ("lambda_pose", C.c_double), ("mu0", C.c_double),
                ("tangent_weight", C.c_double)]


class LossIn(C.Structure):
    """hands_loss_in (include/hands_hip.h): the first LOSS_N_MANDATORY pointers are mandatory, the rest come in groups."""
    _fields_ = [(n, C.c_void_p) for n in (
        "pred_pose_r", "pred_pose_l", "pred_beta_r", "pred_beta_l", "pred_j3d_r", "pred_j3d_l", "pred_j2d_r", "pred_j2d_l",
        "pred_cam_wp_r", "pred_cam_wp_l", "pred_cam_wp_init_r", "pred_cam_wp_init_l",
        "gt_pose_r", "gt_pose_l", "gt_beta_r", "gt_beta_l", "gt_j3d_r", "gt_j3d_l", "gt_j2d_r", "gt_j2d_l",
        "gt_cam_wp_r", "gt_cam_wp_l", "right_valid", "left_valid", "joints_valid_r", "joints_valid_l",
        "is_cam_loss", "is_j2d_loss", "is_j3d_loss", "is_pose_loss", "is_beta_loss",
        "pred_grasp_r", "pred_grasp_l", "gt_grasp_r", "gt_grasp_l", "grasp_valid_r", "grasp_valid_l", "is_grasp_loss",
        "pred_mask_r", "pred_mask_l", "gt_mask_r", "gt_mask_l", "render_valid_r", "render_valid_l", "is_mask_loss",
        "pred_depth_r", "pred_depth_l", "gt_depth_r", "gt_depth_l", "is_depth_loss",
        "pred_center_r", "pred_center_l", "gt_center_r", "gt_center_l",
        "pred_corner_r", "pred_corner_l", "gt_corner_r", "gt_corner_l")]


LOSS_NKEYS, LOSS_N_MANDATORY = 21, 31     # HANDS_LOSS_NKEYS, HANDS_LOSS_N_MANDATORY


class ShadeMesh(C.Structure):
    """hands_shade_mesh (include/hands_hip.h): one mesh of a shaded picture."""
    _fields_ = [("workspace", C.c_void_p), ("faces", C.c_void_p), ("valid", C.c_void_p), ("n_verts", C.c_int32),
                ("n_faces", C.c_int32), ("face_offset", C.c_int32), ("color", C.c_float * 3), ("metallic", C.c_float),
                ("roughness", C.c_float)]


SHADE_MAX_MESHES = 4     # HANDS_SHADE_MAX_MESHES


class ShadeScene(C.Structure):
    _fields_ = [("mesh", ShadeMesh * SHADE_MAX_MESHES), ("n_meshes", C.c_int32)]


# name -> argtypes; every function returns int (0 = ok) except the two noted below
_P, _I, _F = C.c_void_p, C.c_int, C.c_float
class ConvJob(C.Structure):
    """hands_conv_job (include/hands_hip.h): one member of a grouped pointwise launch."""
    _fields_ = [("desc", C.POINTER(ConvDesc)), ("in_", C.c_void_p), ("w_packed", C.c_void_p), ("bias", C.c_void_p),
                ("residual", C.c_void_p), ("out", C.c_void_p), ("pre_scale", C.c_void_p), ("pre_shift", C.c_void_p)]


SIGNATURES = {
    "hands_conv2d_nhwc_f32": [C.POINTER(ConvDesc), _P, _P, _P, _P, _P, _P],
    "hands_conv3x3_winograd_supported": [C.POINTER(ConvDesc)],
    "hands_conv3x3_winograd_f32": [C.POINTER(ConvDesc), _P, _P, _P, _P, _P],
    "hands_conv3x3_winograd4_supported": [C.POINTER(ConvDesc)],
    "hands_conv3x3_winograd4_f32": [C.POINTER(ConvDesc), _P, _P, _P, _P, _P],
    "hands_conv2d_splitk_factor": [C.POINTER(ConvDesc)],
    "hands_conv2d_group_class": [C.POINTER(ConvDesc), _I],
    "hands_conv2d_group_f32": [C.POINTER(ConvJob), _I, _P],
    "hands_conv2d_nhwc_splitk_f32": [C.POINTER(ConvDesc), _P, _P, _P, _P, _P, _P, C.c_longlong, _P],
    "hands_conv2d_nhwc_splitk_fused_f32": [C.POINTER(ConvDesc), _P, _P, _P, _P, _P, _I, _P, C.c_longlong, _P, C.c_longlong, _P],
    "hands_conv2d_streamk_grid": [C.POINTER(ConvDesc)],
    "hands_conv2d_nhwc_streamk_f32": [C.POINTER(ConvDesc), _P, _P, _P, _P, _P, _P, C.c_longlong, _I, _P],
    "hands_conv1x1_dual_nhwc_f32": [C.POINTER(ConvDesc), _P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P],
    "hands_conv2d_nhwc_splitk_n_f32": [C.POINTER(ConvDesc), _P, _P, _P, _P, _P, _I, _P, C.c_longlong, _P],
    "hands_conv2d_nhwc_pre_f32": [C.POINTER(ConvDesc), _P, _P, _P, _P, _P, _P, _P, _I, _P, C.c_longlong, _P],
    "hands_stem_conv_maxpool_nhwc_f32": [_P, _P, _P, _P, _I, _I, _I, _I, _P],
    "hands_stem_conv_maxpool_nchw_f32": [_P, _P, _P, _P, _I, _I, _I, _I, _P],
    "hands_nchw3_to_nhwc4_f32": [_P, _P, _I, _I, _I, _P],
    "hands_maxpool3x3s2_nhwc_f32": [_P, _P, _I, _I, _I, _I, _P],
    "hands_sumpool_nhwc_f32": [_P, _P, _I, _I, _I, _I, _P],
    "hands_avgpool_nhwc_f32": [_P, _P, _I, _I, _I, _I, _P],
    "hands_image_posenc_nhwc_f32": [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P],
    "hands_frontend_dense_maps_f32": [_P, _P, _P, _P, _I, _I, _I, _P],
    "hands_dense_posenc_f32": [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P],
    "hands_concat_nhwc_f32": [_P, _I, _I, _P, _I, _P, C.c_longlong, _I, _P, _I, _I, _I, _I, _P],
    "hands_upsample_bilinear_ac_f32": [_P, _P, _I, _I, _I, _I, _I, _I, _P],
    "hands_rot_leftmul_f32": [_P, _P, _I, _P],
    "hands_perspective_correction_f32": [_P, _P, _P, _P, _I, _P],
    "hands_kpe_concat_f32": [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P],
    "hands_hmr_init_f32": [_P, _P, _I, _I, _I, _P],
    "hands_rot6d_to_matrix_f32": [_P, _I, _P, _I, _P],
    "hands_flip_swap_f32": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P],
    "hands_matrix_to_axis_angle_f32": [_P, _P, C.c_longlong, _P],
    "hands_axis_angle_to_matrix_f32": [_P, _P, C.c_longlong, _P],
    "hands_grasp_input_f32": [_P, _I, _P, _P, _P, _I, _I, _I, _I, _P],
    "hands_mano_pose_f32": [C.POINTER(ManoConsts), _P, _P, _I, _P, _I, _P, _P, _I, _P],
    "hands_mano_heads_f32": [C.POINTER(ManoSide), _I, _P, _I, _F, _F, _I, _I, _P],
    "hands_mano_heads_vsplit": [_I, _I],
    "hands_mano_skin_f32": [C.POINTER(ManoConsts), _P, _I, _P, _P, _P, _P, _F, _F, C.POINTER(ManoOut), _I, _P],
    "hands_resize_crop_nchw3_to_nhwc4_f32": [_P, _P, _I, _I, _I, _I, _I, _I, _P],
    "hands_layernorm_f32": [_P, _P, _P, _P, _P, _I, _I, _I, _F, _P],
    "hands_add_pos_f32": [_P, _P, _P, _I, _I, _I, _P],
    "hands_kpe_encode_f32": [_P, _P, _P, _I, _I, _I, _P],
    "hands_attention_f32": [_P, _P, _I, _I, _I, _I, _F, _P],
    "hands_cross_attention_1q_f32": [_P, _P, _P, _I, _I, _I, _I, _F, _P],
    "hands_rot6d_to_matrix_cols_f32": [_P, _I, _P, _I, _P],
    "hands_vit_tokens_f32": [_P, _P, _P, _P, _I, _I, _I, _P],
    "hands_vit_tail_f32": [_P, _P, _P, _P, _I, _I, _I, _F, _P],
    "hands_wide_attention_f32": [_P, C.c_longlong, _I, _P, C.c_longlong, _I, _P, C.c_longlong, _I, _P, C.c_longlong, _I,
                                 _I, _I, _I, _I, _F, _P],
    "hands_vector_tokens_f32": [_P, _I, _I, _I, _P, _P, _P, _I, _I, _I, _P],
    "hands_token_mean_f32": [_P, _P, _I, _I, _I, _P],
    "hands_upsample_bilinear_add_f32": [_P, _P, _P, _I, _I, _I, _I, _I, _I, _P],
    "hands_pool2x2_nhwc_f32": [_P, _P, _I, _I, _I, _I, _I, _P],
    "hands_channel_pool_f32": [_P, _P, C.c_longlong, _I, _P],
    "hands_gate_apply_f32": [_P, _P, _I, _P, _P, C.c_longlong, _I, _P],
    "hands_add_embed2_f32": [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P],
    "hands_add_rowvec_f32": [_P, _P, _P, _I, _I, _I, _P],
    "hands_token_sum_f32": [_P, _P, _I, _I, _I, _P],
    "hands_bn_leaky_f32": [_P, _P, _P, _P, C.c_longlong, _I, _P],
    "hands_upsample_nearest2x_add_f32": [_P, _P, _P, _I, _I, _I, _I, _P],
    "hands_spatial_softmax_f32": [_P, _I, _P, _P, _I, _I, _I, _I, _P],
    "hands_flash_attention_f32": [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _F, _P],
    "hands_ceiling_hbm_read_f32": [_P, C.c_longlong, _P, _P],
    "hands_eval_metrics_f32": [C.POINTER(EvalIn), C.POINTER(EvalOut), _I, _P],
    "hands_eval_metrics_masked_f32": [C.POINTER(EvalIn), _P, _P, C.POINTER(EvalMaskedOut), _I, _P],
    "hands_eval_mesh_metrics_f32": [C.POINTER(MeshEvalIn), C.POINTER(MeshEvalOut), _I, _I, _P],
    "hands_mesh_closest_f32": [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P],
    "hands_mesh_signed_f32": [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P],
    "hands_eval_surface_metrics_f32": [C.POINTER(MeshEvalIn), _P, _P, _I, _I, C.POINTER(SurfEvalOut), _I, _I, _P],
    "hands_accel_error_f32": [_P, _P, _P, _P, _P, _I, _I, _I, _F, _P],
    "hands_eval_accel_metrics_f32": [C.POINTER(MeshEvalIn), _P, C.POINTER(AccelEvalOut), _I, _I, _F, _P],
    "hands_smooth_mano_f32": [C.POINTER(SmoothSide), _I, _P, _I, _I, _F, C.POINTER(SmoothCfg), _P],
    "hands_mano_fit_f32": [C.POINTER(ManoFitSide), _I, C.POINTER(FitCfg), _I, _P],
    "hands_mano_fit2d_f32": [C.POINTER(ManoFit2DSide), _I, _P, C.POINTER(Fit2DCfg), _I, _P],
    "hands_mano_fit_verts_f32": [C.POINTER(ManoFitVertsSide), _I, C.POINTER(FitCfg), _I, _P],
    "hands_mano_fit_surf_f32": [C.POINTER(ManoFitSurfSide), _I, C.POINTER(FitSurfCfg), _I, _I, _P],
    "hands_mesh_correspond_f32": [_P, _P, _P, _P, _P, _F, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P],
    "hands_loss_light_f32": [C.POINTER(LossIn), _I, _I, _I, _P, _P, _P, _P, _P],
    "hands_mano_pose_aa_f32": [C.POINTER(ManoConsts), _P, _P, _I, _P, _I, _P, _P, _I, _P],
    "hands_gt_targets_f32": [_P, _P, _P, _P, _F, _P, _P, _P, _I, _I, _P],
    "hands_unnormalize_kp2d_f32": [_P, _P, C.c_longlong, _F, _P],
    "hands_frontend_boxes_f32": [_P, _P, _I, _P, _I, _I, _I, C.c_double] + [_P] * 10 + [_P],
    "hands_warp_affine_cubic_norm_f32": [_P, _P, _P, _I, _I, _I, _I, _I, C.POINTER(C.c_float), C.POINTER(C.c_float), _P],
    "hands_render_silhouette_f32": [_P, _I, _I, _P, _I, _P, _I, _I, _F, _F, _I, _P, _P, _P, _P],
    "hands_mesh_prepare_f32": [_P, _I, _I, _P, _I, _P, _P, _P, _P, _I, _I, _P, _P],
    "hands_render_shaded_f32": [C.POINTER(ShadeScene), _P, _I, _I, _P, _P, _P, _P, _P],
    # host-side packing (csrc/pack.cpp): HOST pointers
    "hands_pack_conv_dims": [_I, _I, _I, _I, _I, C.POINTER(PackedDims)],
    "hands_fold_bn_f32": [_I, C.c_longlong, _P, _P, _P, _P, _P, C.c_double, _P, _P],
    "hands_pack_conv_f64": [_I, _I, _I, _I, _I, _P, _P, _P, _P],
    "hands_pack_linear_f64": [_I, _I, _P, _P, _P, _I, _P, _I, _P, _P],
    "hands_pack_conv1x1_dual_f64": [_I, _I, _I, _P, _P, _P, _P, _P, _P],
    "hands_pack_mano_f32": [_P] * 10,
    "hands_pack_conv3x3_winograd_f64": [_I, _I, _P, _P],
    "hands_pack_conv3x3_winograd4_f64": [_I, _I, _P, _P],
}
EXTRA_SYMBOLS = ("hands_abi_version", "hands_error_string", "hands_conv2d_workspace_floats", "hands_pack_conv3x3_winograd_floats", "hands_conv3x3_winograd_executed_macs",
                 "hands_pack_conv3x3_winograd4_floats", "hands_conv3x3_winograd4_executed_macs",
                 "hands_conv2d_streamk_workspace_bytes", "hands_stream_is_capturing", "hands_csrc_sha16", "hands_ceiling_mfma_f32", "hands_mesh_workspace_floats",
                 "hands_loss_workspace_bytes", "hands_smooth_state_bytes")

ABI_VERSION = 5      # HANDS_ABI_VERSION of include/hands_hip.h this wrapper was written against
_lib = None


def lib():
    """Load (once) and return the shared library; raise if it is not there."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise RuntimeError(
            f"hands_amd: {LIB_PATH} not found. Build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` or `make -C hands_amd/csrc`. There is no CPU fallback.")
    h = C.CDLL(LIB_PATH)
    h.hands_abi_version.restype = C.c_int
    if h.hands_abi_version() != ABI_VERSION:
        # a stale build (e.g. an A/B variant through $HANDS_HIP_LIB) would otherwise fail late with an AttributeError
        raise RuntimeError(f"hands_amd: {LIB_PATH} has ABI version {h.hands_abi_version()}, this package needs {ABI_VERSION}: "
                           "rebuild it (`make -C hands_amd/csrc`)")
    for name, argtypes in SIGNATURES.items():
        fn = getattr(h, name)
        fn.argtypes = argtypes
        fn.restype = C.c_int
    h.hands_conv2d_workspace_floats.restype = C.c_longlong
    h.hands_conv2d_workspace_floats.argtypes = [C.POINTER(ConvDesc), C.c_int]
    h.hands_conv2d_streamk_workspace_bytes.restype = C.c_longlong
    h.hands_conv2d_streamk_workspace_bytes.argtypes = []
    h.hands_pack_conv3x3_winograd_floats.restype = C.c_longlong
    h.hands_pack_conv3x3_winograd_floats.argtypes = [C.c_int, C.c_int]
    h.hands_conv3x3_winograd_executed_macs.restype = C.c_longlong
    h.hands_conv3x3_winograd_executed_macs.argtypes = [C.POINTER(ConvDesc)]
    h.hands_pack_conv3x3_winograd4_floats.restype = C.c_longlong
    h.hands_pack_conv3x3_winograd4_floats.argtypes = [C.c_int, C.c_int]
    h.hands_conv3x3_winograd4_executed_macs.restype = C.c_longlong
    h.hands_conv3x3_winograd4_executed_macs.argtypes = [C.POINTER(ConvDesc)]
    h.hands_abi_version.restype = C.c_int
    h.hands_stream_is_capturing.restype = C.c_int
    h.hands_stream_is_capturing.argtypes = [C.c_void_p]
    h.hands_csrc_sha16.restype = C.c_char_p
    h.hands_csrc_sha16.argtypes = []
    h.hands_ceiling_mfma_f32.restype = C.c_longlong
    h.hands_ceiling_mfma_f32.argtypes = [C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_void_p]
    h.hands_mesh_workspace_floats.restype = C.c_longlong
    h.hands_mesh_workspace_floats.argtypes = [C.c_int, C.c_int]
    h.hands_loss_workspace_bytes.restype = C.c_longlong
    h.hands_loss_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
    h.hands_smooth_state_bytes.restype = C.c_longlong
    h.hands_smooth_state_bytes.argtypes = []
    h.hands_error_string.restype = C.c_char_p
    h.hands_error_string.argtypes = [C.c_int]
    _lib = h
    return h


def check(code: int, what: str = ""):
    if code != 0:
        msg = lib().hands_error_string(code).decode()
        raise RuntimeError(f"hands_amd: {what} failed with code {code}: {msg}")


def ptr(t, offset_elems: int = 0):
    """Device pointer of a torch tensor (optionally offset by elements), or None."""
    if t is None:
        return None
    return t.data_ptr() + offset_elems * t.element_size()
