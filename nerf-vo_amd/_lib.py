"""ctypes binding of libnerfvo_hip.so (C-ABI declared in include/nerfvo_hip.h).

No torch types cross this boundary: tensors are passed as raw device pointers (``Tensor.data_ptr()``)
and the stream as ``torch.cuda.current_stream().cuda_stream``.  The product path has NO fallback:
if the library is missing or a call fails, a RuntimeError is raised.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

PKG_DIR = Path(__file__).resolve().parent
LIB_PATH = PKG_DIR / "lib" / "libnerfvo_hip.so"

_lib = None

# name -> (restype, argtypes); mirrors include/nerfvo_hip.h one to one
_u32, _u64, _i64, _int = C.c_uint32, C.c_uint64, C.c_int64, C.c_int
_i32 = C.c_int32
_p = C.c_void_p
_f = C.c_float


class WeightsPdfArgs(C.Structure):
    """mirror of nvo_weights_pdf_args"""
    _fields_ = [("R", _u32), ("S", _u32), ("S_out", _u32), ("pre", _p), ("pre_stride", _u32), ("x01", _p),
                ("sbins", _p), ("tbins", _p), ("density_bias", _f), ("sigma", _p), ("weights", _p),
                ("anneal", _f), ("histogram_padding", _f), ("near_plane", _f), ("far_plane", _f),
                ("jitter", _p), ("sbins_out", _p), ("tbins_out", _p), ("anneal_dev", _p),
                ("origins", _p), ("directions", _p), ("x01_out", _p), ("act_bf16", _int)]


class MainLossArgs(C.Structure):
    """mirror of nvo_main_loss_args"""
    _fields_ = [("R", _u32), ("S", _u32), ("pre", _p), ("pre_stride", _u32), ("rgb", _p), ("rgb_stride", _u32),
                ("x01", _p), ("sbins", _p), ("tbins", _p), ("density_bias", _f), ("gt_rgb", _p),
                ("gt_depth", _p), ("directions_norm", _p), ("rgb_mult", _f), ("distortion_mult", _f),
                ("depth_mult", _f), ("depth_sigma", _f), ("inv_rays", _f), ("depth_level_div", _f),
                ("loss_scale", _f), ("out_rgb", _p), ("out_depth", _p), ("out_expected_depth", _p),
                ("out_accumulation", _p), ("weights", _p), ("losses", _p), ("dpre", _p), ("dpre_stride", _u32),
                ("drgb", _p), ("drgb_stride", _u32),
                ("dsigma_dx", _p), ("dsigma_inv_scale", _f), ("gt_normal", _p), ("normal_mult", _f),
                ("out_normals", _p), ("act_bf16", _int), ("loss_scale_dev", _p), ("nonfinite_flag", _p),
                ("tile_live", _p)]


class PropLossArgs(C.Structure):
    """mirror of nvo_prop_loss_args"""
    _fields_ = [("R", _u32), ("S", _u32), ("S_main", _u32), ("pre", _p), ("pre_stride", _u32), ("x01", _p),
                ("sbins", _p), ("tbins", _p), ("sbins_main", _p), ("weights_main", _p), ("density_bias", _f),
                ("gt_depth", _p), ("directions_norm", _p), ("interlevel_mult", _f), ("depth_mult", _f),
                ("depth_sigma", _f), ("inv_rays", _f), ("depth_level_div", _f), ("loss_scale", _f),
                ("losses", _p), ("dpre", _p), ("dpre_stride", _u32), ("act_bf16", _int), ("loss_scale_dev", _p),
                ("nonfinite_flag", _p)]


class ColorArgs(C.Structure):
    """mirror of nvo_color_args"""
    _fields_ = [("R", _u32), ("S", _u32), ("sh", _p), ("base_out", _p), ("embedding", _p), ("cam_idx", _p),
                ("weights", _p), ("rgb", _p), ("hidden", _p), ("drgb", _p), ("d_base_out", _p),
                ("d_embedding", _p), ("d_sh", _p), ("d_weights", _p), ("act_bf16", _int), ("det_scratch", _p),
                ("det_scratch_bytes", _u64), ("n_cameras", _u32), ("nonfinite_flag", _p), ("dw_replicas", _p),
                ("n_dw_replicas", _u32), ("tile_live", _p), ("tile_live_count", _p)]


class RayHeadArgs(C.Structure):
    """mirror of nvo_ray_head_args"""
    _fields_ = [("R", _u32), ("S", _u32), ("seed", _u32), ("n_jitter", _u32), ("step_dev", _p), ("extent_dev", _p),
                ("intrinsics", _p), ("c2w", _p), ("c2w_stride", _u32), ("corrections", _p), ("H", _u32), ("W", _u32),
                ("images", _p), ("depths", _p), ("normals", _p), ("near_plane", _f), ("far_plane", _f),
                ("ray_indices", _p), ("jitter", _p), ("origins", _p), ("directions", _p), ("directions_norm", _p),
                ("pixel_area", _p), ("cam_idx", _p), ("gt_rgb", _p), ("gt_depth", _p), ("gt_normal", _p), ("dirs01", _p),
                ("sh", _p), ("sh_bf16", _int), ("sbins", _p), ("tbins", _p), ("x01", _p)]


class FusedAdamArgs(C.Structure):
    """nvo_fused_adam_args (include/nerfvo_hip.h): optimiser step inside a hash grid's parameter backward."""
    _fields_ = [("params", _p), ("params_half", _p), ("exp_avg", _p), ("exp_avg_sq", _p), ("hyper_dev", _p),
                ("bias_dev", _p), ("loss_scale_dev", _p), ("skip_flag", _p), ("lr", _f), ("grad_scale", _f),
                ("beta1", _f), ("beta2", _f), ("eps", _f), ("step", _u32), ("ema", _p), ("ema_half", _p), ("ema_decay", _f),
                ("ema_step_dev", _p)]


class AdamGroup(C.Structure):
    """mirror of nvo_adam_group"""
    _fields_ = [("offset", _u64), ("n", _u64), ("lr", _f), ("step", _u32), ("hyper_dev", _p), ("bias_dev", _p),
                ("flag_slot", _u32), ("weight_decay", _f)]


class OptCommitArgs(C.Structure):
    """mirror of nvo_opt_commit_args"""
    _fields_ = [("n_groups", _u32), ("active_mask", _u32), ("scale_mask", _u32), ("applied", _p), ("skip_flags", _p),
                ("scale", _p), ("growth_tracker", _p), ("growth_factor", _f), ("backoff_factor", _f),
                ("growth_interval", _u32), ("min_scale", _f), ("max_scale", _f), ("bias", _p), ("beta1", _f), ("beta2", _f)]


class AdamTail(C.Structure):
    """mirror of nvo_adam_tail"""
    _fields_ = [("ema", _p), ("ema_half", _p), ("ema_decay", _f), ("ema_step_dev", _p), ("ema_flag_slot", _u32),
                ("ema_commit", _u32), ("done_counter", _p), ("commit", OptCommitArgs)]


class AdamArgs(C.Structure):
    """mirror of nvo_adam_args"""
    _fields_ = [("params", _p), ("params_half", _p), ("grads", _p), ("grads_fmt", _int), ("exp_avg", _p),
                ("exp_avg_sq", _p), ("beta1", _f), ("beta2", _f), ("eps", _f), ("grad_scale", _f), ("skip_flags", _p),
                ("loss_scale_dev", _p), ("n_bf16_ranges", _u32), ("bf16_lo", _p), ("bf16_hi", _p)]


class StepScalars(C.Structure):
    """mirror of nvo_step_scalars"""
    _fields_ = [("dst", _p), ("n", _u32), ("host_values", _p), ("table", _p), ("table_rows", _u32), ("next_step", _p)]


class DepthAlignArgs(C.Structure):
    """mirror of nvo_depth_align_args"""
    _fields_ = [("K", _u32), ("M", _u32), ("P", _u32), ("H", _u32), ("W", _u32), ("patches", _p), ("noise", _p),
                ("frames_depth", _p), ("out_depth", _p), ("scratch", _p), ("scale_shift_out", _p)]


class NgpRgbArgs(C.Structure):
    """mirror of nvo_ngp_rgb_args"""
    _fields_ = [("capacity", _u32), ("sh", _p), ("density_out", _p), ("ray_idx", _p), ("weights", _p), ("rgb_out", _p),
                ("hidden", _p), ("d_rgb_out", _p), ("d_density_out", _p), ("d_density_pre", _p), ("d_weights", _p),
                ("nonfinite_flag", _p), ("dw_replicas", _p), ("n_dw_replicas", _u32)]


class NgpLossArgs(C.Structure):
    """mirror of nvo_ngp_loss_args"""
    _fields_ = [("R", _u32), ("capacity", _u32), ("counts", _p), ("offsets", _p), ("ray_idx", _p), ("t", _p), ("dt", _p),
                ("density_out", _p), ("density_stride", _u32), ("rgb_out", _p), ("rgb_stride", _u32),
                ("background", _p), ("gt_rgb", _p), ("gt_depth", _p), ("directions_norm", _p), ("rgb_mult", _f),
                ("depth_mult", _f), ("inv_rays", _f), ("loss_scale", _f), ("out_rgb", _p), ("out_depth", _p),
                ("out_accumulation", _p), ("losses", _p), ("d_rgb_out", _p), ("d_rgb_stride", _u32),
                ("d_density_pre", _p), ("carry_in", _p), ("carry_out", _p), ("accumulate_outputs", _u32),
                ("train_min_transmittance", _f), ("gt_depth_cov", _p), ("ray_state", _p), ("R_dev", _p), ("world_size", _u32)]


class NgpAliveArgs(C.Structure):
    """mirror of nvo_ngp_alive_args"""
    _fields_ = [("R", _u32), ("counts", _p), ("offsets", _p), ("dt", _p), ("density_out", _p), ("density_stride", _u32),
                ("min_transmittance", _f), ("kept", _p), ("state", _p), ("R_dev", _p), ("resume_in", _p), ("carry_in", _p),
                ("kept_base", _u32), ("t_next", _p), ("resume_out", _p), ("carry_out", _p)]


class NgpNormalArgs(C.Structure):
    """mirror of nvo_ngp_normal_args"""
    _fields_ = [("R", _u32), ("capacity", _u32), ("counts", _p), ("offsets", _p), ("t", _p), ("dt", _p), ("density_out", _p),
                ("density_stride", _u32), ("dx01", _p), ("origins", _p), ("directions", _p), ("aabb_lo", _f), ("aabb_hi", _f),
                ("carry_in", _p), ("accumulate", _u32), ("out_normal", _p)]


class TsdfArgs(C.Structure):
    """mirror of nvo_tsdf_args"""
    _fields_ = [("tsdf", _p), ("weight", _p), ("color", _p), ("frames", _p), ("depth", _p), ("rgb", _p),
                ("nx", _u32), ("ny", _u32), ("nz", _u32), ("K", _u32), ("H", _u32), ("W", _u32),
                ("lower_x", _f), ("lower_y", _f), ("lower_z", _f), ("voxel_size", _f), ("trunc", _f), ("depth_max", _f)]


TSDF_MAX_FRAMES = 16  # NVO_TSDF_MAX_FRAMES


class NnArgs(C.Structure):
    """mirror of nvo_nn_args"""
    _fields_ = [("points", _p), ("point_index", _p), ("cell_start", _p), ("queries", _p), ("out_dist2", _p), ("out_index", _p),
                ("N", _u32), ("M", _u32), ("gx", _u32), ("gy", _u32), ("gz", _u32),
                ("lower_x", _f), ("lower_y", _f), ("lower_z", _f), ("cell_size", _f), ("max_dist", _f),
                ("has_xf", _i32), ("xf", _f * 12)]


NN_MAX_CELLS_PER_AXIS = 1024  # NVO_NN_MAX_CELLS_PER_AXIS


class KnnArgs(C.Structure):
    """mirror of nvo_knn_args"""
    _fields_ = [("points", _p), ("point_index", _p), ("cell_start", _p), ("queries", _p), ("out_dist2", _p), ("out_index", _p),
                ("out_mean_dist", _p), ("N", _u32), ("M", _u32), ("k", _u32), ("gx", _u32), ("gy", _u32), ("gz", _u32),
                ("lower_x", _f), ("lower_y", _f), ("lower_z", _f), ("cell_size", _f)]


KNN_MAX_K = 32  # NVO_KNN_MAX_K


class IsoArgs(C.Structure):
    """mirror of nvo_iso_args"""
    _fields_ = [("values", _p), ("valid", _p), ("scratch", _p), ("vertex_base", _p), ("face_base", _p), ("vertices", _p),
                ("faces", _p), ("n_vertices", _u64), ("n_faces", _u64), ("nx", _u32), ("ny", _u32), ("nz", _u32),
                ("points_per_workgroup", _u32), ("threshold", _f), ("lower", _f * 3), ("step", _f * 3)]


ISO_DEFAULT_POINTS_PER_WORKGROUP = 4096  # NVO_ISO_DEFAULT_POINTS_PER_WORKGROUP


class LatticeArgs(C.Structure):
    """mirror of nvo_lattice_args"""
    _fields_ = [("positions", _p), ("first", _u64), ("count", _u32), ("nx", _u32), ("ny", _u32), ("nz", _u32),
                ("lower", _f * 3), ("step", _f * 3)]


class PoissonSplatArgs(C.Structure):
    """mirror of nvo_poisson_splat_args"""
    _fields_ = [("points", _p), ("cell_start", _p), ("values", _p), ("denom", _p), ("out", _p), ("K", _u32), ("channels", _u32),
                ("nx", _u32), ("ny", _u32), ("nz", _u32), ("origin", _f * 3), ("h", _f)]


class PoissonSampleArgs(C.Structure):
    """mirror of nvo_poisson_sample_args"""
    _fields_ = [("field", _p), ("points", _p), ("out", _p), ("K", _u32), ("channels", _u32), ("nx", _u32), ("ny", _u32),
                ("nz", _u32), ("origin", _f * 3), ("h", _f)]


class PoissonLevelArgs(C.Structure):
    """mirror of nvo_poisson_level_args"""
    _fields_ = [("chi", _p), ("rhs", _p), ("field", _p), ("coarse", _p), ("norm_bits", _p), ("nx", _u32), ("ny", _u32),
                ("nz", _u32), ("color", _u32)]


class PoissonVcycleArgs(C.Structure):
    """mirror of nvo_poisson_vcycle_args"""
    _fields_ = [("chi", _p), ("rhs", _p), ("scratch", _p), ("nx", _u32), ("ny", _u32), ("nz", _u32), ("levels", _u32)]


POISSON_MAX_NODES_PER_AXIS = 4097  # NVO_POISSON_MAX_NODES_PER_AXIS


class TsdfBlocksArgs(C.Structure):
    """mirror of nvo_tsdf_blocks_args"""
    _fields_ = [("table", _p), ("tsdf", _p), ("weight", _p), ("color", _p), ("frames", _p), ("touch_frames", _p), ("depth", _p),
                ("rgb", _p), ("marks", _p), ("list", _p), ("list_mask", _p), ("n_list", _u32), ("n_allocated", _u32),
                ("tbx", _u32), ("tby", _u32), ("tbz", _u32), ("K", _u32), ("H", _u32), ("W", _u32), ("n_samples", _u32),
                ("lower_x", _f), ("lower_y", _f), ("lower_z", _f), ("voxel_size", _f), ("trunc", _f), ("depth_max", _f)]


class TsdfBlocksIsoArgs(C.Structure):
    """mirror of nvo_tsdf_blocks_iso_args"""
    _fields_ = [("table", _p), ("tsdf", _p), ("weight", _p), ("color", _p), ("order", _p), ("totals", _p), ("vrank", _p),
                ("mask", _p), ("tcount", _p), ("vertex_base", _p), ("face_base", _p), ("vertices", _p), ("colors", _p),
                ("faces", _p), ("n_vertices", _u64), ("n_faces", _u64), ("n_blocks", _u32), ("n_allocated", _u32),
                ("tbx", _u32), ("tby", _u32), ("tbz", _u32), ("weight_threshold", _f), ("lower", _f * 3), ("voxel_size", _f)]


TSDF_BLOCK = 8                          # NVO_TSDF_BLOCK
TSDF_BLOCKS_MAX_TABLE = 1 << 26         # NVO_TSDF_BLOCKS_MAX_TABLE
TSDF_BLOCKS_MAX_ALLOCATED = 1 << 22     # NVO_TSDF_BLOCKS_MAX_ALLOCATED


class M2dColorArgs(C.Structure):
    """mirror of nvo_m2d_color_args"""
    _fields_ = [("a", _p), ("b", _p), ("table", _p), ("scratch", _p), ("F", _u32), ("H", _u32), ("W", _u32), ("is_float", _i32),
                ("taps", _f * 11)]


class M2dDepthArgs(C.Structure):
    """mirror of nvo_m2d_depth_args"""
    _fields_ = [("gt", _p), ("pred", _p), ("table", _p), ("scratch", _p), ("F", _u32), ("H", _u32), ("W", _u32),
                ("gt_f64", _i32), ("pred_f64", _i32), ("with_scale", _i32)]


M2D_TILE_H = 32        # NVO_M2D_TILE_H
M2D_TILE_W = 32        # NVO_M2D_TILE_W
M2D_TAPS = 11          # NVO_M2D_TAPS
M2D_COLOR_WORDS = 3    # NVO_M2D_COLOR_WORDS
M2D_DEPTH_WORDS = 9    # NVO_M2D_DEPTH_WORDS


class LpipsConvArgs(C.Structure):
    """mirror of nvo_lpips_conv_args"""
    _fields_ = [("x", _p), ("weights", _p), ("bias", _p), ("out", _p), ("F", _u32), ("Cin", _u32), ("H", _u32), ("W", _u32),
                ("Cout", _u32), ("ksize", _u32), ("stride", _u32), ("pad", _u32), ("Kpad", _u32), ("ingest", _i32),
                ("shift", _f * 3), ("scale", _f * 3)]


class LpipsPoolArgs(C.Structure):
    """mirror of nvo_lpips_pool_args"""
    _fields_ = [("x", _p), ("out", _p), ("planes", _u32), ("H", _u32), ("W", _u32)]


class LpipsHeadArgs(C.Structure):
    """mirror of nvo_lpips_head_args"""
    _fields_ = [("f0", _p), ("f1", _p), ("lin", _p), ("map", _p), ("scratch", _p), ("out", _p), ("F", _u32), ("C", _u32),
                ("HW", _u32), ("accumulate", _i32)]


LPIPS_TILE_M = 64        # NVO_LPIPS_TILE_M
LPIPS_TILE_N = 128       # NVO_LPIPS_TILE_N
LPIPS_TILE_K = 16        # NVO_LPIPS_TILE_K
LPIPS_HEAD_BLOCK = 256   # NVO_LPIPS_HEAD_BLOCK


class BaArgs(C.Structure):
    """mirror of nvo_ba_args"""
    _fields_ = [("poses", _p), ("disps", _p), ("intrinsics", _f * 4), ("target", _p), ("weight", _p), ("eta", _p),
                ("coords", _p), ("valid", _p), ("B", _p), ("v", _p), ("C", _p), ("wz", _p), ("Q", _p), ("Ei", _p), ("Ej", _p),
                ("Ehat", _p), ("S", _p), ("g", _p), ("prior_weight", C.c_double), ("dx", _p), ("Mx", _p), ("status", _p),
                ("cov", _p)]


BA_MAX_NATIVE_N = 192    # NVO_BA_MAX_NATIVE_N


_SIGNATURES = {
    "nvo_last_error": (C.c_char_p, []),
    "nvo_version": (_int, []),
    "nvo_profile_enable": (_int, [_int]),
    "nvo_profile_summary": (_i64, [C.c_char_p, _u64]),
    "nvo_create_encoding": (_int, [_u32, C.c_char_p, C.POINTER(_p)]),
    "nvo_create_network": (_int, [_u32, _u32, C.c_char_p, C.POINTER(_p)]),
    "nvo_create_network_with_input_encoding": (_int, [_u32, _u32, C.c_char_p, C.c_char_p, C.POINTER(_p)]),
    "nvo_destroy": (_int, [_p]),
    "nvo_n_input_dims": (_u32, [_p]),
    "nvo_n_output_dims": (_u32, [_p]),
    "nvo_padded_output_dims": (_u32, [_p]),
    "nvo_n_params": (_u64, [_p]),
    "nvo_initial_params": (_int, [_p, _u64, _p]),
    "nvo_ctx_bytes": (_u64, [_p, _u32]),
    "nvo_set_option": (_int, [_p, C.c_char_p, _i64]),
    "nvo_fwd": (_int, [_p, _p, _u32, _p, _p, _p, _p]),
    "nvo_bwd": (_int, [_p, _p, _u32, _p, _p, _p, _p, _p, _p, _p]),
    "nvo_bwd_fork": (_int, [_p, _p, _p, _u32, _p, _p, _p, _p, _p, _p, _p]),
    "nvo_grid_describe": (_int, [_p, _p, _p]),
    "nvo_grid_indices": (_int, [_p, _p, _u32, _p, _p]),
    # group B
    "nvo_raygen": (_int, [_p, _u32, _p, _p, _p, _p, _p, _p, _p, _p, _p]),
    "nvo_se3_exp_map": (_int, [_p, _u32, _p, _p]),
    "nvo_pose_exp_map": (_int, [_p, _u32, _p, _p, _int]),
    "nvo_positions_bwd": (_int, [_p, _u32, _u32, _p, _p, _p, _p, _p, _p]),
    "nvo_sh_bwd_input_f32": (_int, [_p, _u32, _u32, _p, _p, _p]),
    "nvo_pose_bwd": (_int, [_p, _u32, _p, _p, _p, _p, _p, _p, _p]),
    "nvo_se3_exp_map_bwd": (_int, [_p, _u32, _p, _p, _f, _f, _f, _p, _p, _int]),
    "nvo_se3_exp_map_bwd_scaled": (_int, [_p, _u32, _p, _p, _f, _f, _f, _p, _p, _int, _p]),
    "nvo_gather_pixels": (_int, [_p, _u32, _p, _u32, _u32, _u32, _p, _p]),
    "nvo_sample_lindisp": (_int, [_p, _u32, _u32, _f, _f, _p, _p, _p]),
    "nvo_sample_pixels": (_int, [_p, _u32, _u32, _p, _p, _p, _p, _u32]),
    "nvo_lindisp_positions": (_int, [_p, _u32, _u32, _f, _f, _p, _p, _p, _p, _p, _p]),
    "nvo_gather_targets": (_int, [_p, _u32, _p, _u32, _u32, _p, _p, _p, _p, _p, _p, _p, _p]),
    "nvo_sample_positions": (_int, [_p, _u32, _u32, _p, _p, _p, _p]),
    "nvo_dirs01": (_int, [_p, _u32, _p, _p]),
    "nvo_sh_encode": (_int, [_p, _u32, _u32, _p, _p]),
    "nvo_sh_encode_t": (_int, [_p, _u32, _u32, _p, _p, _int]),
    "nvo_ray_head": (_int, [_p, C.POINTER(RayHeadArgs)]),
    "nvo_rays_given": (_int, [_p, _u32, _p, _p, _p, _p, _u32, _u32, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p]),
    "nvo_ray_head_zero": (_int, [_p, C.POINTER(RayHeadArgs), _u32, _p, _p]),
    # group C
    "nvo_weights_pdf": (_int, [_p, C.POINTER(WeightsPdfArgs)]),
    "nvo_main_render_loss": (_int, [_p, C.POINTER(MainLossArgs)]),
    "nvo_prop_loss": (_int, [_p, C.POINTER(PropLossArgs)]),
    "nvo_prop_loss_pair": (_int, [_p, _p, _p]),
    # group D
    "nvo_nerfacto_color_fwd": (_int, [_p, C.POINTER(ColorArgs)]),
    "nvo_nerfacto_color_bwd": (_int, [_p, C.POINTER(ColorArgs)]),
    "nvo_color_det_scratch_bytes": (_u64, [_u32, _u32]),
    "nvo_pose_bwd_cams": (_int, [_p, _u32, _p, _p, _p, _p, _p, _p, _p, _u32]),
    "nvo_pose_bwd_det": (_int, [_p, _u32, _p, _p, _p, _p, _p, _p, _p, _p, _u32]),
    # group F
    "nvo_occ_march_scratch_bytes": (_u64, [_u32]),
    "nvo_occ_march": (_int, [_p, _u32, _p, _p, _p, _int, _f, _f, _p, _u32, _p, _p, _p, _p, _p, _p, _u64]),
    "nvo_occ_march_resume": (_int, [_p, _u32, _p, _p, _p, _int, _f, _f, _p, _u32, _p, _p, _p, _p, _p, _p, _u64, _p, _u32, _p]),
    "nvo_occ_update": (_int, [_p, _int, _p, _p, _f, _f, _p, _p]),
    "nvo_occ_cell_positions": (_int, [_p, _int, _p, _p]),
    "nvo_occ_mark_untrained": (_int, [_p, _int, _p, _u32, _p, _p, _u32, _u32, _f]),
    "nvo_occ_sample_cells": (_int, [_p, _u32, _u32, _u32, _u32, _u32, _u32, _int, _p, _f, _f, _f, _p, _p]),
    "nvo_occ_march_runs": (_int, [_p, _u32, _p, _p, _p, _int, _f, _f, _p, _p, _p, _u64, _p, _u32, _p, _p, _u32]),
    "nvo_occ_pack": (_int, [_p, _u32, _p, _u32, _p, _p, _p, _p, _u64, _p, _p, _p, _p, _u32]),
    "nvo_occ_pack_state_bytes": (_u64, []),
    "nvo_occ_pack_fused": (_int, [_p, _u32, _p, _u32, _p, _p, _p, _p, _u64, _p, _p, _p, _p, _u32, _p, _p, _p, _f, _f, _p, _u32]),
    "nvo_ngp_count_alive": (_int, [_p, C.POINTER(NgpAliveArgs)]),
    "nvo_ngp_positions_live": (_int, [_p, _u32, _p, _p, _p, _p, _f, _f, _p, _p]),
    "nvo_ngp_positions_bwd_dev": (_int, [_p, _u32, _u32, _p, _p, _p, _p, _p, _f, _f, _p, _p, _p, _p]),
    "nvo_ngp_positions": (_int, [_p, _u32, _p, _p, _p, _p, _f, _f, _p]),
    "nvo_depth_align_scratch_bytes": (_u64, [_u32, _u32]),
    "nvo_depth_align": (_int, [_p, C.POINTER(DepthAlignArgs)]),
    "nvo_ngp_positions_bwd": (_int, [_p, _u32, _u32, _p, _p, _p, _p, _p, _f, _f, _p, _p, _p]),
    "nvo_ngp_rgb_fwd": (_int, [_p, C.POINTER(NgpRgbArgs)]),
    "nvo_ngp_rgb_bwd": (_int, [_p, C.POINTER(NgpRgbArgs)]),
    "nvo_ngp_composite_loss": (_int, [_p, C.POINTER(NgpLossArgs)]),
    "nvo_ngp_thickness": (_int, [_p, _u32, _p, _u32, _int, _p]),
    "nvo_ngp_thickness_splat": (_int, [_p, _u32, _p, _u32, _p, _p]),
    "nvo_fill_i32": (_int, [_p, _u32, _p, _i32]),
    "nvo_ngp_normal_seed": (_int, [_p, _u32, _f, _p]),
    "nvo_ngp_composite_normals": (_int, [_p, C.POINTER(NgpNormalArgs)]),
    # group H
    "nvo_tsdf_integrate": (_int, [_p, C.POINTER(TsdfArgs)]),
    # group I
    "nvo_nn_query": (_int, [_p, C.POINTER(NnArgs)]),
    # group J
    "nvo_iso_workgroups": (_u64, [_u32, _u32, _u32, _u32]),
    "nvo_iso_scratch_bytes": (_u64, [_u32, _u32, _u32, _u32]),
    "nvo_iso_count": (_int, [_p, C.POINTER(IsoArgs)]),
    "nvo_iso_emit": (_int, [_p, C.POINTER(IsoArgs)]),
    "nvo_lattice_positions": (_int, [_p, C.POINTER(LatticeArgs)]),
    # group K
    "nvo_knn_query": (_int, [_p, C.POINTER(KnnArgs)]),
    # group L
    "nvo_poisson_splat": (_int, [_p, C.POINTER(PoissonSplatArgs)]),
    "nvo_poisson_sample": (_int, [_p, C.POINTER(PoissonSampleArgs)]),
    "nvo_poisson_divergence": (_int, [_p, C.POINTER(PoissonLevelArgs)]),
    "nvo_poisson_sweep": (_int, [_p, C.POINTER(PoissonLevelArgs)]),
    "nvo_poisson_restrict": (_int, [_p, C.POINTER(PoissonLevelArgs)]),
    "nvo_poisson_prolong": (_int, [_p, C.POINTER(PoissonLevelArgs)]),
    "nvo_poisson_residual_norm": (_int, [_p, C.POINTER(PoissonLevelArgs)]),
    "nvo_poisson_vcycle_scratch_bytes": (_u64, [_u32, _u32, _u32, _u32]),
    "nvo_poisson_vcycle": (_int, [_p, C.POINTER(PoissonVcycleArgs)]),
    # group M
    "nvo_tsdf_blocks_touch": (_int, [_p, C.POINTER(TsdfBlocksArgs)]),
    "nvo_tsdf_blocks_integrate": (_int, [_p, C.POINTER(TsdfBlocksArgs)]),
    "nvo_tsdf_blocks_iso_count": (_int, [_p, C.POINTER(TsdfBlocksIsoArgs)]),
    "nvo_tsdf_blocks_iso_emit": (_int, [_p, C.POINTER(TsdfBlocksIsoArgs)]),
    # group N
    "nvo_m2d_color_scratch_bytes": (_u64, [_u32, _u32, _u32]),
    "nvo_m2d_color": (_int, [_p, C.POINTER(M2dColorArgs)]),
    "nvo_m2d_depth_chunks": (_u32, [_u32, _u32]),
    "nvo_m2d_depth_scratch_bytes": (_u64, [_u32, _u32, _u32]),
    "nvo_m2d_depth": (_int, [_p, C.POINTER(M2dDepthArgs)]),
    # group O
    "nvo_lpips_conv_kpad": (_u32, [_u32]),
    "nvo_lpips_conv": (_int, [_p, C.POINTER(LpipsConvArgs)]),
    "nvo_lpips_pool": (_int, [_p, C.POINTER(LpipsPoolArgs)]),
    "nvo_lpips_head_scratch_bytes": (_u64, [_u32, _u32, _u32]),
    "nvo_lpips_head": (_int, [_p, C.POINTER(LpipsHeadArgs)]),
    # group P
    "nvo_ba_plan_create": (_int, [_p, _p, _u32, _u32, _u32, _u32, _u32, _u32, C.POINTER(_p)]),
    "nvo_ba_plan_destroy": (_int, [_p]),
    "nvo_ba_plan_bytes": (_u64, [_p]),
    "nvo_ba_plan_kx": (_u32, [_p, _p]),
    "nvo_ba_plan_bind": (_int, [_p, _p, _p, _u64]),
    "nvo_ba_reproject": (_int, [_p, _p, C.POINTER(BaArgs)]),
    "nvo_ba_accumulate": (_int, [_p, _p, C.POINTER(BaArgs)]),
    "nvo_ba_schur": (_int, [_p, _p, C.POINTER(BaArgs)]),
    "nvo_ba_solve": (_int, [_p, _u32, _p, _p, _p, _p, _p, _p]),
    "nvo_ba_update": (_int, [_p, _p, C.POINTER(BaArgs)]),
    "nvo_ba_covariance": (_int, [_p, _p, C.POINTER(BaArgs)]),
    # group E
    "nvo_adam_step": (_int, [_p, C.POINTER(AdamArgs), _u32, C.POINTER(AdamGroup), C.POINTER(AdamTail)]),
    "nvo_opt_commit": (_int, [_p, C.POINTER(OptCommitArgs), C.POINTER(StepScalars)]),
    "nvo_nonfinite_flag": (_int, [_p, _u32, _p, _p, _p, _p, _int, _p, _int]),
    "nvo_ema_update": (_int, [_p, _u64, _p, _p, _p, _f, _p, _p, _int]),
    "nvo_write_floats": (_int, [_p, _p, _u32, _p]),
    "nvo_cast_half": (_int, [_p, _u64, _p, _p]),
    "nvo_cast_bf16": (_int, [_p, _u64, _p, _p]),
    "nvo_cast_working_copy": (_int, [_p, _u64, _p, _p, _u32, _p, _p]),
    "nvo_cast_shards": (_int, [_p, _u64, _u32, _u32, _p, _p, _int, _p]),
    "nvo_flag_from_wire": (_int, [_p, _p, _p]),
    "nvo_zero_ranges": (_int, [_p, _u32, _p, _p]),
    "nvo_bwd_zero_ranges": (_int, [_p, _p, _p, _p, _u32]),
    "nvo_fold_replicas": (_int, [_p, _u32, _p, _p, _p, _p]),
    "nvo_fused_adam_range": (_int, [_p, _p, _p]),
    "nvo_set_fused_adam": (_int, [_p, _p]),
}


def exported_symbols() -> list[str]:
    return sorted(_SIGNATURES)


def lib() -> C.CDLL:
    """Load (once) and return the native library; raise if it has not been built."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise RuntimeError(
                f"{LIB_PATH} is missing: the HIP extension has not been built. "
                "Run `python -c 'import __graft_entry__ as g; g.build()'` (or `python nerf-vo_amd/build.py`). "
                "There is no CPU fallback."
            )
        # PyTorch bundles its own libamdhip64.so.7 (+ HSA runtime); this library is linked against the
        # SONAME only.  Whichever copy is loaded first serves the whole process, and mixing the system
        # HIP runtime with torch's bundled HSA runtime ends in "no ROCm-capable device is detected".
        # Import torch FIRST so that both sides share torch's runtime (streams and pointers are then
        # handles of one and the same runtime instance).
        import torch  # noqa: F401

        handle = C.CDLL(str(LIB_PATH), mode=getattr(os, "RTLD_NOW", 2))
        for name, (restype, argtypes) in _SIGNATURES.items():
            fn = getattr(handle, name)  # AttributeError here == header/library mismatch
            fn.restype = restype
            fn.argtypes = argtypes
        _lib = handle
    return _lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib().nvo_last_error()
        raise RuntimeError(f"nerfvo_hip {what} failed (code {rc}): {msg.decode() if msg else '?'}")
