"""ctypes binding of the C ABI (include/dsm_hotpath.h) -- the only way the Python host side reaches
the device.  There is no CPU fallback: if the HIP library is missing or no GPU is present the
failure is loud (ImportError / DsmError)."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# DSM_HOTPATH_LIB: developer override used for A/B builds of the same sources (e.g. other compiler flags)
LIB_PATH = os.environ.get("DSM_HOTPATH_LIB") or os.path.join(_HERE, "lib", "libdsm_hotpath.so")
MAX_LEVELS = 6
ABI_VERSION = 4  # DSM_ABI_VERSION of the header the structures below mirror

c_float_p = C.POINTER(C.c_float)
c_double_p = C.POINTER(C.c_double)
c_int_p = C.POINTER(C.c_int)
c_int64_p = C.POINTER(C.c_int64)
NO_CANDIDATE = 0x7FFFFFFFFFFFFFFF


class DsmError(RuntimeError):
    pass


class Params(C.Structure):
    _fields_ = [
        ("struct_size", C.c_size_t),
        ("huber_th", C.c_float),
        ("coarse_cutoff_th", C.c_float),
        ("scale_xi_rot", C.c_float),
        ("scale_xi_trans", C.c_float),
        ("scale_a", C.c_float),
        ("scale_b", C.c_float),
        ("affine_opt_mode_a", C.c_float),
        ("affine_opt_mode_b", C.c_float),
        ("lambda_extrapolation_limit", C.c_float),
        ("max_iterations", C.c_int * MAX_LEVELS),
        ("adaptive_schedule", C.c_int),
        ("persistent_coarse", C.c_int),
        ("fuse_lm", C.c_int),
        ("work_queue", C.c_int),
        ("speculate", C.c_int),
        ("compact_tail", C.c_int),
        ("fixed_schedule", C.c_int),
        ("chunk_geometry", C.c_int),
        ("frame_check", C.c_int),
        ("frame_grad_tol", C.c_float),
    ]


class Stats(C.Structure):
    _fields_ = [
        ("evals", C.c_int64 * MAX_LEVELS),
        ("launches", C.c_int64 * MAX_LEVELS),
        ("algorithmic_bytes", C.c_int64),
        ("eval_kernel_ms", C.c_double * MAX_LEVELS),
        ("eval_kernel_union_ms", C.c_double * MAX_LEVELS),
        ("eval_dispatches", C.c_int64 * MAX_LEVELS),
        ("total_ms", C.c_double),
        ("polls", C.c_int64),
        ("coarse_launches", C.c_int64),
        ("queue_blocks", C.c_int64),
        ("queue_items", C.c_int64),
        ("queue_kernel_ms", C.c_double),
        ("evals_residual_only", C.c_int64 * MAX_LEVELS),
    ]


class StreamResult(C.Structure):
    _fields_ = [
        ("ticket", C.c_uint64),
        ("kind", C.c_int),
        ("good", C.c_int),
        ("status", C.c_int),
        ("passes", C.c_int),
        ("pose", C.c_double * 7),
        ("aff", C.c_double * 2),
        ("last_residuals", C.c_double * MAX_LEVELS),
        ("flow", C.c_double * 3),
        ("scale", C.c_float),
        ("err", C.c_float),
        ("evals", C.c_int64 * MAX_LEVELS),
    ]


class StreamHypResult(C.Structure):
    _fields_ = [
        ("ticket", C.c_uint64),
        ("have_one_good", C.c_int),
        ("tries_used", C.c_int),
        ("tries_run", C.c_int),
        ("advances", C.c_int),
        ("pose", C.c_double * 7),
        ("aff", C.c_double * 2),
        ("flow", C.c_double * 3),
        ("achieved_res", C.c_double * MAX_LEVELS),
        ("evals", C.c_int64 * MAX_LEVELS),
    ]


class RefJob(C.Structure):
    _fields_ = [
        ("t", C.c_void_p), ("frame_owner", C.c_void_p), ("slot", C.c_int), ("ref_frame_id", C.c_int),
        ("ref_aff_a", C.c_double), ("ref_aff_b", C.c_double), ("ref_exposure", C.c_float), ("npts", C.c_int),
        ("pu", c_float_p), ("pv", c_float_p), ("pidepth", c_float_p), ("pweight", c_float_p), ("n_out", c_int_p),
    ]


class LoopJob(C.Structure):
    _fields_ = [
        ("n_kf", C.c_int), ("kf_ids", c_int_p), ("kf_pose_wc", c_double_p), ("cur_cw", c_double_p),
        ("n_pts", C.c_int), ("pt_kf_id", c_int_p), ("pt_xyz", c_double_p),
        ("kf_keep", c_int_p), ("n_out", c_int_p), ("sel_idx", c_int_p), ("pts_spherical", c_double_p),
        ("ringkey", c_float_p), ("sig_idx", c_int_p), ("sig_val", c_double_p), ("n_sig", c_int_p), ("tfm_pca_rig", c_double_p),
    ]



class IcpJob(C.Structure):
    _fields_ = [
        ("n_src", C.c_int), ("src_xyz", c_double_p), ("n_tgt", C.c_int), ("tgt_xyz", c_double_p), ("tfm_target_source", c_double_p),
        ("score", c_float_p), ("ok", c_int_p), ("iterations", c_int_p), ("state", c_int_p), ("corr_counts", c_int_p),
    ]


class PoseJob(C.Structure):
    _fields_ = [
        ("n_pts", C.c_int), ("xyz", c_double_p), ("ref_colors", C.POINTER(c_float_p)), ("ref_ab_exposure", C.c_float),
        ("new_dIp", C.POINTER(c_float_p)), ("new_I", C.POINTER(c_float_p)), ("new_ab_exposure", C.c_float), ("new_cam", C.c_float * 4),
        ("ref_to_new_io", c_double_p), ("pose_error", c_float_p), ("inlier_percent", c_int_p), ("ok", c_int_p),
    ]


class ActivationJob(C.Structure):
    _fields_ = [
        ("map", C.c_void_p), ("n_hosts", C.c_int), ("krki", c_float_p), ("kt", c_float_p),
        ("n_seeds", C.c_int), ("seed_host", c_int_p), ("seed_u", c_float_p), ("seed_v", c_float_p), ("seed_idepth", c_float_p),
        ("n_cand", C.c_int), ("cand_host", c_int_p), ("cand_u", c_float_p), ("cand_v", c_float_p), ("cand_idepth", c_float_p),
        ("cand_type", c_float_p), ("min_act_dist", C.c_float), ("decision_out", C.POINTER(C.c_ubyte)), ("n_activated_out", c_int_p),
    ]


class ImmatureJob(C.Structure):
    _fields_ = [
        ("window", C.c_void_p), ("cam", C.c_float * 4), ("cam_inv", C.c_float * 2), ("n_frames", C.c_int), ("frame_ids", c_int_p),
        ("pre_R", c_float_p), ("pre_t", c_float_p), ("pre_aff", c_float_p),
        ("n_pts", C.c_int), ("host", c_int_p), ("u", c_float_p), ("v", c_float_p), ("idepth_min", c_float_p), ("idepth_max", c_float_p),
        ("energy_th", c_float_p), ("color", c_float_p), ("weights", c_float_p), ("min_obs", C.c_int),
        ("status", C.POINTER(C.c_ubyte)), ("idepth_out", c_float_p), ("res_state", C.POINTER(C.c_ubyte)),
        ("hdd_out", c_float_p), ("bd_out", c_float_p), ("energy_out", c_float_p), ("iterations_out", c_int_p),
    ]


class TraceParams(C.Structure):
    _fields_ = [
        ("max_pix_search", C.c_float), ("slack_interval", C.c_float), ("stepsize", C.c_float), ("min_improvement", C.c_float),
        ("min_test_radius", C.c_int), ("gn_iterations", C.c_int), ("gn_threshold", C.c_float), ("extra_slack_on_th", C.c_float),
        ("huber_th", C.c_float),
    ]


class TraceJob(C.Structure):
    _fields_ = [
        ("target_tracker", C.c_void_p), ("target_slot", C.c_int), ("target_window", C.c_void_p), ("target_frame_id", C.c_int),
        ("n_hosts", C.c_int), ("krki", c_float_p), ("kt", c_float_p), ("aff", c_float_p),
        ("n_pts", C.c_int), ("host", c_int_p), ("u", c_float_p), ("v", c_float_p), ("energy_th", c_float_p), ("grad_h", c_float_p),
        ("color", c_float_p), ("weights", c_float_p),
        ("status", C.POINTER(C.c_ubyte)), ("idepth_min", c_float_p), ("idepth_max", c_float_p), ("quality", c_float_p),
        ("trace_uv", c_float_p), ("trace_interval", c_float_p), ("steps_out", c_int_p), ("counts_out", c_int_p),
    ]


class SelectParams(C.Structure):
    _fields_ = [
        ("min_grad_hist_cut", C.c_float), ("min_grad_hist_add", C.c_float), ("grad_downweight_per_level", C.c_float),
        ("select_direction_distribution", C.c_int), ("th_factor", C.c_float), ("recursions", C.c_int), ("pattern_padding", C.c_int),
        ("outlier_th", C.c_float), ("outlier_th_sum_component", C.c_float), ("overall_energy_th_weight", C.c_float),
    ]


class SelectJob(C.Structure):
    _fields_ = [
        ("tracker", C.c_void_p), ("slot", C.c_int), ("b_inv", c_float_p), ("density", C.c_float), ("potential_io", c_int_p),
        ("max_pts", C.c_int), ("u", c_float_p), ("v", c_float_p), ("energy_th", c_float_p), ("grad_h", c_float_p), ("color", c_float_p),
        ("weights", c_float_p), ("status", C.POINTER(C.c_ubyte)), ("idepth_min", c_float_p), ("idepth_max", c_float_p),
        ("quality", c_float_p), ("type", c_float_p), ("n_pts_out", c_int_p), ("num_total_out", c_int_p), ("counts_out", c_int_p),
        ("passes_out", c_int_p), ("map_out", C.POINTER(C.c_ubyte)),
    ]


class LinearizeParams(C.Structure):
    _fields_ = [
        ("huber_th", C.c_float), ("outlier_th_sum_component", C.c_float), ("scale_idepth", C.c_float), ("scale_f", C.c_float),
        ("scale_c", C.c_float), ("thn", C.c_float), ("fac_median", C.c_float), ("cw", C.c_float), ("ow", C.c_float),
        ("zero_jab_a", C.c_int), ("zero_jab_b", C.c_int),
    ]


class LinearizeJob(C.Structure):
    _fields_ = [
        ("window", C.c_void_p), ("cam", C.c_float * 4), ("cam_inv", C.c_float * 2), ("n_frames", C.c_int), ("frame_ids", c_int_p),
        ("pre_RTll_0", c_float_p), ("pre_tTll_0", c_float_p), ("pre_KRKiTll", c_float_p), ("pre_KtTll", c_float_p),
        ("pre_aff_mode", c_float_p), ("pre_b0_mode", c_float_p), ("frame_energy_th", c_float_p),
        ("n_pts", C.c_int), ("host", c_int_p), ("u", c_float_p), ("v", c_float_p), ("idepth_scaled", c_float_p),
        ("idepth_zero_scaled", c_float_p), ("color", c_float_p), ("weights", c_float_p),
        ("n_res", C.c_int), ("point", c_int_p), ("target", c_int_p), ("state_in", C.POINTER(C.c_ubyte)), ("energy_in", c_float_p),
        ("is_new", C.POINTER(C.c_ubyte)), ("fix_linearization", C.c_int),
        ("new_state", C.POINTER(C.c_ubyte)), ("new_energy", c_float_p), ("new_energy_with_outlier", c_float_p),
        ("J_out", c_float_p), ("center_projected_to", c_float_p), ("projected_to", c_float_p), ("keep", C.POINTER(C.c_ubyte)),
        ("rel_bs", c_float_p), ("energy_out", c_double_p), ("new_frame_energy_th_out", c_float_p),
    ]


class HessianJob(C.Structure):
    _fields_ = [
        ("lin", LinearizeJob), ("ad_host", c_double_p), ("ad_target", c_double_p),
        ("prior", c_float_p), ("delta", c_float_p), ("hdd_lin", c_float_p), ("bd_lin", c_float_p), ("hcd_lin", c_float_p),
        ("shift_prior_to_zero", C.c_int),
        ("H_A", c_double_p), ("b_A", c_double_p), ("H_sc", c_double_p), ("b_sc", c_double_p),
        ("acc_top", c_double_p), ("acc_D", c_double_p), ("acc_E", c_double_p), ("acc_EB", c_double_p), ("acc_Hcc", c_double_p),
        ("acc_bc", c_double_p), ("active", C.POINTER(C.c_ubyte)), ("JpJdF", c_float_p),
        ("hdd_acc", c_float_p), ("bd_acc", c_float_p), ("hcd_acc", c_float_p), ("hdi", c_float_p), ("bd_sum", c_float_p),
        ("idepth_hessian", c_float_p),
    ]


class SolveJob(C.Structure):
    _fields_ = [
        ("hes", HessianJob), ("H_L", c_double_p), ("b_L", c_double_p), ("H_M", c_double_p), ("b_M", c_double_p), ("delta_x", c_double_p),
        ("lambda_", C.c_double), ("n_null", C.c_int), ("null_basis", c_double_p), ("null_pinv", c_double_p),
        ("x", c_double_p), ("step", c_float_p), ("flags", c_int_p), ("last_HS", c_double_p), ("last_bS", c_double_p),
    ]


class StepParams(C.Structure):
    _fields_ = [
        ("scale_xi_trans", C.c_double), ("scale_xi_rot", C.c_double), ("scale_a", C.c_double), ("scale_b", C.c_double),
        ("th_opt_iterations", C.c_double),
    ]


class StepJob(C.Structure):
    _fields_ = [
        ("sol", SolveJob), ("world_to_cam_eval", c_double_p), ("state_zero", c_double_p), ("state_backup", c_double_p),
        ("frame_step", c_double_p), ("calib_zero", c_double_p), ("calib_backup", c_double_p), ("calib_step", c_double_p),
        ("idepth_backup", c_float_p), ("idepth_step", c_float_p), ("exposure", c_float_p), ("stepfac", C.c_float * 5),
        ("prior", c_double_p), ("prior_zero", c_double_p),
        ("state_out", c_double_p), ("calib_out", c_double_p), ("idepth_out", c_float_p), ("world_to_cam_out", c_double_p),
        ("cam_to_world_out", c_double_p), ("can_break", c_int_p), ("step_sums", c_float_p), ("energy_m", c_double_p),
        ("cam_out", c_float_p), ("pre_RTll_0_out", c_float_p), ("pre_tTll_0_out", c_float_p), ("pre_KRKiTll_out", c_float_p),
        ("pre_KtTll_out", c_float_p), ("pre_aff_mode_out", c_float_p), ("pre_b0_mode_out", c_float_p),
        ("delta_x_out", c_double_p), ("H_L_out", c_double_p), ("b_L_out", c_double_p),
    ]


class OptimizeParams(C.Structure):
    _fields_ = [
        ("lambda_init", C.c_double), ("lambda_accept_fac", C.c_double), ("lambda_reject_fac", C.c_double), ("fixed_lambda", C.c_double),
        ("min_iterations", C.c_int), ("force_accept", C.c_int), ("step_momentum", C.c_int),
    ]


class OptimizeJob(C.Structure):
    _fields_ = [
        ("step", StepJob), ("max_iterations", C.c_int), ("n_iterations", c_int_p), ("n_passes", c_int_p), ("pattern", C.POINTER(C.c_ubyte)),
        ("pass_energy", c_double_p), ("pass_lambda", c_double_p), ("iter_stepsize", c_float_p), ("iter_can_break", C.POINTER(C.c_ubyte)),
        ("last_energy", c_double_p), ("lambda_out", c_double_p), ("frame_energy_th_out", c_float_p),
    ]


class FinishJob(C.Structure):
    _fields_ = [
        ("opt", OptimizeJob), ("n_good_residuals_in", c_int_p), ("max_rel_baseline_in", c_float_p), ("last_res", c_int_p),
        ("last_state_in", C.POINTER(C.c_ubyte)),
        ("world_to_cam_eval_out", c_double_p), ("state_zero_out", c_double_p), ("state_out", c_double_p),
        ("ad_host_out", c_double_p), ("ad_target_out", c_double_p), ("ad_ht_delta_out", c_float_p), ("c_delta_out", c_float_p),
        ("delta_x_out", c_double_p), ("pre_RTll_0_out", c_float_p), ("pre_tTll_0_out", c_float_p), ("pre_KRKiTll_out", c_float_p),
        ("pre_KtTll_out", c_float_p), ("pre_aff_mode_out", c_float_p), ("pre_b0_mode_out", c_float_p), ("cam_out", c_float_p),
        ("new_state", C.POINTER(C.c_ubyte)), ("new_energy", c_float_p), ("new_energy_with_outlier", c_float_p),
        ("keep", C.POINTER(C.c_ubyte)), ("rel_bs", c_float_p), ("energy", c_double_p), ("frame_energy_th_out", c_float_p),
        ("n_good_residuals_out", c_int_p), ("max_rel_baseline_out", c_float_p), ("last_res_out", c_int_p),
        ("last_state_out", C.POINTER(C.c_ubyte)), ("n_res_kept", c_int_p), ("point_dropped", C.POINTER(C.c_ubyte)),
        ("res_index_out", c_int_p), ("point_index_out", c_int_p), ("n_res_out", c_int_p), ("n_pts_out", c_int_p),
        ("rmse", c_float_p), ("lost", c_int_p), ("cam_to_world_out", c_double_p), ("J_out", c_float_p),
    ]


class MarginalizeParams(C.Structure):
    _fields_ = [
        ("min_good_active_res_for_marg", C.c_int), ("min_good_res_for_marg", C.c_int), ("min_idepth_h_marg", C.c_float),
        ("marg_weight_fac", C.c_float), ("idepth_fix_prior_marg_fac", C.c_float),
    ]


class MarginalizeJob(C.Structure):
    _fields_ = [
        ("hes", HessianJob), ("flagged", C.POINTER(C.c_ubyte)), ("n_good_residuals", c_int_p), ("last_state", C.POINTER(C.c_ubyte)),
        ("idepth_hessian", c_float_p), ("ad_ht_delta", c_float_p), ("c_delta", c_float_p), ("H_M", c_double_p), ("b_M", c_double_p),
        ("n_marg_frames", C.c_int), ("marg_frames", c_int_p), ("frame_prior", c_double_p), ("frame_delta_prior", c_double_p),
        ("verdict", C.POINTER(C.c_ubyte)), ("H_M_out", c_double_p), ("b_M_out", c_double_p), ("n_res_marg", c_int_p),
        ("H_M_points", c_double_p), ("b_M_points", c_double_p), ("res_to_zero", c_float_p),
    ]


class NullspaceParams(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int), ("scale_xi_trans", C.c_double), ("scale_xi_rot", C.c_double), ("scale_a", C.c_double),
        ("scale_b", C.c_double), ("solver_mode_delta", C.c_double),
    ]


class NullspaceJob(C.Structure):
    _fields_ = [
        ("n_frames", C.c_int), ("world_to_cam_eval", c_double_p), ("state_zero", c_double_p), ("exposure", c_float_p),
        ("frame_null_in", c_double_p), ("null_basis", c_double_p), ("null_pinv", c_double_p), ("sing", c_double_p),
        ("rank", c_int_p), ("flags", c_int_p), ("frame_null_out", c_double_p), ("null_x0_pre", c_double_p),
    ]


class RescaleJob(C.Structure):
    _fields_ = (
        [("n_frames", C.c_int), ("n_pts", C.c_int), ("enabled", C.c_int), ("scale_error", C.c_float), ("new_scale", C.c_float),
         ("thres", C.c_float), ("trapped", C.c_int), ("fails", C.c_int)]
        + [(k, c_float_p) for k in ("idepth", "idepth_scaled", "idepth_zero_scaled", "delta")]
        + [("world_to_cam_eval", c_double_p), ("state", c_double_p), ("state_zero", c_double_p), ("exposure", c_float_p),
           ("cam_to_tracking_ref", c_double_p), ("ref_cam_to_world", c_double_p), ("cam_to_world", c_double_p), ("aff_g2l", C.c_double * 2),
           ("calib_value", c_double_p), ("calib_zero", c_double_p), ("ad_host", c_double_p), ("ad_target", c_double_p)]
        + [(k, c_float_p) for k in ("pre_RTll_0", "pre_tTll_0", "pre_KRKiTll", "pre_KtTll", "pre_aff_mode", "pre_b0_mode", "cam", "c_delta")]
        + [("delta_x", c_double_p), ("ad_ht_delta", c_float_p), ("world_to_cam", c_double_p), ("cam_to_world_all", c_double_p)]
        + [(k, c_float_p) for k in ("idepth_out", "idepth_scaled_out", "idepth_zero_scaled_out", "delta_out")]
        + [(k, c_double_p) for k in ("world_to_cam_eval_out", "state_out", "state_zero_out", "cam_to_tracking_ref_out", "cam_to_world_out")]
        + [(k, c_float_p) for k in ("pre_RTll_0_out", "pre_tTll_0_out", "pre_KRKiTll_out", "pre_KtTll_out", "pre_aff_mode_out",
                                    "pre_b0_mode_out", "cam_out", "c_delta_out")]
        + [("delta_x_out", c_double_p), ("ad_ht_delta_out", c_float_p), ("world_to_cam_out", c_double_p), ("cam_to_world_out_all", c_double_p),
           ("decision", c_int_p), ("scale_error_out", c_float_p), ("trapped_out", c_int_p), ("fails_out", c_int_p), ("applied_scale", c_float_p)]
    )


class AdmitParams(C.Structure):
    _fields_ = [("min_frames", C.c_int), ("max_frames", C.c_int), ("min_frame_age", C.c_int), ("min_points_remaining", C.c_float),
                ("max_log_aff_fac_in_window", C.c_float)]


c_ubyte_p = C.POINTER(C.c_ubyte)


class AdmitJob(C.Structure):
    _fields_ = (
        [("n_frames", C.c_int), ("n_pts", C.c_int), ("n_res", C.c_int), ("new_keyframe_id", C.c_int), ("new_exposure", C.c_float),
         ("new_frame_energy_th", C.c_float), ("aff_g2l", C.c_double * 2),
         ("world_to_cam_eval", c_double_p), ("state", c_double_p), ("state_zero", c_double_p), ("exposure", c_float_p), ("frame_energy_th", c_float_p),
         ("keyframe_id", c_int_p), ("n_points_in", c_int_p), ("n_points_out", c_int_p)]
        + [(k, c_double_p) for k in ("ref_cam_to_world", "cam_to_tracking_ref", "new_frame_prior", "new_frame_prior_zero", "calib_value", "calib_zero",
                                     "H_M", "b_M", "H_L", "b_L", "prior", "prior_zero")]
        + [("host", c_int_p), ("last_res", c_int_p), ("last_state", c_ubyte_p), ("point", c_int_p), ("target", c_int_p), ("state_in", c_ubyte_p),
           ("energy_in", c_float_p), ("is_new", c_ubyte_p),
           ("world_to_cam_eval_out", c_double_p), ("state_out", c_double_p), ("state_zero_out", c_double_p), ("exposure_out", c_float_p),
           ("frame_energy_th_out", c_float_p), ("keyframe_id_out", c_int_p), ("world_to_cam_out", c_double_p), ("flagged_out", c_ubyte_p),
           ("cam_to_world_out", c_double_p)]
        + [(k, c_float_p) for k in ("pre_RTll_0_out", "pre_tTll_0_out", "pre_KRKiTll_out", "pre_KtTll_out", "pre_aff_mode_out", "pre_b0_mode_out",
                                    "distance_ll_out", "cam_out", "c_delta_out")]
        + [("delta_x_out", c_double_p), ("ad_host_out", c_double_p), ("ad_target_out", c_double_p), ("ad_ht_delta_out", c_float_p)]
        + [(k, c_double_p) for k in ("H_M_out", "b_M_out", "H_L_out", "b_L_out", "prior_out", "prior_zero_out", "frame_prior_out", "frame_delta_prior_out")]
        + [("point_out", c_int_p), ("target_out", c_int_p), ("res_state_out", c_ubyte_p), ("energy_out", c_float_p), ("is_new_out", c_ubyte_p),
           ("res_index_out", c_int_p), ("new_res_index_out", c_int_p), ("last_res_out", c_int_p), ("last_state_out", c_ubyte_p),
           ("n_res_out", c_int_p), ("n_flagged", c_int_p), ("dist_score_out", c_double_p)]
    )


class LmProposeIn(C.Structure):
    _fields_ = [
        ("H", C.c_double * 64), ("b", C.c_double * 8), ("cur", C.c_double * 7), ("aff_cur", C.c_double * 2),
        ("lam", C.c_float), ("level_cutoff_repeat", C.c_float), ("iteration", C.c_int),
        ("Hs", C.c_float), ("bs", C.c_float), ("scale_cur", C.c_float),
    ]


class LmProposeOut(C.Structure):
    _fields_ = [
        ("inc", C.c_double * 8), ("inc_norm", C.c_double), ("cand", C.c_double * 7), ("aff_cand", C.c_double * 2),
        ("M", C.c_float * 9), ("t", C.c_float * 3), ("aff0", C.c_float), ("aff1", C.c_float), ("cutoff", C.c_float),
        ("max_energy", C.c_float), ("residual_only", C.c_int), ("Ki", C.c_float * 9),
        ("inc_f", C.c_float), ("scale_cand", C.c_float), ("pad", C.c_int * 2),
    ]


class LmStepEval(C.Structure):
    _fields_ = [
        ("M", C.c_float * 9), ("t", C.c_float * 3), ("aff0", C.c_float), ("aff1", C.c_float), ("cutoff", C.c_float),
        ("max_energy", C.c_float), ("residual_only", C.c_int), ("scale", C.c_float), ("Ki", C.c_float * 9), ("n", C.c_int),
    ]


class LmStepState(C.Structure):
    _fields_ = [
        ("H", C.c_double * 64), ("b", C.c_double * 8), ("cur", C.c_double * 7), ("aff_cur", C.c_double * 2),
        ("cand", C.c_double * 7), ("aff_cand", C.c_double * 2), ("spec_cand", C.c_double * 7), ("spec_aff_cand", C.c_double * 2),
        ("inc_norm", C.c_double), ("spec_inc_norm", C.c_double), ("res_old", C.c_double * 6),
        ("min_res", C.c_double * MAX_LEVELS), ("last_residuals", C.c_double * MAX_LEVELS), ("last_inners", C.c_double * MAX_LEVELS),
        ("flow", C.c_double * 3),
        ("evals", C.c_longlong * MAX_LEVELS), ("evals_ro", C.c_longlong * MAX_LEVELS), ("rounds", C.c_longlong * MAX_LEVELS),
        ("status", C.c_int), ("lvl", C.c_int), ("phase", C.c_int), ("iteration", C.c_int), ("have_repeated", C.c_int),
        ("coarsest", C.c_int), ("spec_valid", C.c_int), ("ticks", C.c_int),
        ("lam", C.c_float), ("level_cutoff_repeat", C.c_float),
        ("inc_f", C.c_float), ("spec_inc_f", C.c_float), ("scale_cur", C.c_float), ("scale_cand", C.c_float),
        ("spec_scale_cand", C.c_float), ("Hs", C.c_float), ("bs", C.c_float),
        ("nch", C.c_int),
        ("ev", LmStepEval), ("spec_ev", LmStepEval),
    ]


# dsm_diag_tick_*: the tick engine's lists and rings (DSM_TICK_* of include/dsm_hotpath.h)
TICK_SENTINEL, TICK_NOOP, TICK_CAND, TICK_CHUNK_BITS, TICK_MAX_SEGS = 0x3FFFF5A5, 0x80000000, 0x40000000, 12, 20


class TickSeg(C.Structure):
    _fields_ = [("mode", C.c_int), ("i0", C.c_int), ("ns", C.c_int)]


class TickListCfg(C.Structure):
    _fields_ = [("cap", C.c_int), ("chain_cap", C.c_int), ("chain_max_n0", C.c_int), ("buf", C.c_int), ("count", C.c_int), ("chain", C.c_int)]


class TickSegCtl(C.Structure):
    _fields_ = [("count", C.c_int * 2), ("overflow", C.c_int), ("chain", C.c_int * 2), ("pad", C.c_int * 27)]


class TickModeCtl(C.Structure):
    _fields_ = [("pending_head", C.c_longlong), ("pending_count", C.c_longlong), ("retired", C.c_longlong), ("ring", C.c_int), ("pad", C.c_int),
                ("sched_evals", C.c_longlong * MAX_LEVELS), ("sched_ro", C.c_longlong * MAX_LEVELS), ("sched_items", C.c_longlong * MAX_LEVELS)]


class TickPending(C.Structure):
    _fields_ = [("pose", C.c_double * 7), ("aff", C.c_double * 2), ("min_res", C.c_double * MAX_LEVELS), ("scale", C.c_float),
                ("coarsest", C.c_int), ("ticket", C.c_uint64)]


_TICK_RESULT_TAIL = [("cur", C.c_double * 7), ("aff_cur", C.c_double * 2), ("last_residuals", C.c_double * MAX_LEVELS), ("flow", C.c_double * 3),
                     ("scale_cur", C.c_float), ("pad1", C.c_float),
                     ("evals", C.c_longlong * MAX_LEVELS), ("evals_ro", C.c_longlong * MAX_LEVELS), ("rounds", C.c_longlong * MAX_LEVELS)]


class TickResult(C.Structure):
    _fields_ = [("ticket", C.c_uint64), ("status", C.c_int), ("ticks", C.c_int)] + _TICK_RESULT_TAIL


class TickSlot(C.Structure):
    _fields_ = [("status", C.c_int), ("lvl", C.c_int), ("n", C.c_int), ("ppt", C.c_int), ("spec_valid", C.c_int), ("n0", C.c_int),
                ("residual_only", C.c_int), ("ticks", C.c_int), ("stepped", C.c_int), ("reserve", C.c_int), ("res_base", C.c_int),
                ("res_total", C.c_int), ("ticket", C.c_uint64)] + _TICK_RESULT_TAIL


class TickSlotOut(C.Structure):
    _fields_ = [("status", C.c_int), ("lvl", C.c_int), ("stepped", C.c_int), ("n", C.c_int), ("ppt", C.c_int), ("spec_valid", C.c_int),
                ("n0", C.c_int), ("residual_only", C.c_int), ("tracker_set", C.c_int), ("pad", C.c_int), ("ticket", C.c_uint64)]


# every symbol include/dsm_hotpath.h declares: name -> (restype, argtypes)
_vp = C.c_void_p
_pp_f = C.POINTER(c_float_p)
_pp_i = C.POINTER(c_int_p)
_pp_d = C.POINTER(c_double_p)
# transports of dsm_ringdb_merge_topk_with: (user, d_buf, count, hip_stream) / (user, d_send, d_recv, count, hip_stream)
ALLREDUCE_MIN_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)
ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)
MERGE_ALGOS = {"allreduce_min": 0, "allgather": 1}
# DSM_RINGKEY_FORM_* of include/dsm_hotpath.h, in the enum's order (dsm_ringdb_scan_plan)
RINGKEY_FORMS = ("FEWQ4_1", "FEWQ4_2", "FEWQ_4", "FEWQ_8", "TILE_1", "TILE_2", "TILE_ANYDIM", "MANY4", "MANY_ANYDIM")
SYMBOLS = {
    "dsm_last_error": (C.c_char_p, []),
    "dsm_abi_version": (C.c_int, []),
    "dsm_tracker_upload_intensity": (C.c_int, [_vp, C.c_int, _pp_f, C.c_float]),
    "dsm_params_default": (None, [C.POINTER(Params)]),
    "dsm_params_default_sized": (C.c_int, [C.POINTER(Params), C.c_size_t]),
    "dsm_stream_create": (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(_vp)]),
    "dsm_stream_destroy": (C.c_int, [_vp]),
    "dsm_stream_submit_track": (C.c_int, [_vp, C.c_int, C.POINTER(_vp), c_double_p, c_double_p, C.c_int, c_double_p, C.POINTER(C.c_uint64)]),
    "dsm_stream_submit_scale": (C.c_int, [_vp, C.c_int, C.POINTER(_vp), c_float_p, C.c_int, C.POINTER(C.c_uint64)]),
    "dsm_stream_advance": (C.c_int, [_vp]),
    "dsm_stream_drain": (C.c_int, [_vp]),
    "dsm_stream_sync": (C.c_int, [_vp]),
    "dsm_stream_set_pipelined": (C.c_int, [_vp, C.c_int]),
    "dsm_stream_results": (C.c_int, [_vp, C.c_int, C.POINTER(StreamResult), c_int_p]),
    "dsm_stream_counts": (C.c_int, [_vp, c_int_p, c_int_p, c_int_p]),
    "dsm_stream_set_quantile": (C.c_int, [_vp, C.c_int, C.c_double]),
    "dsm_stream_set_engine": (C.c_int, [_vp, C.c_int, C.c_int]),
    "dsm_stream_set_chain": (C.c_int, [_vp, C.c_int]),
    "dsm_stream_set_rounds": (C.c_int, [_vp, C.c_int, c_int_p]),
    "dsm_stream_get_stats": (C.c_int, [_vp, C.POINTER(Stats), C.POINTER(Stats)]),
    "dsm_stream_get_schedule": (C.c_int, [_vp, C.c_int, c_int_p, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    "dsm_stream_submit_hypotheses": (C.c_int, [_vp, _vp, C.c_int, c_double_p, c_double_p, C.c_int, C.c_double, C.c_double, C.POINTER(C.c_uint64)]),
    "dsm_stream_hypotheses_results": (C.c_int, [_vp, C.c_int, C.POINTER(StreamHypResult), c_int_p]),
    "dsm_stream_hypotheses_counts": (C.c_int, [_vp, c_int_p, c_int_p]),
    "dsm_stream_set_hypothesis_window": (C.c_int, [_vp, C.c_int]),
    "dsm_hypotheses_resolve": (C.c_int, [C.c_int, c_double_p, c_double_p, C.c_int, C.c_double, C.c_double, C.c_int, c_int_p, c_double_p, c_double_p,
                                         c_double_p, c_double_p, C.POINTER(StreamHypResult), c_int_p]),
    "dsm_context_create": (C.c_int, [C.c_int, C.POINTER(_vp)]),
    "dsm_context_destroy": (C.c_int, [_vp]),
    "dsm_context_sync": (C.c_int, [_vp]),
    "dsm_context_set_timing": (C.c_int, [_vp, C.c_int]),
    "dsm_context_set_streams": (C.c_int, [_vp, C.c_int]),
    "dsm_context_get_stats": (C.c_int, [_vp, C.POINTER(Stats)]),
    "dsm_context_stream": (_vp, [_vp]),
    "dsm_context_stream_queues": (C.c_int, [_vp, c_int_p, c_int_p]),
    "dsm_diag_read_bandwidth": (C.c_int, [_vp, C.c_size_t, C.c_int, c_double_p]),
    "dsm_diag_read_bandwidth_chunked": (C.c_int, [_vp, C.c_size_t, C.c_size_t, C.c_int, c_double_p]),
    "dsm_diag_xwg_litmus": (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    "dsm_tracker_create": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, c_double_p, c_float_p, C.POINTER(Params), C.POINTER(_vp)]),
    "dsm_tracker_destroy": (C.c_int, [_vp]),
    "dsm_tracker_make_k": (C.c_int, [_vp, C.c_float, C.c_float, C.c_float, C.c_float]),
    "dsm_tracker_set_ref": (C.c_int, [_vp, C.c_int, C.c_double, C.c_double, C.c_float, c_int_p, _pp_f, _pp_f, _pp_f, _pp_f]),
    "dsm_set_refs_from_points": (C.c_int, [_vp, C.c_int, C.POINTER(RefJob)]),
    "dsm_tracker_set_ref_from_points": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_float, C.c_int, c_float_p, c_float_p, c_float_p, c_float_p, c_int_p]),
    "dsm_tracker_scale_depth": (C.c_int, [_vp, C.c_float]),
    "dsm_tracker_get_template": (C.c_int, [_vp, C.c_int, c_int_p, c_float_p, c_float_p, c_float_p, c_float_p]),
    "dsm_tracker_upload_frame": (C.c_int, [_vp, C.c_int, _pp_f, C.c_float]),
    "dsm_tracker_upload_image": (C.c_int, [_vp, C.c_int, c_float_p, C.c_float]),
    "dsm_upload_images": (C.c_int, [_vp, C.c_int, C.POINTER(_vp), c_int_p, C.POINTER(_vp), c_float_p, C.c_int, C.c_size_t]),
    "dsm_upload_images_async": (C.c_int, [_vp, C.c_int, C.POINTER(_vp), c_int_p, C.POINTER(_vp), c_float_p, C.c_int, C.c_size_t]),
    "dsm_upload_images_enqueue": (C.c_int, [_vp, C.c_int, C.POINTER(_vp), c_int_p, C.POINTER(_vp), c_float_p, C.c_int, C.c_size_t]),
    "dsm_upload_wait": (C.c_int, [_vp]),
    "dsm_frames_advance": (C.c_int, [_vp, C.c_int, C.POINTER(_vp), c_int_p]),
    "dsm_pinhole_undistort_map": (C.c_int, [c_double_p, C.c_int, C.c_int, C.c_int, c_float_p, C.c_int, C.c_int, c_float_p, c_int_p, c_float_p, c_float_p]),
    "dsm_undistorter_create": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, c_float_p, c_float_p, c_float_p, c_float_p, C.POINTER(_vp)]),
    "dsm_undistorter_destroy": (C.c_int, [_vp]),
    "dsm_upload_images_undistorted": (C.c_int, [_vp, _vp, C.c_int, C.POINTER(_vp), c_int_p, C.POINTER(_vp), c_float_p, C.c_size_t, C.c_int]),
    "dsm_host_alloc": (C.c_int, [C.c_size_t, C.POINTER(_vp)]),
    "dsm_host_free": (C.c_int, [_vp]),
    "dsm_tracker_get_frame": (C.c_int, [_vp, C.c_int, C.c_int, c_float_p]),
    "dsm_tracker_calc_res_pose": (C.c_int, [_vp, C.c_int, c_double_p, c_double_p, C.c_float, c_double_p, c_double_p, c_double_p, c_int_p]),
    "dsm_tracker_calc_res_scale": (C.c_int, [_vp, C.c_int, C.c_float, C.c_float, c_double_p, c_float_p, c_float_p, c_int_p]),
    "dsm_diag_single_eval": (C.c_int, [_vp, C.c_int, C.c_int, c_double_p, c_double_p, C.c_float, C.c_float, C.c_int, C.c_int, c_double_p, c_double_p,
                                       c_double_p, c_float_p, c_float_p, c_int_p]),
    "dsm_diag_eval_facts": (C.c_int, [_vp, C.c_int, c_double_p, c_int_p, c_float_p]),
    "dsm_diag_tracker_force_general": (C.c_int, [_vp, C.c_int]),
    "dsm_pose_fact_host": (C.c_int, [C.c_int, c_float_p, c_int_p]),
    "dsm_fact_rules_host": (C.c_int, [C.c_int, c_float_p, c_int_p]),
    "dsm_diag_pose_estimator_eval": (C.c_int, [_vp, C.c_int, c_double_p, _pp_f, C.c_float, _pp_f, C.c_float, c_float_p, C.c_int, c_double_p, c_double_p,
                                               C.c_float, C.c_int, C.c_int, c_double_p, c_double_p, c_double_p, c_int_p]),
    "dsm_diag_lm_propose": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.POINTER(LmProposeIn), C.c_int, C.c_int, C.POINTER(LmProposeOut)]),
    "dsm_diag_lm_step": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.POINTER(LmStepState), c_float_p, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int,
                                   C.POINTER(LmStepState)]),
    "dsm_diag_tick_reserve": (C.c_int, [_vp, C.c_int, C.POINTER(TickSeg), C.c_int, C.POINTER(C.c_ubyte), C.POINTER(C.c_longlong),
                                        C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), c_int_p]),
    "dsm_diag_tick_stage": (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(TickSlot), C.POINTER(TickListCfg), C.POINTER(TickModeCtl), C.c_int,
                                      C.POINTER(TickPending), C.c_int, C.POINTER(C.c_uint), c_int_p, C.POINTER(TickSegCtl), C.POINTER(TickModeCtl),
                                      C.POINTER(TickResult), C.POINTER(TickSlotOut), C.POINTER(LmStepState), C.POINTER(C.c_ubyte), c_int_p,
                                      C.POINTER(C.c_ubyte)]),
    "dsm_diag_tick_step": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.POINTER(LmStepState), C.POINTER(TickSlot), c_float_p, C.c_longlong, C.c_int,
                                     C.c_int, C.POINTER(TickListCfg), C.POINTER(TickModeCtl), C.c_int, C.POINTER(TickPending),
                                     C.POINTER(C.c_longlong), C.POINTER(C.c_uint), c_int_p, C.POINTER(TickSegCtl), C.POINTER(TickModeCtl),
                                     C.POINTER(TickResult), C.POINTER(TickSlotOut), C.POINTER(LmStepState), C.POINTER(C.c_ubyte), c_int_p,
                                     C.POINTER(C.c_ubyte)]),
    "dsm_diag_icp_stages":(C.c_int, [_vp, C.c_int, C.POINTER(IcpJob), C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, c_float_p, c_float_p,
                                      c_float_p, C.POINTER(C.c_uint64), _vp]),
    "dsm_tracker_track": (C.c_int, [_vp, c_double_p, c_double_p, C.c_int, c_double_p, c_double_p, c_double_p, c_int_p]),
    "dsm_tracker_optimize_scale": (C.c_int, [_vp, c_float_p, C.c_int, c_float_p]),
    "dsm_tracker_optimize_scale_guesses": (C.c_int, [_vp, C.c_int, c_float_p, C.c_int, c_float_p, c_float_p, c_float_p, c_float_p]),
    "dsm_track_and_scale_batch": (C.c_int, [_vp, C.c_int, C.POINTER(_vp), c_double_p, c_double_p, C.c_int, c_double_p, c_double_p, c_double_p, c_int_p,
                                           C.c_int, C.POINTER(_vp), c_float_p, c_float_p]),
    "dsm_context_get_stats2": (C.c_int, [_vp, C.POINTER(Stats)]),
    "dsm_track_batch": (C.c_int, [_vp, C.c_int, C.POINTER(_vp), c_double_p, c_double_p, C.c_int, c_double_p, c_double_p, c_double_p, c_int_p]),
    "dsm_optimize_scale_batch": (C.c_int, [_vp, C.c_int, C.POINTER(_vp), c_float_p, C.c_int, c_float_p]),
    "dsm_tracker_ref_frame_id": (C.c_int, [_vp]),
    "dsm_reduction_geometry": (C.c_int, [_vp, C.c_int, C.c_int, c_int_p, c_int_p, c_int_p]),
    "dsm_pose_estimator_create": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.POINTER(Params), C.POINTER(_vp)]),
    "dsm_pose_estimator_destroy": (C.c_int, [_vp]),
    "dsm_pose_estimator_estimate": (C.c_int, [_vp, C.c_int, c_double_p, _pp_f, C.c_float, _pp_f, C.c_float, c_float_p, C.c_int, c_double_p, c_float_p, c_int_p]),
    "dsm_pose_batch_create": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.POINTER(Params), C.POINTER(_vp)]),
    "dsm_pose_batch_destroy": (C.c_int, [_vp]),
    "dsm_pose_estimate_batch": (C.c_int, [_vp, C.c_int, C.POINTER(PoseJob), C.c_int]),
    "dsm_ringdb_create": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_float, c_float_p, C.c_int64, C.c_int, C.c_int, C.POINTER(_vp)]),
    "dsm_ringdb_destroy": (C.c_int, [_vp]),
    "dsm_ringdb_size": (C.c_int64, [_vp]),
    "dsm_ringdb_query_then_enqueue": (C.c_int, [_vp, c_float_p, c_int_p, c_int_p]),
    "dsm_ringdb_query_then_enqueue_many": (C.c_int, [C.c_int, C.POINTER(_vp), c_float_p, c_int_p, c_int_p]),
    "dsm_ringdb_add_points": (C.c_int, [_vp, c_float_p, C.c_int64]),
    "dsm_ringdb_enqueue": (C.c_int, [_vp, c_float_p]),
    "dsm_ringdb_knn_packed": (C.c_int, [_vp, c_float_p, C.c_int, _vp]),
    "dsm_ringdb_knn_packed_dev": (C.c_int, [_vp, _vp, C.c_int, _vp]),
    "dsm_ringdb_knn_packed_host": (C.c_int, [_vp, c_float_p, C.c_int, c_int64_p]),
    "dsm_ringdb_scan_plan": (C.c_int, [_vp, C.c_int, C.c_int, c_int_p, c_int_p, C.POINTER(C.c_longlong)]),
    "dsm_comm_unique_id": (C.c_int, [C.POINTER(C.c_ubyte)]),
    "dsm_comm_create": (C.c_int, [_vp, C.POINTER(C.c_ubyte), C.c_int, C.c_int, C.POINTER(_vp)]),
    "dsm_comm_destroy": (C.c_int, [_vp]),
    "dsm_comm_rank": (C.c_int, [_vp]),
    "dsm_comm_size": (C.c_int, [_vp]),
    "dsm_ringdb_merge_topk": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int]),
    "dsm_ringdb_merge_topk_with": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, ALLREDUCE_MIN_FN, ALLGATHER_FN, _vp]),
    "dsm_ringdb_attach_comm": (C.c_int, [_vp, _vp]),
    "dsm_ringdb_attach_transport": (C.c_int, [_vp, C.c_int, ALLREDUCE_MIN_FN, ALLGATHER_FN, _vp]),
    "dsm_scancontext_generate": (C.c_int, [c_double_p, C.c_int, C.c_double, C.c_int, C.c_int, c_float_p, c_int_p, c_double_p, c_int_p, c_double_p]),
    "dsm_generate_spherical_points": (C.c_int, [C.c_int, c_int_p, c_double_p, c_double_p, C.c_double, C.c_int, c_int_p, c_double_p, c_int_p, c_int_p, c_int_p, c_double_p]),
    "dsm_loop_descriptors_batch": (C.c_int, [_vp, C.c_int, C.POINTER(LoopJob), C.c_double, C.c_int, C.c_int]),
    "dsm_loop_detect_batch": (C.c_int, [_vp, _vp, C.c_int, C.POINTER(LoopJob), C.c_double, C.c_int, C.c_int, c_int_p, c_int_p]),
    "dsm_loop_detect_batch_many": (C.c_int, [_vp, C.c_int, C.POINTER(LoopJob), C.POINTER(_vp), C.c_double, C.c_int, C.c_int, c_int_p, c_int_p]),
    "dsm_icp_batch": (C.c_int, [_vp, C.c_int, C.POINTER(IcpJob), C.c_int, C.c_double, C.c_double, C.c_double]),
    "dsm_distmap_create": (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(_vp)]),
    "dsm_distmap_destroy": (C.c_int, [_vp]),
    "dsm_distmap_get": (C.c_int, [_vp, c_float_p]),
    "dsm_distmap_add": (C.c_int, [_vp, C.c_int, C.c_int]),
    "dsm_distmaps_make": (C.c_int, [_vp, C.c_int, C.POINTER(ActivationJob)]),
    "dsm_activate_points_batch": (C.c_int, [_vp, C.c_int, C.POINTER(ActivationJob)]),
    "dsm_activate_points_host": (C.c_int, [C.c_int, C.c_int, C.POINTER(ActivationJob), c_float_p]),
    "dsm_window_create": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.POINTER(_vp)]),
    "dsm_window_destroy": (C.c_int, [_vp]),
    "dsm_window_put_host": (C.c_int, [_vp, C.c_int, c_float_p]),
    "dsm_window_put_from_tracker": (C.c_int, [_vp, C.c_int, _vp, C.c_int]),
    "dsm_window_drop": (C.c_int, [_vp, C.c_int]),
    "dsm_window_get": (C.c_int, [_vp, C.c_int, c_float_p]),
    "dsm_optimize_immature_points_batch": (C.c_int, [_vp, C.c_int, C.POINTER(ImmatureJob), C.c_float, C.c_float, C.c_int]),
    "dsm_optimize_immature_points_host": (C.c_int, [C.c_int, C.c_int, C.POINTER(ImmatureJob), C.POINTER(c_float_p), C.c_float, C.c_float, C.c_int]),
    "dsm_trace_params_default": (C.c_int, [C.POINTER(TraceParams)]),
    "dsm_trace_points_batch": (C.c_int, [_vp, C.c_int, C.POINTER(TraceJob), C.POINTER(TraceParams)]),
    "dsm_trace_points_host": (C.c_int, [C.c_int, C.c_int, c_float_p, C.POINTER(TraceJob), C.POINTER(TraceParams)]),
    "dsm_select_params_default": (C.c_int, [C.POINTER(SelectParams)]),
    "dsm_pixel_selector_create": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_ubyte), C.POINTER(_vp)]),
    "dsm_pixel_selector_destroy": (C.c_int, [_vp]),
    "dsm_select_pixels_batch": (C.c_int, [_vp, C.c_int, C.POINTER(SelectJob), C.POINTER(SelectParams)]),
    "dsm_select_pixels_host": (C.c_int, [C.c_int, C.c_int, c_float_p, c_float_p, c_float_p, C.POINTER(C.c_ubyte), C.POINTER(SelectJob),
                                         C.POINTER(SelectParams)]),
    "dsm_linearize_params_default": (C.c_int, [C.POINTER(LinearizeParams)]),
    "dsm_linearize_residuals_batch": (C.c_int, [_vp, C.c_int, C.POINTER(LinearizeJob), C.POINTER(LinearizeParams)]),
    "dsm_linearize_residuals_host": (C.c_int, [C.c_int, C.c_int, C.POINTER(LinearizeJob), C.POINTER(c_float_p), C.POINTER(LinearizeParams)]),
    "dsm_window_hessian_batch": (C.c_int, [_vp, C.c_int, C.POINTER(HessianJob), C.POINTER(LinearizeParams)]),
    "dsm_window_hessian_host": (C.c_int, [C.c_int, C.c_int, C.POINTER(HessianJob), C.POINTER(c_float_p), C.POINTER(LinearizeParams)]),
    "dsm_window_solve_batch": (C.c_int, [_vp, C.c_int, C.POINTER(SolveJob), C.POINTER(LinearizeParams)]),
    "dsm_window_solve_host": (C.c_int, [C.c_int, C.c_int, C.POINTER(SolveJob), C.POINTER(c_float_p), C.POINTER(LinearizeParams)]),
    "dsm_step_params_default": (C.c_int, [C.POINTER(StepParams)]),
    "dsm_window_step_batch": (C.c_int, [_vp, C.c_int, C.POINTER(StepJob), C.POINTER(LinearizeParams), C.POINTER(StepParams)]),
    "dsm_window_step_host": (C.c_int, [C.c_int, C.c_int, C.POINTER(StepJob), C.POINTER(c_float_p), C.POINTER(LinearizeParams), C.POINTER(StepParams)]),
    "dsm_optimize_params_default": (C.c_int, [C.POINTER(OptimizeParams)]),
    "dsm_window_optimize_batch": (C.c_int, [_vp, C.c_int, C.POINTER(OptimizeJob), C.POINTER(LinearizeParams), C.POINTER(StepParams),
                                            C.POINTER(OptimizeParams)]),
    "dsm_window_optimize_host": (C.c_int, [C.c_int, C.c_int, C.POINTER(OptimizeJob), C.POINTER(c_float_p), C.POINTER(LinearizeParams),
                                           C.POINTER(StepParams), C.POINTER(OptimizeParams)]),
    "dsm_window_finish_batch": (C.c_int, [_vp, C.c_int, C.POINTER(FinishJob), C.POINTER(LinearizeParams), C.POINTER(StepParams),
                                          C.POINTER(OptimizeParams)]),
    "dsm_window_finish_host": (C.c_int, [C.c_int, C.c_int, C.POINTER(FinishJob), C.POINTER(c_float_p), C.POINTER(LinearizeParams),
                                         C.POINTER(StepParams), C.POINTER(OptimizeParams)]),
    "dsm_diag_finish_prepare_host": (C.c_int, [C.POINTER(FinishJob), C.POINTER(LinearizeParams), C.POINTER(StepParams), c_float_p,
                                                 C.POINTER(LinearizeJob)]),
    "dsm_diag_finish_book_host": (C.c_int, [C.POINTER(FinishJob)]),
    "dsm_marginalize_params_default": (C.c_int, [C.POINTER(MarginalizeParams)]),
    "dsm_window_marginalize_batch": (C.c_int, [_vp, C.c_int, C.POINTER(MarginalizeJob), C.POINTER(LinearizeParams), C.POINTER(MarginalizeParams)]),
    "dsm_window_marginalize_host": (C.c_int, [C.c_int, C.c_int, C.POINTER(MarginalizeJob), C.POINTER(c_float_p), C.POINTER(LinearizeParams),
                                              C.POINTER(MarginalizeParams)]),
    "dsm_nullspace_params_default": (C.c_int, [C.POINTER(NullspaceParams)]),
    "dsm_window_nullspace_batch": (C.c_int, [_vp, C.c_int, C.POINTER(NullspaceJob), C.POINTER(NullspaceParams)]),
    "dsm_window_nullspace_host": (C.c_int, [C.c_int, C.POINTER(NullspaceJob), C.POINTER(NullspaceParams)]),
    "dsm_window_rescale_batch": (C.c_int, [_vp, C.c_int, C.POINTER(RescaleJob), C.POINTER(LinearizeParams), C.POINTER(StepParams)]),
    "dsm_window_rescale_host": (C.c_int, [C.c_int, C.POINTER(RescaleJob), C.POINTER(LinearizeParams), C.POINTER(StepParams)]),
    "dsm_rescale_geometry": (C.c_int, [c_int_p, c_int_p]),
    "dsm_admit_params_default": (None, [C.POINTER(AdmitParams)]),
    "dsm_window_admit_batch": (C.c_int, [_vp, C.c_int, C.POINTER(AdmitJob), C.POINTER(LinearizeParams), C.POINTER(StepParams), C.POINTER(AdmitParams)]),
    "dsm_window_admit_host": (C.c_int, [C.c_int, C.POINTER(AdmitJob), C.POINTER(LinearizeParams), C.POINTER(StepParams), C.POINTER(AdmitParams)]),
    "dsm_admit_geometry": (C.c_int, [c_int_p, c_int_p]),
    "dsm_write_trajectory": (C.c_int, [C.c_char_p, C.c_int, c_int_p, c_double_p]),
    "dsm_make_coarse_depth_l0": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, c_float_p, c_float_p, c_float_p, c_float_p, _pp_f, c_int_p, _pp_f, _pp_f, _pp_f, _pp_f]),
    "dsm_sc_distance": (C.c_float, [c_int_p, c_double_p, C.c_int, c_int_p, c_double_p, C.c_int, C.c_int]),
    "dsm_search_sc": (C.c_int, [c_int_p, c_double_p, C.c_int, C.c_int, c_int_p, _pp_i, _pp_d, c_int_p, C.c_int, c_int_p, c_float_p]),
}

_lib = None


def load():
    """Load libdsm_hotpath.so (built by __graft_entry__.build()).  Raises ImportError if absent."""
    global _lib
    if _lib is not None:
        return _lib
    # One HIP runtime per process: this image's PyTorch bundles its own libamdhip64.so (same SONAME
    # libamdhip64.so.7 as /opt/rocm's).  If torch is imported AFTER this library, the loader maps a
    # second copy of the runtime; imported before, ours resolves to the already loaded one.  So when
    # torch is installed, make sure it is loaded first (bench.py and the RCCL merge use it anyway).
    import sys

    if "torch" not in sys.modules:
        try:
            import torch  # noqa: F401
        except Exception:  # torch absent: plain /opt/rocm runtime
            pass
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        try:
            fn = getattr(L, name)  # AttributeError if the library does not export a declared symbol
        except AttributeError:
            if os.environ.get("DSM_HOTPATH_LIB") and os.environ.get("DSM_HOTPATH_LIB_OLDER_BUILD"):
                continue  # developer A/B against a build of an earlier commit (same ABI version, fewer entry points)
            raise
        fn.restype = res
        fn.argtypes = args
    # the struct layouts above are those of ABI version ABI_VERSION (include/dsm_hotpath.h: DSM_ABI_VERSION)
    have = L.dsm_abi_version()
    if have != ABI_VERSION:
        raise ImportError(f"{LIB_PATH} implements ABI version {have}, this binding was written for {ABI_VERSION}: rebuild the library")
    _lib = L
    return L


def check(rc):
    if rc != 0:
        msg = load().dsm_last_error()
        raise DsmError(f"dsm error {rc}: {msg.decode() if msg else ''}")
