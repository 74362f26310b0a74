// rescale_host.cpp -- the host form of adopting the stereo scale into the window (dsm_window_rescale_host) and the
// job rules both forms share (V, S0, S1, S6).  FrontEnd::optimizeScale behind its scale search (FrontEnd.cpp:1010-1061, gated at :806)
// as plain loops over S2-S4; the expressions are rescale_math.hpp, shared with the device kernel (rescale_kernels.hip).  Plain C++; no
// device code.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "dsm_internal.hpp"
#include "rescale_launch.hpp"

namespace dsm {

// V of DESIGN.md section 25
const char *rescale_job_error(const dsm_rescale_job &J) {
  if (J.n_frames < 1 || J.n_frames > DSM_WINDOW_MAX_FRAMES || J.n_pts < 0) return "n_frames outside [1, 16] or a negative n_pts";
  if (!J.world_to_cam_eval || !J.state || !J.state_zero || !J.exposure || !J.cam_to_tracking_ref || !J.ref_cam_to_world || !J.cam_to_world ||
      !J.calib_value || !J.calib_zero || !J.ad_host || !J.ad_target)
    return "NULL frame, pose, calibration or adjoint input";
  if (!J.pre_RTll_0 || !J.pre_tTll_0 || !J.pre_KRKiTll || !J.pre_KtTll || !J.pre_aff_mode || !J.pre_b0_mode || !J.cam || !J.c_delta || !J.delta_x ||
      !J.ad_ht_delta || !J.world_to_cam)
    return "NULL given table";
  if (J.n_pts && (!J.idepth || !J.idepth_scaled || !J.idepth_zero_scaled || !J.delta)) return "NULL point input";
  if (J.n_pts && (!J.idepth_out || !J.idepth_scaled_out || !J.idepth_zero_scaled_out || !J.delta_out)) return "NULL point output";
  if (!J.world_to_cam_eval_out || !J.state_out || !J.state_zero_out || !J.cam_to_tracking_ref_out || !J.cam_to_world_out || !J.pre_RTll_0_out ||
      !J.pre_tTll_0_out || !J.pre_KRKiTll_out || !J.pre_KtTll_out || !J.pre_aff_mode_out || !J.pre_b0_mode_out || !J.cam_out || !J.c_delta_out ||
      !J.delta_x_out || !J.ad_ht_delta_out || !J.world_to_cam_out || !J.decision || !J.scale_error_out || !J.trapped_out || !J.fails_out ||
      !J.applied_scale)
    return "NULL required output";
  if (J.cam_to_world_out_all && !J.cam_to_world_all) return "cam_to_world_out_all without cam_to_world_all";
  if (!std::isfinite(J.new_scale) || J.new_scale == 0.0f) return "a new_scale that is not finite or 0";
  if (!std::isfinite(J.thres)) return "a non-finite thres";
  if (J.fails < 0) return "a negative fails";
  const size_t n = J.n_frames, n2 = n * n, N = 4 + 8 * n, np = J.n_pts;
  auto finite = [](const double *a, size_t m) {
    for (size_t i = 0; a && i < m; i++)
      if (!std::isfinite(a[i])) return false;
    return true;
  };
  auto finite_f = [](const float *a, size_t m) {
    for (size_t i = 0; a && i < m; i++)
      if (!std::isfinite(a[i])) return false;
    return true;
  };
  if (!finite_f(J.idepth, np) || !finite_f(J.idepth_scaled, np) || !finite_f(J.idepth_zero_scaled, np) || !finite_f(J.delta, np))
    return "a non-finite point input";
  if (!finite(J.world_to_cam_eval, 7 * n) || !finite(J.state, 8 * n) || !finite(J.state_zero, 8 * n) || !finite_f(J.exposure, n))
    return "a non-finite world_to_cam_eval, state, state_zero or exposure";
  if (!finite(J.cam_to_tracking_ref, 7) || !finite(J.ref_cam_to_world, 7) || !finite(J.cam_to_world, 7) || !finite(J.aff_g2l, 2))
    return "a non-finite cam_to_tracking_ref, ref_cam_to_world, cam_to_world or aff_g2l";
  if (!finite(J.calib_value, 4) || !finite(J.calib_zero, 4)) return "a non-finite calibration input";
  if (!finite(J.ad_host, 64 * n2) || !finite(J.ad_target, 64 * n2)) return "a non-finite ad_host or ad_target";
  if (!finite_f(J.pre_RTll_0, 9 * n2) || !finite_f(J.pre_tTll_0, 3 * n2) || !finite_f(J.pre_KRKiTll, 9 * n2) || !finite_f(J.pre_KtTll, 3 * n2) ||
      !finite_f(J.pre_aff_mode, 2 * n2) || !finite_f(J.pre_b0_mode, n2) || !finite_f(J.cam, 6) || !finite_f(J.c_delta, 4) || !finite(J.delta_x, N) ||
      !finite_f(J.ad_ht_delta, 8 * n2) || !finite(J.world_to_cam, 7 * n) || !finite(J.cam_to_world_all, 7 * n))
    return "a non-finite given table";
  auto unit = [](const double *q) { return fabs(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3] - 1.0) <= 1e-9; };
  for (size_t f = 0; f < n; f++)
    if (!unit(J.world_to_cam_eval + 7 * f)) return "a world_to_cam_eval quaternion that is not of unit length (squared norm within 1e-9 of 1)";
  if (!unit(J.cam_to_tracking_ref) || !unit(J.ref_cam_to_world) || !unit(J.cam_to_world))
    return "a cam_to_tracking_ref, ref_cam_to_world or cam_to_world quaternion that is not of unit length (squared norm within 1e-9 of 1)";
  return nullptr;
}

int rescale_check(const char *call, int n_jobs, const dsm_rescale_job *jobs, const dsm_linearize_params *lp, const dsm_step_params *sp,
                  dsm_linearize_params &LP, dsm_step_params &SP) {
  auto bad = [call](const char *msg) { return invalid((std::string(call) + ": " + msg).c_str()); };
  if (n_jobs < 1 || !jobs) return bad("bad argument");
  if (lp)
    LP = *lp;
  else
    dsm_linearize_params_default(&LP);
  if (sp)
    SP = *sp;
  else
    dsm_step_params_default(&SP);
  if (const char *e = linearize_params_error(&LP)) return bad(e);
  if (!(LP.scale_f > 0.0f) || !(LP.scale_c > 0.0f) || !(LP.scale_idepth > 0.0f)) return bad("a scale_f, scale_c or scale_idepth that is not positive");
  if (const char *e = step_params_error(&SP)) return bad(e);
  for (int j = 0; j < n_jobs; j++)
    if (const char *e = rescale_job_error(jobs[j])) return bad(e);
  return DSM_OK;
}

stp::Scales rescale_scales(const dsm_linearize_params &LP, const dsm_step_params &SP) {
  return stp::Scales{SP.scale_xi_trans, SP.scale_xi_rot, SP.scale_a, SP.scale_b, SP.th_opt_iterations, LP.scale_f, LP.scale_c, LP.scale_idepth};
}

int rescale_decide(const dsm_rescale_job &J) {
  const rsc::Decision d = rsc::decide(J.enabled, J.scale_error, J.new_scale, J.thres, J.trapped, J.fails);
  *J.decision = d.decision, *J.scale_error_out = d.scale_error, *J.trapped_out = d.trapped, *J.fails_out = d.fails;
  *J.applied_scale = d.decision == DSM_RESCALE_ACCEPTED ? J.new_scale : 1.0f;
  return d.decision;
}

void rescale_copy_through(const dsm_rescale_job &J) {
  const size_t n = J.n_frames, n2 = n * n, N = 4 + 8 * n, np = J.n_pts;
  auto copy = [](void *to, const void *from, size_t bytes) {
    if (bytes && to != from) memmove(to, from, bytes);
  };
  copy(J.idepth_out, J.idepth, 4 * np), copy(J.idepth_scaled_out, J.idepth_scaled, 4 * np);
  copy(J.idepth_zero_scaled_out, J.idepth_zero_scaled, 4 * np), copy(J.delta_out, J.delta, 4 * np);
  copy(J.world_to_cam_eval_out, J.world_to_cam_eval, 56 * n), copy(J.state_out, J.state, 64 * n), copy(J.state_zero_out, J.state_zero, 64 * n);
  copy(J.cam_to_tracking_ref_out, J.cam_to_tracking_ref, 56), copy(J.cam_to_world_out, J.cam_to_world, 56);
  copy(J.pre_RTll_0_out, J.pre_RTll_0, 36 * n2), copy(J.pre_tTll_0_out, J.pre_tTll_0, 12 * n2), copy(J.pre_KRKiTll_out, J.pre_KRKiTll, 36 * n2);
  copy(J.pre_KtTll_out, J.pre_KtTll, 12 * n2), copy(J.pre_aff_mode_out, J.pre_aff_mode, 8 * n2), copy(J.pre_b0_mode_out, J.pre_b0_mode, 4 * n2);
  copy(J.cam_out, J.cam, 24), copy(J.c_delta_out, J.c_delta, 16), copy(J.delta_x_out, J.delta_x, 8 * N), copy(J.ad_ht_delta_out, J.ad_ht_delta, 32 * n2);
  copy(J.world_to_cam_out, J.world_to_cam, 56 * n);
  if (J.cam_to_world_out_all) copy(J.cam_to_world_out_all, J.cam_to_world_all, 56 * n);
}

namespace {

void rescale_one(const dsm_rescale_job &J, const stp::Scales &S) {
  const int n = J.n_frames, np = J.n_pts, N = 4 + 8 * n, f = n - 1;
  const size_t n2 = (size_t)n * n;
  // S2
  for (int p = 0; p < np; p++) {
    const float id = rsc::point_idepth(J.idepth[p], J.new_scale), ids = stp::point_idepth_scaled(S.idepth, id);
    J.idepth_out[p] = id, J.idepth_scaled_out[p] = ids, J.idepth_zero_scaled_out[p] = ids, J.delta_out[p] = 0.0f;
  }
  // S3
  std::vector<double> eval(J.world_to_cam_eval, J.world_to_cam_eval + 7 * (size_t)n), state(J.state, J.state + 8 * (size_t)n),
      zero(J.state_zero, J.state_zero + 8 * (size_t)n);
  double ctr[7], c2w[7];
  rsc::newest_frame(J.cam_to_tracking_ref, J.ref_cam_to_world, J.aff_g2l, J.new_scale, S, ctr, c2w, &eval[7 * (size_t)f], &state[8 * (size_t)f]);
  memcpy(&zero[8 * (size_t)f], &state[8 * (size_t)f], 64);
  // S4: section 22's Z3 on the primed values
  float cam[6], c_delta[4];
  for (int c = 0; c < 4; c++) fin::calib_cam(c, J.calib_value[c], J.calib_zero[c], S, cam[c], c_delta[c]);
  cam[4] = stp::cam_inverse(cam[0]), cam[5] = stp::cam_inverse(cam[1]);
  std::vector<double> delta_f(8 * (size_t)n), aff(2 * (size_t)n), aff0(2 * (size_t)n), W(7 * (size_t)n), Cw(7 * (size_t)n), Ei(7 * (size_t)n);
  for (int k = 0; k < n; k++) {
    fin::frame_pose(&state[8 * (size_t)k], &zero[8 * (size_t)k], &eval[7 * (size_t)k], S, &delta_f[8 * (size_t)k], &aff[2 * (size_t)k], &aff0[2 * (size_t)k],
                    &W[7 * (size_t)k], &Cw[7 * (size_t)k]);
    stp::se3_inverse(&eval[7 * (size_t)k], &Ei[7 * (size_t)k]);
  }
  std::vector<float> R0(9 * n2, 0.0f), t0(3 * n2, 0.0f), M(9 * n2, 0.0f), Kt(3 * n2, 0.0f), am(2 * n2, 0.0f), b0(n2, 0.0f), dp(8 * n2, 0.0f);
  for (int hh = 0; hh < n; hh++)
    for (int t = 0; t < n; t++) {
      if (hh == t) continue;
      stp::PairRow o;
      stp::pair_row(&eval[7 * (size_t)t], &Ei[7 * (size_t)hh], &W[7 * (size_t)t], &Cw[7 * (size_t)hh], cam, J.exposure[hh], J.exposure[t], &aff[2 * (size_t)hh],
                    &aff[2 * (size_t)t], zero[8 * (size_t)hh + 7], S.b, o);
      const size_t pr = (size_t)hh * n + t;
      memcpy(&R0[9 * pr], o.R0, 36), memcpy(&t0[3 * pr], o.t0, 12), memcpy(&M[9 * pr], o.M, 36), memcpy(&Kt[3 * pr], o.Kt, 12);
      am[2 * pr] = o.aff[0], am[2 * pr + 1] = o.aff[1], b0[pr] = o.b0;
      for (int c = 0; c < 8; c++)
        dp[8 * pr + c] = ad_ht_delta_entry(J.ad_host + 64 * pr, J.ad_target + 64 * pr, &state[8 * (size_t)hh], &zero[8 * (size_t)hh], &state[8 * (size_t)t],
                                           &zero[8 * (size_t)t], c);
    }
  std::vector<double> dx(N);
  for (int c = 0; c < 4; c++) dx[c] = (double)c_delta[c]; // E1
  for (int i = 4; i < N; i++) dx[i] = delta_f[i - 4];
  // the outputs last: an output may be the array its input is
  memcpy(J.world_to_cam_eval_out, eval.data(), 56 * (size_t)n), memcpy(J.state_out, state.data(), 64 * (size_t)n);
  memcpy(J.state_zero_out, zero.data(), 64 * (size_t)n), memcpy(J.cam_to_tracking_ref_out, ctr, 56), memcpy(J.cam_to_world_out, c2w, 56);
  memcpy(J.pre_RTll_0_out, R0.data(), 36 * n2), memcpy(J.pre_tTll_0_out, t0.data(), 12 * n2), memcpy(J.pre_KRKiTll_out, M.data(), 36 * n2);
  memcpy(J.pre_KtTll_out, Kt.data(), 12 * n2), memcpy(J.pre_aff_mode_out, am.data(), 8 * n2), memcpy(J.pre_b0_mode_out, b0.data(), 4 * n2);
  memcpy(J.cam_out, cam, 24), memcpy(J.c_delta_out, c_delta, 16), memcpy(J.delta_x_out, dx.data(), 8 * (size_t)N);
  memcpy(J.ad_ht_delta_out, dp.data(), 32 * n2), memcpy(J.world_to_cam_out, W.data(), 56 * (size_t)n);
  if (J.cam_to_world_out_all) memcpy(J.cam_to_world_out_all, Cw.data(), 56 * (size_t)n);
}

} // namespace
} // namespace dsm

extern "C" int dsm_rescale_geometry(int *block, int *grid_stride) {
  if (!block || !grid_stride) return DSM_ERR_INVALID;
  *block = dsm::kRscBlock, *grid_stride = dsm::kRscBlock * dsm::kRscPointBlocks;
  return DSM_OK;
}

extern "C" int dsm_window_rescale_host(int n_jobs, const dsm_rescale_job *jobs, const dsm_linearize_params *lp, const dsm_step_params *sp) {
  using namespace dsm;
  dsm_linearize_params LP;
  dsm_step_params SP;
  if (int rc = rescale_check("dsm_window_rescale_host", n_jobs, jobs, lp, sp, LP, SP)) return rc;
  const stp::Scales S = rescale_scales(LP, SP);
  for (int j = 0; j < n_jobs; j++) {
    if (rescale_decide(jobs[j]) == DSM_RESCALE_ACCEPTED)
      rescale_one(jobs[j], S);
    else
      rescale_copy_through(jobs[j]);
  }
  return DSM_OK;
}
