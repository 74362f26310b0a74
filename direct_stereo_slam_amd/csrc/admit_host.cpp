// admit_host.cpp -- the host form of admitting the new keyframe into the window (dsm_window_admit_host) and the
// job rules both forms share (V).  The head of FrontEnd::makeKeyFrame (FrontEnd.cpp:722-762) with flagFramesForMarginalization
// (dso_helpers/FrontEndMarginalize.cpp:62-146) as plain loops over A1-A6; the expressions are admit_math.hpp and the headers it sits
// on, shared with the device kernel (admit_kernels.hip).  Plain C++; no device code.
#include <climits>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "admit_launch.hpp"
#include "dsm_internal.hpp"
#include "rescale_launch.hpp"

extern "C" void dsm_admit_params_default(dsm_admit_params *p) {
  if (!p) return;
  p->min_frames = 5, p->max_frames = 7, p->min_frame_age = 1, p->min_points_remaining = 0.05f, p->max_log_aff_fac_in_window = 0.7f;
}

namespace dsm {

// V of DESIGN.md section 26
const char *admit_job_error(const dsm_admit_job &J) {
  if (J.n_frames < 1 || J.n_frames > DSM_WINDOW_MAX_FRAMES - 1) return "n_frames outside [1, 15]: a window of DSM_WINDOW_MAX_FRAMES has no room";
  if (J.n_pts < 0 || J.n_res < 0) return "a negative n_pts or n_res";
  if ((long long)J.n_pts + J.n_res > INT_MAX) return "n_pts + n_res overflows";
  if (!J.world_to_cam_eval || !J.state || !J.state_zero || !J.exposure || !J.frame_energy_th || !J.keyframe_id || !J.n_points_in || !J.n_points_out)
    return "NULL frame input";
  if (!J.ref_cam_to_world || !J.cam_to_tracking_ref || !J.new_frame_prior || !J.new_frame_prior_zero || !J.calib_value || !J.calib_zero)
    return "NULL new-frame or calibration input";
  if (J.n_pts && (!J.host || !J.last_res || !J.last_state)) return "NULL point input";
  if (J.n_res && (!J.point || !J.target || !J.state_in || !J.energy_in || !J.is_new)) return "NULL residual input";
  if (!J.prior != !J.prior_zero) return "prior without prior_zero, or the reverse";
  if (!J.world_to_cam_eval_out || !J.state_out || !J.state_zero_out || !J.exposure_out || !J.frame_energy_th_out || !J.keyframe_id_out ||
      !J.world_to_cam_out || !J.flagged_out || !J.cam_to_world_out || !J.pre_RTll_0_out || !J.pre_tTll_0_out || !J.pre_KRKiTll_out || !J.pre_KtTll_out ||
      !J.pre_aff_mode_out || !J.pre_b0_mode_out || !J.cam_out || !J.c_delta_out || !J.delta_x_out || !J.ad_host_out || !J.ad_target_out ||
      !J.ad_ht_delta_out || !J.frame_prior_out || !J.frame_delta_prior_out || !J.n_res_out || !J.n_flagged || !J.dist_score_out)
    return "NULL required output";
  if ((J.H_M && !J.H_M_out) || (J.b_M && !J.b_M_out) || (J.H_L && !J.H_L_out) || (J.b_L && !J.b_L_out) || (J.prior && (!J.prior_out || !J.prior_zero_out)))
    return "NULL output of an optional array that is given";
  if (J.n_pts && (!J.new_res_index_out || !J.last_res_out || !J.last_state_out)) return "NULL point output";
  if (J.n_res && !J.res_index_out) return "NULL residual output";
  if ((J.n_pts || J.n_res) && (!J.point_out || !J.target_out || !J.res_state_out || !J.energy_out || !J.is_new_out)) return "NULL list output";
  const size_t n = J.n_frames, N = 4 + 8 * n, np = J.n_pts, nr = J.n_res;
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
  if (!std::isfinite(J.new_exposure) || !finite_f(J.exposure, n)) return "an exposure that is not finite";
  if (!std::isfinite(J.new_frame_energy_th) || !finite_f(J.frame_energy_th, n)) return "a non-finite frame_energy_th";
  if (!finite(J.world_to_cam_eval, 7 * n) || !finite(J.state, 8 * n) || !finite(J.state_zero, 8 * n)) return "a non-finite world_to_cam_eval, state or state_zero";
  if (!finite(J.ref_cam_to_world, 7) || !finite(J.cam_to_tracking_ref, 7) || !finite(J.aff_g2l, 2) || !finite(J.new_frame_prior, 8) ||
      !finite(J.new_frame_prior_zero, 8))
    return "a non-finite ref_cam_to_world, cam_to_tracking_ref, aff_g2l, new_frame_prior or new_frame_prior_zero";
  if (!finite(J.calib_value, 4) || !finite(J.calib_zero, 4)) return "a non-finite calibration input";
  if (!finite(J.H_M, N * N) || !finite(J.b_M, N) || !finite(J.H_L, N * N) || !finite(J.b_L, N) || !finite(J.prior, N) || !finite(J.prior_zero, N))
    return "a non-finite H_M, b_M, H_L, b_L, prior or prior_zero";
  if (!finite_f(J.energy_in, nr)) return "a non-finite energy_in";
  auto unit = [](const double *q) { return fabs(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3] - 1.0) <= 1e-9; };
  for (size_t f = 0; f < n; f++)
    if (!unit(J.world_to_cam_eval + 7 * f)) return "a world_to_cam_eval quaternion that is not of unit length (squared norm within 1e-9 of 1)";
  if (!unit(J.ref_cam_to_world) || !unit(J.cam_to_tracking_ref))
    return "a ref_cam_to_world or cam_to_tracking_ref quaternion that is not of unit length (squared norm within 1e-9 of 1)";
  for (size_t f = 0; f < n; f++) {
    if (J.n_points_in[f] < 0 || J.n_points_out[f] < 0) return "a negative n_points_in or n_points_out";
    if ((long long)J.n_points_in[f] + J.n_points_out[f] > INT_MAX) return "n_points_in + n_points_out overflows";
  }
  auto state = [](unsigned char s) { return s == DSM_RES_IN || s == DSM_RES_OOB || s == DSM_RES_OUTLIER; };
  for (size_t p = 0; p < np; p++)
    if (J.host[p] < 0 || J.host[p] >= J.n_frames) return "a host out of range";
  for (size_t r = 0; r < nr; r++) {
    if (J.point[r] < 0 || J.point[r] >= J.n_pts) return "a point out of range";
    if (J.target[r] < 0 || J.target[r] >= J.n_frames) return "a target out of range";
    if (J.target[r] == J.host[J.point[r]]) return "a target equal to its point's host";
    if (r && J.point[r] < J.point[r - 1]) return "residuals not grouped by ascending point";
    if (!state(J.state_in[r])) return "a state_in other than DSM_RES_IN / _OOB / _OUTLIER";
  }
  for (size_t p = 0; p < np; p++)
    for (int k = 0; k < 2; k++) {
      const int l = J.last_res[2 * p + k];
      if (l < -1 || l >= J.n_res) return "a last_res out of range";
      if (l >= 0 && J.point[l] != (int)p) return "a last_res that names another point's residual";
      if (!state(J.last_state[2 * p + k])) return "a last_state other than DSM_RES_IN / _OOB / _OUTLIER";
    }
  return nullptr;
}

int admit_check(const char *call, int n_jobs, const dsm_admit_job *jobs, const dsm_linearize_params *lp, const dsm_step_params *sp,
                const dsm_admit_params *ap, dsm_linearize_params &LP, dsm_step_params &SP, adm::Params &AP) {
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
  dsm_admit_params A;
  if (ap)
    A = *ap;
  else
    dsm_admit_params_default(&A);
  if (const char *e = linearize_params_error(&LP)) return bad(e);
  if (!(LP.scale_f > 0.0f) || !(LP.scale_c > 0.0f) || !(LP.scale_idepth > 0.0f)) return bad("a scale_f, scale_c or scale_idepth that is not positive");
  if (const char *e = step_params_error(&SP)) return bad(e);
  if (!std::isfinite(A.min_points_remaining) || !std::isfinite(A.max_log_aff_fac_in_window))
    return bad("a min_points_remaining or max_log_aff_fac_in_window that is not finite");
  if (A.min_frames < 0 || A.max_frames < 0) return bad("a negative min_frames or max_frames");
  AP = adm::Params{A.min_frames, A.max_frames, A.min_frame_age, A.min_points_remaining, A.max_log_aff_fac_in_window};
  for (int j = 0; j < n_jobs; j++)
    if (const char *e = admit_job_error(jobs[j])) return bad(e);
  return DSM_OK;
}

namespace {

void admit_one(const dsm_admit_job &J, const stp::Scales &S, const adm::Params &P) {
  const int n = J.n_frames, m = n + 1, np = J.n_pts, nr = J.n_res, N = 4 + 8 * n, M = N + 8;
  const size_t m2 = (size_t)m * m;
  // A1
  std::vector<double> eval(7 * (size_t)m), state(8 * (size_t)m), zero(8 * (size_t)m);
  std::vector<float> expo(m), eth(m);
  std::vector<int> ids(m);
  memcpy(eval.data(), J.world_to_cam_eval, 56 * (size_t)n), memcpy(state.data(), J.state, 64 * (size_t)n), memcpy(zero.data(), J.state_zero, 64 * (size_t)n);
  memcpy(expo.data(), J.exposure, 4 * (size_t)n), memcpy(eth.data(), J.frame_energy_th, 4 * (size_t)n), memcpy(ids.data(), J.keyframe_id, 4 * (size_t)n);
  double ctr[7], c2w[7];
  rsc::newest_frame(J.cam_to_tracking_ref, J.ref_cam_to_world, J.aff_g2l, 1.0f, S, ctr, c2w, &eval[7 * (size_t)n], &state[8 * (size_t)n]);
  memcpy(&zero[8 * (size_t)n], &state[8 * (size_t)n], 64);
  expo[n] = J.new_exposure, eth[n] = J.new_frame_energy_th, ids[n] = J.new_keyframe_id;
  // A2: section 22's Z3 on the primed values, and the distances
  float cam[6], c_delta[4];
  for (int c = 0; c < 4; c++) fin::calib_cam(c, J.calib_value[c], J.calib_zero[c], S, cam[c], c_delta[c]);
  cam[4] = stp::cam_inverse(cam[0]), cam[5] = stp::cam_inverse(cam[1]);
  std::vector<double> delta_f(8 * (size_t)m), aff(2 * (size_t)m), aff0(2 * (size_t)m), W(7 * (size_t)m), Cw(7 * (size_t)m), Ei(7 * (size_t)m);
  for (int k = 0; k < m; k++) {
    fin::frame_pose(&state[8 * (size_t)k], &zero[8 * (size_t)k], &eval[7 * (size_t)k], S, &delta_f[8 * (size_t)k], &aff[2 * (size_t)k], &aff0[2 * (size_t)k],
                    &W[7 * (size_t)k], &Cw[7 * (size_t)k]);
    stp::se3_inverse(&eval[7 * (size_t)k], &Ei[7 * (size_t)k]);
  }
  std::vector<float> R0(9 * m2, 0.0f), t0(3 * m2, 0.0f), Mx(9 * m2, 0.0f), Kt(3 * m2, 0.0f), am(2 * m2, 0.0f), b0(m2, 0.0f), dp(8 * m2, 0.0f), dist(m2, 0.0f);
  std::vector<double> AH(64 * m2), AT(64 * m2);
  for (int h = 0; h < m; h++)
    for (int t = 0; t < m; t++) {
      const size_t pr = (size_t)h * m + t;
      // A3: every pair, the diagonal too
      double Adj[36];
      fin::adjoint(&eval[7 * (size_t)t], &Ei[7 * (size_t)h], Adj);
      fin::adjoint_pair(Adj, fin::aff_a0(&aff0[2 * (size_t)h], &aff0[2 * (size_t)t], expo[h], expo[t]), S, &AH[64 * pr], &AT[64 * pr]);
      if (h == t) continue;
      stp::PairRow o;
      stp::pair_row(&eval[7 * (size_t)t], &Ei[7 * (size_t)h], &W[7 * (size_t)t], &Cw[7 * (size_t)h], cam, expo[h], expo[t], &aff[2 * (size_t)h], &aff[2 * (size_t)t],
                    zero[8 * (size_t)h + 7], S.b, o);
      memcpy(&R0[9 * pr], o.R0, 36), memcpy(&t0[3 * pr], o.t0, 12), memcpy(&Mx[9 * pr], o.M, 36), memcpy(&Kt[3 * pr], o.Kt, 12);
      am[2 * pr] = o.aff[0], am[2 * pr + 1] = o.aff[1], b0[pr] = o.b0;
      dist[pr] = adm::distance_ll(&W[7 * (size_t)t], &Cw[7 * (size_t)h]);
      for (int c = 0; c < 8; c++)
        dp[8 * pr + c] = ad_ht_delta_entry(&AH[64 * pr], &AT[64 * pr], &state[8 * (size_t)h], &zero[8 * (size_t)h], &state[8 * (size_t)t], &zero[8 * (size_t)t], c);
    }
  std::vector<double> dx(M);
  for (int c = 0; c < 4; c++) dx[c] = (double)c_delta[c]; // E1
  for (int i = 4; i < M; i++) dx[i] = delta_f[i - 4];
  // A4, over the n old frames
  std::vector<unsigned char> flagged(m, 0);
  std::vector<double> score(n, 0.0);
  if (adm::f0_branch(P)) {
    for (int i = 0; i < n; i++) flagged[i] = adm::f0_flagged(i, n, P);
  } else {
    int count = 0;
    for (int i = 0; i < n; i++)
      if (adm::f1_flagged(J.n_points_in[i], J.n_points_out[i], expo[n - 1], expo[i], &aff[2 * (size_t)(n - 1)], &aff[2 * (size_t)i], n, count, P))
        flagged[i] = 1, count++;
    if (n - count >= P.max_frames) {
      for (int h = 0; h < n; h++)
        if (adm::f2_candidate(ids[h], ids[n - 1], P)) score[h] = adm::f2_score(&dist[(size_t)h * m], ids.data(), h, n, P);
      const int pick = adm::f2_pick(score.data(), ids.data(), n, P);
      if (pick >= 0) flagged[pick] = 1;
    }
  }
  int n_flagged = 0;
  for (int i = 0; i < n; i++) n_flagged += flagged[i];
  // the outputs
  memcpy(J.world_to_cam_eval_out, eval.data(), 56 * (size_t)m), memcpy(J.state_out, state.data(), 64 * (size_t)m), memcpy(J.state_zero_out, zero.data(), 64 * (size_t)m);
  memcpy(J.exposure_out, expo.data(), 4 * (size_t)m), memcpy(J.frame_energy_th_out, eth.data(), 4 * (size_t)m), memcpy(J.keyframe_id_out, ids.data(), 4 * (size_t)m);
  memcpy(J.world_to_cam_out, W.data(), 56 * (size_t)m), memcpy(J.flagged_out, flagged.data(), m), memcpy(J.cam_to_world_out, c2w, 56);
  memcpy(J.pre_RTll_0_out, R0.data(), 36 * m2), memcpy(J.pre_tTll_0_out, t0.data(), 12 * m2), memcpy(J.pre_KRKiTll_out, Mx.data(), 36 * m2);
  memcpy(J.pre_KtTll_out, Kt.data(), 12 * m2), memcpy(J.pre_aff_mode_out, am.data(), 8 * m2), memcpy(J.pre_b0_mode_out, b0.data(), 4 * m2);
  if (J.distance_ll_out) memcpy(J.distance_ll_out, dist.data(), 4 * m2);
  memcpy(J.cam_out, cam, 24), memcpy(J.c_delta_out, c_delta, 16), memcpy(J.delta_x_out, dx.data(), 8 * (size_t)M);
  memcpy(J.ad_host_out, AH.data(), 512 * m2), memcpy(J.ad_target_out, AT.data(), 512 * m2), memcpy(J.ad_ht_delta_out, dp.data(), 32 * m2);
  *J.n_flagged = n_flagged, *J.n_res_out = nr + np;
  memcpy(J.dist_score_out, score.data(), 8 * (size_t)n);
  // A5
  auto grow_matrix = [&](const double *in, double *out) {
    for (int i = 0; i < M; i++)
      for (int j = 0; j < M; j++) out[(size_t)i * M + j] = i < N && j < N ? in[(size_t)i * N + j] : 0.0;
  };
  auto grow_vector = [&](const double *in, double *out, const double *tail) {
    for (int i = 0; i < M; i++) out[i] = i < N ? in[i] : tail ? tail[i - N] : 0.0;
  };
  if (J.H_M) grow_matrix(J.H_M, J.H_M_out);
  if (J.b_M) grow_vector(J.b_M, J.b_M_out, nullptr);
  if (J.H_L) grow_matrix(J.H_L, J.H_L_out);
  if (J.b_L) grow_vector(J.b_L, J.b_L_out, nullptr);
  if (J.prior) grow_vector(J.prior, J.prior_out, J.new_frame_prior), grow_vector(J.prior_zero, J.prior_zero_out, J.new_frame_prior_zero);
  for (int k = 0; k < 8; k++) J.frame_prior_out[k] = J.new_frame_prior[k], J.frame_delta_prior_out[k] = state[8 * (size_t)n + k] - J.new_frame_prior_zero[k];
  // A6
  for (int r = 0; r < nr; r++) {
    const int to = adm::old_index(r, J.point[r]);
    J.point_out[to] = J.point[r], J.target_out[to] = J.target[r], J.res_state_out[to] = J.state_in[r], J.energy_out[to] = J.energy_in[r];
    J.is_new_out[to] = J.is_new[r], J.res_index_out[r] = to;
  }
  for (int p = 0; p < np; p++) {
    const int to = adm::new_index(adm::run_end(J.point, nr, p), p), l0 = J.last_res[2 * p];
    J.point_out[to] = p, J.target_out[to] = n, J.res_state_out[to] = DSM_RES_IN, J.energy_out[to] = 0.0f, J.is_new_out[to] = 1;
    J.new_res_index_out[p] = to;
    J.last_res_out[2 * p] = to, J.last_res_out[2 * p + 1] = l0 >= 0 ? adm::old_index(l0, J.point[l0]) : -1;
    J.last_state_out[2 * p] = DSM_RES_IN, J.last_state_out[2 * p + 1] = J.last_state[2 * p];
  }
}

} // namespace
} // namespace dsm

extern "C" int dsm_admit_geometry(int *block, int *grid_stride) {
  if (!block || !grid_stride) return DSM_ERR_INVALID;
  *block = dsm::kAdmBlock, *grid_stride = dsm::kAdmBlock * dsm::kAdmListBlocks;
  return DSM_OK;
}

extern "C" int dsm_window_admit_host(int n_jobs, const dsm_admit_job *jobs, const dsm_linearize_params *lp, const dsm_step_params *sp,
                                     const dsm_admit_params *ap) {
  using namespace dsm;
  dsm_linearize_params LP;
  dsm_step_params SP;
  adm::Params AP;
  if (int rc = admit_check("dsm_window_admit_host", n_jobs, jobs, lp, sp, ap, LP, SP, AP)) return rc;
  const stp::Scales S = rescale_scales(LP, SP);
  for (int j = 0; j < n_jobs; j++) admit_one(jobs[j], S, AP);
  return DSM_OK;
}
