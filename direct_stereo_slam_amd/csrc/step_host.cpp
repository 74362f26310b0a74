// step_host.cpp -- the host form of the window optimisation's step (dsm_window_step_host) and the job rules both
// forms share (V).  The host form is D1-E3 as plain loops, then dsm_window_solve_host on the job completed with what the loops formed;
// the expressions are step_math.hpp, shared with the device kernels (step_kernels.hip).  Plain C++; no device code.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "dsm_internal.hpp"
#include "step_math.hpp"

namespace dsm {

const char *step_params_error(const dsm_step_params *p) {
  if (!p) return "no step parameters";
  const double v[5] = {p->scale_xi_trans, p->scale_xi_rot, p->scale_a, p->scale_b, p->th_opt_iterations};
  for (double x : v)
    if (!std::isfinite(x) || !(x > 0.0)) return "a step parameter that is not finite or not positive";
  return nullptr;
}

// V of DESIGN.md section 19: what this call refuses on top of the solve call's rules, which the caller applies to the completed job
const char *step_job_error(const dsm_step_job &J) {
  const dsm_linearize_job &L = J.sol.hes.lin;
  if (L.n_frames < 1 || L.n_frames > DSM_WINDOW_MAX_FRAMES || L.n_pts < 0) return "n_frames outside [1, 16] or a negative count";
  if (L.pre_RTll_0 || L.pre_tTll_0 || L.pre_KRKiTll || L.pre_KtTll || L.pre_aff_mode || L.pre_b0_mode)
    return "a precalc table given: this call forms them";
  if (L.idepth_scaled || L.idepth_zero_scaled) return "idepth_scaled or idepth_zero_scaled given: this call forms them";
  if (J.sol.hes.delta) return "hes.delta given: this call forms it";
  if (J.sol.delta_x) return "delta_x given: this call forms it";
  if (!J.world_to_cam_eval || !J.state_zero || !J.state_backup || !J.frame_step || !J.calib_zero || !J.calib_backup || !J.calib_step || !J.exposure)
    return "NULL frame or calibration input";
  if (L.n_pts && (!J.idepth_backup || !J.idepth_step)) return "NULL idepth_backup or idepth_step";
  if ((J.prior != nullptr) != (J.prior_zero != nullptr)) return "prior without prior_zero, or the reverse";
  if (!J.state_out || !J.calib_out || !J.world_to_cam_out || !J.can_break || !J.step_sums || !J.energy_m || (L.n_pts && !J.idepth_out))
    return "NULL required output";
  const size_t n = L.n_frames, N = 4 + 8 * n;
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
  if (!finite_f(J.stepfac, 5)) return "a step factor that is not finite";
  if (!finite(J.world_to_cam_eval, 7 * n) || !finite(J.state_zero, 8 * n) || !finite(J.state_backup, 8 * n) || !finite(J.frame_step, 8 * n))
    return "a non-finite world_to_cam_eval, state_zero, state_backup or frame_step";
  if (!finite(J.calib_zero, 4) || !finite(J.calib_backup, 4) || !finite(J.calib_step, 4)) return "a non-finite calibration input";
  if (!finite_f(J.exposure, n) || !finite_f(J.idepth_backup, L.n_pts) || !finite_f(J.idepth_step, L.n_pts))
    return "a non-finite exposure, idepth_backup or idepth_step";
  if (!finite(J.prior, N) || !finite(J.prior_zero, N)) return "a non-finite prior or prior_zero";
  for (size_t f = 0; f < n; f++) {
    const double *q = J.world_to_cam_eval + 7 * f;
    const double nn = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
    if (!(fabs(nn - 1.0) <= 1e-9)) return "a world_to_cam_eval quaternion that is not of unit length (squared norm within 1e-9 of 1)";
  }
  return nullptr;
}

} // namespace dsm

extern "C" int dsm_step_params_default(dsm_step_params *p) {
  if (!p) return DSM_ERR_INVALID;
  p->scale_xi_trans = 0.5, p->scale_xi_rot = 1.0, p->scale_a = 10.0, p->scale_b = 1000.0, p->th_opt_iterations = 1.2;
  return DSM_OK;
}

extern "C" int dsm_window_step_host(int w, int h, const dsm_step_job *job, const float *const *frame_I, const dsm_linearize_params *lp,
                                    const dsm_step_params *sp) {
  using namespace dsm;
  auto fail = [](const char *msg) {
    set_error(std::string("dsm_window_step_host: ") + msg);
    return DSM_ERR_INVALID;
  };
  if (w < 8 || h < 8 || !job || !frame_I) return fail("bad argument");
  if (const char *e = linearize_params_error(lp)) return fail(e);
  if (const char *e = step_params_error(sp)) return fail(e);
  if (const char *e = step_job_error(*job)) return fail(e);
  const dsm_step_job &J = *job;
  const int n = J.sol.hes.lin.n_frames, np = J.sol.hes.lin.n_pts, N = 4 + 8 * n;
  const stp::Scales S{sp->scale_xi_trans, sp->scale_xi_rot, sp->scale_a, sp->scale_b, sp->th_opt_iterations, lp->scale_f, lp->scale_c, lp->scale_idepth};

  double calib[4];
  float cam[6], c_delta[4];
  for (int c = 0; c < 4; c++) // D1
    stp::calib_entry(c, J.calib_backup[c], J.stepfac[0], J.calib_step[c], J.calib_zero[c], S, calib[c], cam[c], c_delta[c]);
  cam[4] = stp::cam_inverse(cam[0]), cam[5] = stp::cam_inverse(cam[1]);

  std::vector<double> state(8 * (size_t)n), delta_f(8 * (size_t)n), aff(2 * (size_t)n), W(7 * (size_t)n), Cw(7 * (size_t)n), Ei(7 * (size_t)n);
  for (int f = 0; f < n; f++) { // D2
    stp::frame_state(J.state_backup + 8 * f, J.frame_step + 8 * f, J.state_zero + 8 * f, J.world_to_cam_eval + 7 * f, J.stepfac, S, &state[8 * f],
                     &delta_f[8 * f], &aff[2 * f], &W[7 * f], &Cw[7 * f]);
    stp::se3_inverse(J.world_to_cam_eval + 7 * f, &Ei[7 * f]);
  }

  std::vector<float> idepth((size_t)np + 1), ids((size_t)np + 1); // D3
  for (int p = 0; p < np; p++) {
    idepth[p] = stp::point_idepth(J.idepth_backup[p], J.stepfac[4], J.idepth_step[p]);
    ids[p] = stp::point_idepth_scaled(S.idepth, idepth[p]);
  }

  float sums[6]; // D4
  stp::frame_sums(J.frame_step, n, sums);
  stp::point_sums(J.idepth_backup, J.idepth_step, np, sums + 4);
  const int can_break = stp::can_break(sums, S.th);

  const size_t n2 = (size_t)n * n; // Q1-Q4; the diagonal stays zero
  std::vector<float> R0(9 * n2, 0.0f), t0(3 * n2, 0.0f), M(9 * n2, 0.0f), Kt(3 * n2, 0.0f), am(2 * n2, 0.0f), b0(n2, 0.0f);
  for (int hh = 0; hh < n; hh++)
    for (int t = 0; t < n; t++) {
      if (hh == t) continue;
      stp::PairRow o;
      stp::pair_row(J.world_to_cam_eval + 7 * t, &Ei[7 * hh], &W[7 * t], &Cw[7 * hh], cam, J.exposure[hh], J.exposure[t], &aff[2 * hh], &aff[2 * t],
                    J.state_zero[8 * hh + 7], S.b, o);
      const size_t pr = (size_t)hh * n + t;
      memcpy(&R0[9 * pr], o.R0, 36), memcpy(&t0[3 * pr], o.t0, 12), memcpy(&M[9 * pr], o.M, 36), memcpy(&Kt[3 * pr], o.Kt, 12);
      am[2 * pr] = o.aff[0], am[2 * pr + 1] = o.aff[1], b0[pr] = o.b0;
    }

  std::vector<double> dx(N), HL(J.sol.H_L ? (size_t)N * N : 0), bL(J.sol.b_L ? N : 0);
  for (int c = 0; c < 4; c++) dx[c] = (double)c_delta[c]; // E1
  for (int i = 4; i < N; i++) dx[i] = delta_f[i - 4];
  double energy_m = 0.0; // E2
  for (int i = 0; i < N; i++) energy_m += stp::energy_m_term(J.sol.H_M ? J.sol.H_M + (size_t)i * N : nullptr, J.sol.b_M, dx.data(), i, N);
  if (J.sol.H_L) memcpy(HL.data(), J.sol.H_L, 8 * (size_t)N * N);
  if (J.sol.b_L) memcpy(bL.data(), J.sol.b_L, 8 * (size_t)N);
  if (J.prior && J.sol.H_L && J.sol.b_L)
    for (int i = 0; i < N; i++) { // E3
      const double dp = i < 4 ? (double)c_delta[i] : state[i - 4] - J.prior_zero[i];
      HL[(size_t)i * N + i] = stp::prior_h(HL[(size_t)i * N + i], J.prior[i]);
      bL[i] = stp::prior_b(bL[i], J.prior[i], dp);
    }

  dsm_solve_job T = J.sol; // the completed job
  dsm_linearize_job &L = T.hes.lin;
  memcpy(L.cam, cam, 16), memcpy(L.cam_inv, cam + 4, 8);
  L.pre_RTll_0 = R0.data(), L.pre_tTll_0 = t0.data(), L.pre_KRKiTll = M.data(), L.pre_KtTll = Kt.data(), L.pre_aff_mode = am.data(), L.pre_b0_mode = b0.data();
  L.idepth_scaled = ids.data(), L.idepth_zero_scaled = ids.data();
  T.delta_x = dx.data();
  if (J.sol.H_L) T.H_L = HL.data();
  if (J.sol.b_L) T.b_L = bL.data();
  if (int rc = dsm_window_solve_host(w, h, &T, frame_I, lp)) return rc;

  memcpy(J.state_out, state.data(), 64 * (size_t)n), memcpy(J.calib_out, calib, 32), memcpy(J.world_to_cam_out, W.data(), 56 * (size_t)n);
  if (np) memcpy(J.idepth_out, idepth.data(), 4 * (size_t)np);
  if (J.cam_to_world_out) memcpy(J.cam_to_world_out, Cw.data(), 56 * (size_t)n);
  *J.can_break = can_break, memcpy(J.step_sums, sums, 24), *J.energy_m = energy_m;
  if (J.cam_out) memcpy(J.cam_out, cam, 24);
  if (J.pre_RTll_0_out) memcpy(J.pre_RTll_0_out, R0.data(), 36 * n2);
  if (J.pre_tTll_0_out) memcpy(J.pre_tTll_0_out, t0.data(), 12 * n2);
  if (J.pre_KRKiTll_out) memcpy(J.pre_KRKiTll_out, M.data(), 36 * n2);
  if (J.pre_KtTll_out) memcpy(J.pre_KtTll_out, Kt.data(), 12 * n2);
  if (J.pre_aff_mode_out) memcpy(J.pre_aff_mode_out, am.data(), 8 * n2);
  if (J.pre_b0_mode_out) memcpy(J.pre_b0_mode_out, b0.data(), 4 * n2);
  if (J.delta_x_out) memcpy(J.delta_x_out, dx.data(), 8 * (size_t)N);
  if (J.H_L_out) memcpy(J.H_L_out, HL.data(), 8 * (size_t)N * N);
  if (J.b_L_out) memcpy(J.b_L_out, bL.data(), 8 * (size_t)N);
  return DSM_OK;
}
