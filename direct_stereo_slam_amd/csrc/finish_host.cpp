// finish_host.cpp -- the host form of the end of optimize behind its loop (dsm_window_finish_host) and the job
// rules both forms share (V).  The host form is dsm_window_optimize_host, then Z1-Z3 as plain loops over finish_math.hpp (shared with
// the device kernels, finish_kernels.hip; dsm_diag_finish_prepare_host), dsm_linearize_residuals_host with the fix flag (Z4), then
// Z5-Z8 as plain loops (dsm_diag_finish_book_host).  The two halves are also diagnostic exports (dsm_diag_*, not a maintained
// interface): the route that runs the loop and the final linearisation as separate device calls, which tools/finish_timing.py times.  Plain C++; no device code.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "dsm_internal.hpp"
#include "finish_math.hpp"

namespace dsm {

// V of DESIGN.md section 22: what both forms refuse on top of the optimize call's rules.  Looks at nothing the optimize call's rules
// have not seen unless it checks it itself, so it may run before them
const char *finish_job_error(const dsm_finish_job &J) {
  const dsm_linearize_job &L = J.opt.step.sol.hes.lin;
  if (L.n_frames < 1 || L.n_frames > DSM_WINDOW_MAX_FRAMES || L.n_pts < 0 || L.n_res < 0) return "n_frames outside [1, 16] or a negative count";
  if (!J.world_to_cam_eval_out || !J.state_zero_out || !J.state_out || !J.ad_host_out || !J.ad_target_out || !J.ad_ht_delta_out || !J.c_delta_out ||
      !J.delta_x_out || !J.pre_RTll_0_out || !J.pre_tTll_0_out || !J.pre_KRKiTll_out || !J.pre_KtTll_out || !J.pre_aff_mode_out || !J.pre_b0_mode_out ||
      !J.cam_out || !J.energy || !J.frame_energy_th_out || !J.n_res_out || !J.n_pts_out || !J.rmse || !J.lost)
    return "NULL required output of the finish";
  if (L.n_res && (!L.is_new || !J.new_state || !J.new_energy || !J.new_energy_with_outlier || !J.keep || !J.rel_bs || !J.res_index_out))
    return "NULL per-residual array of the finish";
  if (L.n_pts && (!J.n_good_residuals_in || !J.max_rel_baseline_in || !J.last_res || !J.last_state_in || !J.n_good_residuals_out ||
                  !J.max_rel_baseline_out || !J.last_res_out || !J.last_state_out || !J.n_res_kept || !J.point_dropped || !J.point_index_out))
    return "NULL per-point array of the finish";
  for (int p = 0; p < L.n_pts; p++) {
    if (J.n_good_residuals_in[p] < 0) return "a negative n_good_residuals_in";
    if (!std::isfinite(J.max_rel_baseline_in[p])) return "a non-finite max_rel_baseline_in";
    for (int s = 0; s < 2; s++) {
      const int r = J.last_res[2 * p + s], st = J.last_state_in[2 * p + s];
      if (r < -1 || r >= L.n_res) return "a last_res outside [-1, n_res)";
      if (r >= 0 && (!L.point || L.point[r] != p)) return "a last_res that names a residual of another point";
      if (st != DSM_RES_IN && st != DSM_RES_OOB && st != DSM_RES_OUTLIER) return "a last_state_in that is no residual state";
    }
  }
  return nullptr;
}

} // namespace dsm

namespace {

struct HostRes { // the final linearisation as finish_math.hpp's point_book asks for it
  const unsigned char *keep_, *is_new_, *state_;
  const float *rel_;
  bool keep(int r) const { return keep_[r] != 0; }
  bool is_new(int r) const { return is_new_[r] != 0; }
  float rel_bs(int r) const { return rel_[r]; }
  int new_state(int r) const { return state_[r]; }
};

} // namespace

extern "C" int dsm_diag_finish_prepare_host(const dsm_finish_job *job, const dsm_linearize_params *lp, const dsm_step_params *sp, float *scratch,
                                              dsm_linearize_job *lin) {
  using namespace dsm;
  auto fail = [](const char *msg) {
    set_error(std::string("dsm_diag_finish_prepare_host: ") + msg);
    return DSM_ERR_INVALID;
  };
  if (!job || !scratch || !lin) return fail("bad argument");
  if (const char *e = linearize_params_error(lp)) return fail(e);
  if (const char *e = step_params_error(sp)) return fail(e);
  if (const char *e = optimize_job_error(job->opt)) return fail(e);
  if (const char *e = finish_job_error(*job)) return fail(e);
  const dsm_finish_job &J = *job;
  const dsm_step_job &T = J.opt.step;
  const dsm_linearize_job &L0 = T.sol.hes.lin;
  if (!T.world_to_cam_eval || !T.state_zero || !T.calib_zero || !T.exposure || !T.state_out || !T.calib_out || !T.world_to_cam_out ||
      !T.sol.hes.ad_host || !T.sol.hes.ad_target || !L0.frame_energy_th || (L0.n_pts && !T.idepth_out) || (L0.n_res && (!L0.new_state || !L0.new_energy)))
    return fail("NULL array of the optimize job");
  const int n = L0.n_frames, np = L0.n_pts, N = 4 + 8 * n, f = n - 1;
  const size_t n2 = (size_t)n * n;
  const stp::Scales S{sp->scale_xi_trans, sp->scale_xi_rot, sp->scale_a, sp->scale_b, sp->th_opt_iterations, lp->scale_f, lp->scale_c, lp->scale_idepth};

  // Z1
  std::vector<double> eval(T.world_to_cam_eval, T.world_to_cam_eval + 7 * (size_t)n), zero(T.state_zero, T.state_zero + 8 * (size_t)n),
      state(T.state_out, T.state_out + 8 * (size_t)n);
  memcpy(&eval[7 * (size_t)f], T.world_to_cam_out + 7 * (size_t)f, 56);
  fin::newest_state(T.state_out + 8 * (size_t)f, &state[8 * (size_t)f]);
  memcpy(&zero[8 * (size_t)f], &state[8 * (size_t)f], 64);

  // Z3's frames and calibration
  float cam[6], c_delta[4];
  for (int c = 0; c < 4; c++) fin::calib_cam(c, T.calib_out[c], T.calib_zero[c], S, cam[c], c_delta[c]);
  cam[4] = stp::cam_inverse(cam[0]), cam[5] = stp::cam_inverse(cam[1]);
  std::vector<double> delta_f(8 * (size_t)n), aff(2 * (size_t)n), aff0(2 * (size_t)n), W(7 * (size_t)n), Cw(7 * (size_t)n), Ei(7 * (size_t)n);
  for (int k = 0; k < n; k++) {
    fin::frame_pose(&state[8 * (size_t)k], &zero[8 * (size_t)k], &eval[7 * (size_t)k], S, &delta_f[8 * (size_t)k], &aff[2 * (size_t)k], &aff0[2 * (size_t)k],
                    &W[7 * (size_t)k], &Cw[7 * (size_t)k]);
    stp::se3_inverse(&eval[7 * (size_t)k], &Ei[7 * (size_t)k]);
  }

  // Z2: the pairs of the newest frame; every other pair is the job's
  double *AH = J.ad_host_out, *AT = J.ad_target_out;
  memcpy(AH, T.sol.hes.ad_host, 512 * n2), memcpy(AT, T.sol.hes.ad_target, 512 * n2);
  for (int hh = 0; hh < n; hh++)
    for (int t = 0; t < n; t++) {
      if (hh != f && t != f) continue;
      double Adj[36];
      fin::adjoint(&eval[7 * (size_t)t], &Ei[7 * (size_t)hh], Adj);
      const double a = fin::aff_a0(&aff0[2 * (size_t)hh], &aff0[2 * (size_t)t], T.exposure[hh], T.exposure[t]);
      fin::adjoint_pair(Adj, a, S, AH + 64 * ((size_t)hh * n + t), AT + 64 * ((size_t)hh * n + t));
    }

  // Z3: Q1-Q4, the diagonal stays zero; adHTdeltaF likewise
  float *R0 = J.pre_RTll_0_out, *t0 = J.pre_tTll_0_out, *M = J.pre_KRKiTll_out, *Kt = J.pre_KtTll_out, *am = J.pre_aff_mode_out, *b0 = J.pre_b0_mode_out;
  float *dp = J.ad_ht_delta_out;
  memset(R0, 0, 36 * n2), memset(t0, 0, 12 * n2), memset(M, 0, 36 * n2), memset(Kt, 0, 12 * n2), memset(am, 0, 8 * n2), memset(b0, 0, 4 * n2);
  memset(dp, 0, 32 * n2);
  for (int hh = 0; hh < n; hh++)
    for (int t = 0; t < n; t++) {
      if (hh == t) continue;
      stp::PairRow o;
      stp::pair_row(&eval[7 * (size_t)t], &Ei[7 * (size_t)hh], &W[7 * (size_t)t], &Cw[7 * (size_t)hh], cam, T.exposure[hh], T.exposure[t], &aff[2 * (size_t)hh],
                    &aff[2 * (size_t)t], zero[8 * (size_t)hh + 7], S.b, o);
      const size_t pr = (size_t)hh * n + t;
      memcpy(&R0[9 * pr], o.R0, 36), memcpy(&t0[3 * pr], o.t0, 12), memcpy(&M[9 * pr], o.M, 36), memcpy(&Kt[3 * pr], o.Kt, 12);
      am[2 * pr] = o.aff[0], am[2 * pr + 1] = o.aff[1], b0[pr] = o.b0;
      for (int c = 0; c < 8; c++)
        dp[8 * pr + c] = ad_ht_delta_entry(&AH[64 * pr], &AT[64 * pr], &state[8 * (size_t)hh], &zero[8 * (size_t)hh], &state[8 * (size_t)t], &zero[8 * (size_t)t], c);
    }
  for (int c = 0; c < 4; c++) J.delta_x_out[c] = (double)c_delta[c]; // E1
  for (int i = 4; i < N; i++) J.delta_x_out[i] = delta_f[i - 4];
  memcpy(J.world_to_cam_eval_out, eval.data(), 56 * (size_t)n), memcpy(J.state_zero_out, zero.data(), 64 * (size_t)n);
  memcpy(J.state_out, state.data(), 64 * (size_t)n), memcpy(J.c_delta_out, c_delta, 16), memcpy(J.cam_out, cam, 24);
  if (J.cam_to_world_out) memcpy(J.cam_to_world_out, Cw.data(), 56 * (size_t)n);

  // Z4's job: the final linearisation at the committed state: the last pass's results are its inputs
  float *eth = scratch, *ids = scratch + n;
  for (int p = 0; p < np; p++) ids[p] = stp::point_idepth_scaled(S.idepth, T.idepth_out[p]);
  memcpy(eth, L0.frame_energy_th, 4 * (size_t)n);
  eth[f] = *J.opt.frame_energy_th_out;
  dsm_linearize_job &L = *lin;
  L = L0;
  memcpy(L.cam, cam, 16), memcpy(L.cam_inv, cam + 4, 8);
  L.pre_RTll_0 = R0, L.pre_tTll_0 = t0, L.pre_KRKiTll = M, L.pre_KtTll = Kt, L.pre_aff_mode = am, L.pre_b0_mode = b0;
  L.frame_energy_th = eth, L.idepth_scaled = ids, L.idepth_zero_scaled = ids;
  L.state_in = L0.new_state, L.energy_in = L0.new_energy, L.fix_linearization = 1;
  L.new_state = J.new_state, L.new_energy = J.new_energy, L.new_energy_with_outlier = J.new_energy_with_outlier;
  L.J_out = J.J_out, L.center_projected_to = nullptr, L.projected_to = nullptr, L.keep = J.keep, L.rel_bs = J.rel_bs;
  L.energy_out = J.energy, L.new_frame_energy_th_out = J.frame_energy_th_out;
  return DSM_OK;
}

extern "C" int dsm_diag_finish_book_host(const dsm_finish_job *job) {
  using namespace dsm;
  auto fail = [](const char *msg) {
    set_error(std::string("dsm_diag_finish_book_host: ") + msg);
    return DSM_ERR_INVALID;
  };
  if (!job) return fail("bad argument");
  if (const char *e = finish_job_error(*job)) return fail(e);
  const dsm_finish_job &J = *job;
  const dsm_linearize_job &L0 = J.opt.step.sol.hes.lin;
  const int np = L0.n_pts, nr = L0.n_res;
  if (nr && !L0.point) return fail("NULL point");
  for (int r = 0; r < nr; r++)
    if (L0.point[r] < 0 || L0.point[r] >= np) return fail("point outside [0, n_pts)");
  // Z5, Z6: per point over its residuals in ascending index
  std::vector<int> start((size_t)np + 1, 0), list((size_t)nr + 1);
  for (int r = 0; r < nr; r++) start[L0.point[r] + 1]++;
  for (int p = 0; p < np; p++) start[p + 1] += start[p];
  {
    std::vector<int> at(start.begin(), start.end() - 1);
    for (int r = 0; r < nr; r++) list[at[L0.point[r]]++] = r;
  }
  const HostRes res{J.keep, L0.is_new, J.new_state, J.rel_bs};
  for (int p = 0; p < np; p++) {
    const int ls[2] = {J.last_state_in[2 * p], J.last_state_in[2 * p + 1]};
    fin::PointBook b;
    fin::point_book(&list[start[p]], start[p + 1] - start[p], res, J.n_good_residuals_in[p], J.max_rel_baseline_in[p], J.last_res + 2 * p, ls, b);
    J.n_good_residuals_out[p] = b.n_good, J.max_rel_baseline_out[p] = b.max_rel_baseline;
    J.last_res_out[2 * p] = b.last_res[0], J.last_res_out[2 * p + 1] = b.last_res[1];
    J.last_state_out[2 * p] = b.last_state[0], J.last_state_out[2 * p + 1] = b.last_state[1];
    J.n_res_kept[p] = b.n_kept, J.point_dropped[p] = b.dropped;
  }
  // Z7
  int kept = 0, stay = 0;
  for (int r = 0; r < nr; r++) J.res_index_out[r] = J.keep[r] ? kept++ : -1;
  for (int p = 0; p < np; p++) J.point_index_out[p] = J.point_dropped[p] ? -1 : stay++;
  *J.n_res_out = kept, *J.n_pts_out = stay;
  // Z8
  *J.lost = fin::lost(*J.energy), *J.rmse = fin::rmse(*J.energy, kept);
  return DSM_OK;
}

extern "C" int dsm_window_finish_host(int w, int h, const dsm_finish_job *job, const float *const *frame_I, const dsm_linearize_params *lp,
                                      const dsm_step_params *sp, const dsm_optimize_params *op) {
  using namespace dsm;
  auto fail = [](const char *msg) {
    set_error(std::string("dsm_window_finish_host: ") + msg);
    return DSM_ERR_INVALID;
  };
  if (w < 8 || h < 8 || !job || !frame_I) return fail("bad argument");
  if (const char *e = linearize_params_error(lp)) return fail(e);
  if (const char *e = step_params_error(sp)) return fail(e);
  if (const char *e = optimize_params_error(op)) return fail(e);
  if (const char *e = optimize_job_error(job->opt)) return fail(e);
  if (const char *e = finish_job_error(*job)) return fail(e);
  if (int rc = dsm_window_optimize_host(w, h, &job->opt, frame_I, lp, sp, op)) return rc;
  const dsm_linearize_job &L0 = job->opt.step.sol.hes.lin;
  std::vector<float> scratch((size_t)L0.n_frames + (size_t)L0.n_pts + 1);
  dsm_linearize_job L;
  if (int rc = dsm_diag_finish_prepare_host(job, lp, sp, scratch.data(), &L)) return rc; // Z1-Z3
  if (int rc = dsm_linearize_residuals_host(w, h, &L, frame_I, lp)) return rc;               // Z4
  return dsm_diag_finish_book_host(job);                                                   // Z5-Z8
}
