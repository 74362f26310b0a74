// optimize_host.cpp -- the host form of the window optimisation's accept / reject loop (dsm_window_optimize_host)
// and the rules both forms share (V).  The host form is the loop over dsm_window_step_host, one call per pass; the decision, the lambda
// schedule and the step-size heuristic are optimize_math.hpp, shared with the device kernels (optimize_kernels.hip).  Plain C++; no
// device code.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "dsm_internal.hpp"
#include "optimize_math.hpp"

namespace dsm {

const char *optimize_params_error(const dsm_optimize_params *p) {
  if (!p) return "no optimize parameters";
  if (!std::isfinite(p->lambda_init) || !std::isfinite(p->lambda_accept_fac) || !std::isfinite(p->lambda_reject_fac) || !std::isfinite(p->fixed_lambda))
    return "an optimize parameter that is not finite";
  if (!(p->lambda_init > -1.0)) return "lambda_init <= -1";
  if (!(p->lambda_accept_fac > 0.0) || !(p->lambda_reject_fac > 0.0)) return "a lambda factor that is not positive";
  if (p->min_iterations < 0) return "a negative min_iterations";
  return nullptr;
}

const char *optimize_job_error(const dsm_optimize_job &J) {
  const dsm_linearize_job &L = J.step.sol.hes.lin;
  if (L.n_frames < 1 || L.n_frames > DSM_WINDOW_MAX_FRAMES || L.n_pts < 0 || L.n_res < 0) return "n_frames outside [1, 16] or a negative count";
  if (J.step.frame_step || J.step.calib_step || J.step.idepth_step) return "frame_step, calib_step or idepth_step given: the loop forms them";
  if (J.max_iterations < 0 || J.max_iterations > DSM_OPTIMIZE_MAX_ITERATIONS) return "max_iterations outside [0, 20]";
  if (!J.n_iterations || !J.n_passes || !J.pass_energy || !J.pass_lambda || !J.last_energy || !J.lambda_out || !J.frame_energy_th_out ||
      (J.max_iterations && (!J.pattern || !J.iter_stepsize || !J.iter_can_break)))
    return "NULL required output of the loop";
  return nullptr;
}

dsm_step_job optimize_first_pass(const dsm_optimize_job &J, const double *zeros, double lambda) {
  dsm_step_job P = J.step;
  P.frame_step = zeros, P.calib_step = zeros, P.idepth_step = reinterpret_cast<const float *>(zeros);
  for (float &f : P.stepfac) f = 0.0f;
  P.sol.lambda = lambda;
  return P;
}

} // namespace dsm

extern "C" int dsm_optimize_params_default(dsm_optimize_params *p) {
  if (!p) return DSM_ERR_INVALID;
  p->lambda_init = 0.1, p->lambda_accept_fac = 0.25, p->lambda_reject_fac = 100.0, p->fixed_lambda = -1.0;
  p->min_iterations = 1, p->force_accept = 0, p->step_momentum = 0;
  return DSM_OK;
}

extern "C" int dsm_window_optimize_host(int w, int h, const dsm_optimize_job *job, const float *const *frame_I, const dsm_linearize_params *lp,
                                        const dsm_step_params *sp, const dsm_optimize_params *op) {
  using namespace dsm;
  auto fail = [](const char *msg) {
    set_error(std::string("dsm_window_optimize_host: ") + msg);
    return DSM_ERR_INVALID;
  };
  if (w < 8 || h < 8 || !job || !frame_I) return fail("bad argument");
  if (const char *e = optimize_params_error(op)) return fail(e);
  if (const char *e = optimize_job_error(*job)) return fail(e);
  const dsm_optimize_job &J = *job;
  const dsm_linearize_job &L0 = J.step.sol.hes.lin;
  const size_t n = L0.n_frames, np = L0.n_pts, nr = L0.n_res, N = 4 + 8 * n;
  const opt::Rules R{op->lambda_accept_fac, op->lambda_reject_fac, op->fixed_lambda, op->min_iterations, op->force_accept != 0, op->step_momentum != 0};
  opt::State S;
  opt::state_init(S, op->lambda_init, J.max_iterations);

  // what the loop holds across passes
  std::vector<double> zeros(std::max(8 * n, np / 2 + 1), 0.0), backup(8 * n), fstep(8 * n, 0.0);
  double cbackup[4], cstep[4] = {0, 0, 0, 0};
  std::vector<float> idb(np + 1), ids(np + 1, 0.0f), ein(nr + 1), eth(n);
  std::vector<unsigned char> sin(nr + 1);
  dsm_step_job P = optimize_first_pass(J, zeros.data(), opt::solve_lambda(S, R));
  // pass 0's job is checked whole before anything is copied or written: the host form of the step call checks again, pass by pass
  if (const char *e = step_job_error(P)) return fail(e);
  if (!L0.frame_energy_th || (nr && (!L0.state_in || !L0.energy_in))) return fail("NULL frame_energy_th, state_in or energy_in");
  memcpy(backup.data(), J.step.state_backup, 64 * n), memcpy(cbackup, J.step.calib_backup, 32), memcpy(eth.data(), L0.frame_energy_th, 4 * n);
  if (np) memcpy(idb.data(), J.step.idepth_backup, 4 * np);
  if (nr) memcpy(sin.data(), L0.state_in, nr), memcpy(ein.data(), L0.energy_in, 4 * nr);
  dsm_linearize_job &L = P.sol.hes.lin;
  P.state_backup = backup.data(), P.frame_step = fstep.data(), P.calib_backup = cbackup, P.calib_step = cstep;
  P.idepth_backup = idb.data(), P.idepth_step = ids.data();
  L.state_in = sin.data(), L.energy_in = ein.data(), L.frame_energy_th = eth.data();
  // the outputs a pass writes for some residuals only go through a copy of the caller's array, so that what the last pass leaves
  // alone is the caller's and not an earlier pass's
  struct Partial {
    float **field;
    float *theirs;
    size_t per;
    std::vector<float> mine;
  };
  Partial partial[4] = {{&L.J_out, L0.J_out, DSM_LINEARIZE_J_FLOATS, {}},
                        {&L.center_projected_to, L0.center_projected_to, 3, {}},
                        {&L.projected_to, L0.projected_to, 16, {}},
                        {&P.sol.hes.JpJdF, J.step.sol.hes.JpJdF, 8, {}}};
  for (Partial &q : partial)
    if (q.theirs && nr) q.mine.resize(q.per * nr), *q.field = q.mine.data();

  while (S.phase != opt::DONE) {
    for (float &f : P.stepfac) f = S.cur_fac;
    P.sol.lambda = opt::solve_lambda(S, R);
    for (Partial &q : partial)
      if (!q.mine.empty()) memcpy(q.mine.data(), q.theirs, 4 * q.mine.size());
    if (int rc = dsm_window_step_host(w, h, &P, frame_I, lp, sp)) return rc;
    const float th = *L.new_frame_energy_th_out;
    opt::judge(S, R, *L.energy_out, *P.energy_m, *P.can_break, th, P.sol.x, (int)N);
    if (S.phase != opt::DONE) eth[n - 1] = th; // setNewFrameEnergyTH inside every linearizeAll
    if (S.commit) {                            // WindowStep::accept()
      memcpy(backup.data(), P.state_out, 64 * n), memcpy(cbackup, P.calib_out, 32);
      if (np) memcpy(idb.data(), P.idepth_out, 4 * np), memcpy(ids.data(), P.sol.step, 4 * np);
      for (size_t r = 0; r < nr; r++) sin[r] = L.new_state[r], ein[r] = L.new_energy[r];
      for (size_t i = 0; i < 8 * n; i++) fstep[i] = -P.sol.x[4 + i];
      for (int c = 0; c < 4; c++) cstep[c] = -P.sol.x[c];
    }
  }
  for (Partial &q : partial)
    if (!q.mine.empty()) memcpy(q.theirs, q.mine.data(), 4 * q.mine.size());

  const size_t its = J.max_iterations, passes = 1 + 2 * its;
  *J.n_iterations = S.iteration, *J.n_passes = S.n_passes;
  memcpy(J.pass_energy, S.pass_energy, 16 * passes), memcpy(J.pass_lambda, S.pass_lambda, 8 * passes);
  if (its) memcpy(J.pattern, S.pattern, its), memcpy(J.iter_stepsize, S.iter_stepsize, 4 * its), memcpy(J.iter_can_break, S.iter_can, its);
  J.last_energy[0] = S.last[0], J.last_energy[1] = S.last[1], *J.lambda_out = S.lambda, *J.frame_energy_th_out = S.eth_out;
  return DSM_OK;
}
