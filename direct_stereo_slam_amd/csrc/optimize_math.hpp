// optimize_math.hpp -- the accept / reject loop of the window optimisation as DESIGN.md section 20 states it: a job's state across
// passes, the step-size heuristic (O4), the decision with the lambda schedule and the break (O1-O3), and new_frame_energy_th from the
// order statistic (B2's float lines).  The device kernels (optimize_kernels.hip) and the host form (optimize_host.cpp) share them, so
// that both evaluate one expression tree and one state machine.  IEEE double and float, left to right as written, no contraction.
#pragma once

#include <cmath>

#include "../../include/dsm_hotpath.h"
#include "point_math.hpp"

namespace dsm {
namespace opt {

constexpr int kMaxIt = DSM_OPTIMIZE_MAX_ITERATIONS, kMaxPass = 1 + 2 * kMaxIt, kMaxN = 4 + 8 * DSM_WINDOW_MAX_FRAMES;
enum Phase { PASS0 = 0, TRIAL = 1, REPASS = 2, DONE = 3 }; // what the pass in flight is; DONE: the job is frozen

struct Rules { // dsm_optimize_params without lambda_init
  double accept_fac, reject_fac, fixed_lambda;
  int min_it, force, momentum;
};

// a job's state across passes, and its log
struct State {
  double lambda;     // the schedule's
  double cur_lambda; // the schedule's lambda of the pass in flight
  double last[2];    // E, E_M of the last committed pass
  double prev_x[kMaxN];
  double pass_energy[2 * kMaxPass], pass_lambda[kMaxPass];
  float iter_stepsize[kMaxIt];
  float stepsize, cur_fac; // cur_fac: the factor of the pass in flight
  float eth_out;
  int phase, iteration, n_passes, max_it, trial_can;
  int commit; // the pass just judged becomes the next pass's inputs
  unsigned char pattern[kMaxIt], iter_can[kMaxIt];
};

DSM_HD bool finite_d(double x) { return fabs(x) <= 1.7976931348623157e308; }

DSM_HD void state_init(State &S, double lambda_init, int max_it) {
  S.lambda = S.cur_lambda = lambda_init, S.last[0] = S.last[1] = 0.0;
  for (int i = 0; i < kMaxN; i++) S.prev_x[i] = NAN; // :384
  for (int i = 0; i < 2 * kMaxPass; i++) S.pass_energy[i] = 0.0;
  for (int i = 0; i < kMaxPass; i++) S.pass_lambda[i] = 0.0;
  for (int i = 0; i < kMaxIt; i++) S.iter_stepsize[i] = 0.0f, S.pattern[i] = 0, S.iter_can[i] = 0;
  S.stepsize = 1.0f, S.cur_fac = 0.0f, S.eth_out = 0.0f;
  S.phase = PASS0, S.iteration = 0, S.n_passes = 0, S.max_it = max_it, S.trial_can = 0, S.commit = 0;
}

// O4 (:390-405): previousX against x in double, ascending index; then the float lines as written
DSM_HD float heuristic(double *prev_x, float stepsize, const double *x, int N) {
  double dot = 0.0, pp = 0.0, xx = 0.0;
  for (int i = 0; i < N; i++) dot += prev_x[i] * x[i], pp += prev_x[i] * prev_x[i], xx += x[i] * x[i];
  const double inc = (1e-20 + dot) / (1e-20 + sqrt(pp) * sqrt(xx));
  for (int i = 0; i < N; i++) prev_x[i] = x[i];
  if (finite_d(inc)) {
    const float fresh = (float)exp(inc * 1.4);
    if (inc < 0 && stepsize > 1) stepsize = 1;
    stepsize = sqrtf(sqrtf(fresh * stepsize * stepsize * stepsize));
    if (stepsize > 2) stepsize = 2;
    if (stepsize < 0.25f) stepsize = 0.25f;
  }
  return stepsize;
}

// O1-O3: the pass in flight has returned E (B1), E_M, can_break, th (B2) and x.  Logs it, decides, advances lambda, the iteration
// and the phase.  Afterwards: phase DONE -- the job is frozen, nothing may be written to its inputs; otherwise cur_fac and cur_lambda
// are the next pass's, frame_energy_th[n - 1] takes th, and with commit the pass's results become the inputs.
DSM_HD void judge(State &S, const Rules &R, double E, double EM, int can_break, float th, const double *x, int N) {
  const int k = S.n_passes++;
  S.pass_energy[2 * k] = E, S.pass_energy[2 * k + 1] = EM, S.pass_lambda[k] = S.cur_lambda, S.eth_out = th;
  S.commit = 0;
  bool iteration_over = false;
  int can = 0;
  if (S.phase == TRIAL) {
    const int i = S.iteration;
    S.iter_can[i] = (unsigned char)(can_break != 0);
    if (!(R.force || E + EM < S.last[0] + S.last[1])) { // :427-429
      S.pattern[i] = 'R', S.trial_can = can_break;
      S.lambda = S.lambda * R.reject_fac; // :448
      S.phase = REPASS, S.cur_fac = 0.0f, S.cur_lambda = S.lambda;
      return;
    }
    S.pattern[i] = 'A', S.lambda = S.cur_lambda; // :442
    iteration_over = true, can = can_break;
  } else if (S.phase == REPASS) {
    iteration_over = true, can = S.trial_can;
  }
  S.last[0] = E, S.last[1] = EM;
  bool done = S.max_it == 0;
  if (iteration_over) {
    const int i = S.iteration++;
    done = (can && i >= R.min_it) || S.iteration >= S.max_it; // :451, :385
  }
  if (done) {
    S.phase = DONE;
    return;
  }
  S.commit = 1, S.phase = TRIAL;
  if (R.momentum) S.stepsize = heuristic(S.prev_x, S.stepsize, x, N);
  S.iter_stepsize[S.iteration] = S.stepsize;
  S.cur_fac = S.stepsize, S.cur_lambda = S.lambda * R.accept_fac;
}

// what the solve of the pass in flight gets
DSM_HD double solve_lambda(const State &S, const Rules &R) { return R.fixed_lambda >= 0.0 ? R.fixed_lambda : S.cur_lambda; }

// B2's float lines on the order statistic v
DSM_HD float energy_th(float v, float fac_median, float cw, float ow) {
  float th = sqrtf(v) * fac_median;
  th = 26.0f * cw + th * (1 - cw);
  th = th * th;
  th *= ow * ow;
  return th;
}

} // namespace opt
} // namespace dsm
