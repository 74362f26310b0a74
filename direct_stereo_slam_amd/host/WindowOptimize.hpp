// WindowOptimize.hpp -- C++ host adaptor with the shape of the loop of FrontEnd::optimize (dso_helpers/FrontEndOptimize.cpp:362-371,
// :382-453): linearizeAll and applyRes before the loop, then per iteration backupState, the step-size heuristic, doStepFromBackup,
// linearizeAll, the accept test, applyRes or loadSateBackup, the lambda schedule and the break -- as ONE call, for one window or for the
// windows of many sequences, every window with its own decisions, on top of the C ABI (include/dsm_hotpath.h).  Header-only, plain
// C++11.  Semantics: DESIGN.md section 20.
//
//   WindowOptimize o;  ... fill o.window as for WindowStep (req, the poses, states, priors; the current state in state, calib, idepth) ...
//   OptimizeResult r = o.optimize(ctx);             // or WindowOptimize::optimizeMany(ctx, {&a, &b}), or o.optimizeHost(w, h, planes)
//   o.window.state, .calib, .idepth, .residuals, .frameEnergyTH, .frameStep ... now hold the committed state and the next step
#pragma once
#include <string>

#include "WindowStep.hpp"

namespace dsm_host {

struct OptimizeResult {
  std::string pattern;               // 'A' / 'R' per iteration run
  int iterations = 0, passes = 0;
  std::vector<double> passEnergy;    // passes x 2: E, E_M
  std::vector<double> passLambda;    // passes
  std::vector<float> stepsize;       // per iteration
  std::vector<unsigned char> canBreak; // per iteration: the trial's
  double lastEnergy = 0, lastEnergyM = 0; // of the last committed pass
  double lambda = 0;                 // the schedule's, after the last iteration
  float frameEnergyTH = 0;           // the newest frame's, after the last pass
};

class WindowOptimize {
public:
  WindowStep window;
  int maxIterations = 6; // mnumOptIts, 0 .. DSM_OPTIMIZE_MAX_ITERATIONS

  OptimizeResult optimize(dsm_context *ctx, const dsm_optimize_params *op = nullptr, const dsm_linearize_params *lp = nullptr,
                          const dsm_step_params *sp = nullptr) {
    std::vector<WindowOptimize *> one(1, this);
    return optimizeMany(ctx, one, op, lp, sp)[0];
  }
  // ... for the windows of many sequences in ONE call (every window of the same image size; each takes its own decisions)
  static std::vector<OptimizeResult> optimizeMany(dsm_context *ctx, const std::vector<WindowOptimize *> &ws, const dsm_optimize_params *op = nullptr,
                                                  const dsm_linearize_params *lp = nullptr, const dsm_step_params *sp = nullptr) {
    WindowStep::Params p(lp, sp);
    dsm_optimize_params defaults;
    dsm_optimize_params_default(&defaults);
    std::vector<dsm_optimize_job> jobs(ws.size());
    for (size_t i = 0; i < ws.size(); i++) jobs[i] = ws[i]->fill();
    immature_check(dsm_window_optimize_batch(ctx, (int)jobs.size(), jobs.data(), p.lp, p.sp, op ? op : &defaults), "WindowOptimize::optimize");
    std::vector<OptimizeResult> out;
    for (WindowOptimize *w : ws) out.push_back(w->finish());
    return out;
  }
  // ... and through the host form (no device): planes[i] is the level-0 intensity plane of frame_ids[i]
  OptimizeResult optimizeHost(int w, int h, const float *const *planes, const dsm_optimize_params *op = nullptr, const dsm_linearize_params *lp = nullptr,
                              const dsm_step_params *sp = nullptr) {
    WindowStep::Params p(lp, sp);
    dsm_optimize_params defaults;
    dsm_optimize_params_default(&defaults);
    dsm_optimize_job job = fill();
    immature_check(dsm_window_optimize_host(w, h, &job, planes, p.lp, p.sp, op ? op : &defaults), "WindowOptimize::optimizeHost");
    return finish();
  }

private:
  friend class WindowFinish; // WindowFinish.hpp: the same job with the finish on top
  int n_iterations_ = 0, n_passes_ = 0;
  std::vector<unsigned char> pattern_, can_;
  std::vector<double> energy_, lambda_;
  std::vector<float> stepsize_;
  double last_[2] = {0, 0}, lambda_out_ = 0;
  float eth_ = 0;

  dsm_optimize_job fill() {
    const float zero[5] = {0, 0, 0, 0, 0};
    if (maxIterations < 0 || maxIterations > DSM_OPTIMIZE_MAX_ITERATIONS) throw std::invalid_argument("WindowOptimize: maxIterations outside [0, 20]");
    window.backupState();
    dsm_optimize_job j;
    memset(&j, 0, sizeof j);
    j.step = window.fill(zero, 0.0);
    j.step.frame_step = nullptr, j.step.calib_step = nullptr, j.step.idepth_step = nullptr; // the loop forms them
    j.max_iterations = maxIterations;
    const size_t its = (size_t)maxIterations, passes = 1 + 2 * its;
    pattern_.assign(its + 1, 0), can_.assign(its + 1, 0), stepsize_.assign(its + 1, 0.f), energy_.assign(2 * passes, 0.0), lambda_.assign(passes, 0.0);
    j.n_iterations = &n_iterations_, j.n_passes = &n_passes_, j.pattern = pattern_.data(), j.pass_energy = energy_.data(), j.pass_lambda = lambda_.data();
    j.iter_stepsize = stepsize_.data(), j.iter_can_break = can_.data(), j.last_energy = last_, j.lambda_out = &lambda_out_, j.frame_energy_th_out = &eth_;
    return j;
  }
  // the job's last pass describes the committed state: it becomes the window's, as WindowStep::accept() makes it
  OptimizeResult finish() {
    window.finish();
    window.accept();
    OptimizeResult r;
    r.iterations = n_iterations_, r.passes = n_passes_;
    r.pattern.assign(pattern_.begin(), pattern_.begin() + n_iterations_);
    r.passEnergy.assign(energy_.begin(), energy_.begin() + 2 * n_passes_), r.passLambda.assign(lambda_.begin(), lambda_.begin() + n_passes_);
    r.stepsize.assign(stepsize_.begin(), stepsize_.begin() + n_iterations_), r.canBreak.assign(can_.begin(), can_.begin() + n_iterations_);
    r.lastEnergy = last_[0], r.lastEnergyM = last_[1], r.lambda = lambda_out_, r.frameEnergyTH = eth_;
    return r;
  }
};

} // namespace dsm_host
