// WindowStep.hpp -- C++ host adaptor with the shape of one iteration of the loop of FrontEnd::optimize (dso_helpers/FrontEndOptimize.cpp:
// 382-453): backupState, then doStepFromBackup (:182-262) with setPrecalcValues (:300-323), linearizeAll, calcMEnergy and the
// solveSystem of the NEXT iteration as ONE call, for one window or for the windows of many sequences, on top of the C ABI
// (include/dsm_hotpath.h).  The adaptor holds what optimize holds across iterations: the committed state of the frames, the calibration
// and the points, state_state / state_energy of the residuals, frameEnergyTH and the step, and the precalc tables and calibration the
// call formed at the committed state (for host/WindowMarginalize.hpp).  The accept decision and the step-size
// heuristic stay the caller's.  Header-only, plain C++11.  Semantics: DESIGN.md section 19 (D1-D4, Q1-Q4, E1-E3).
//
//   WindowStep w;  ... fill w.req (no precalc, deltaF or deltaX), the poses, states, priors ...
//   r = w.iterate(ctx, zero factors, lambda); w.accept();             // linearizeAll + applyRes before the loop, and the first solve
//   loop: w.backupState(); r = w.iterate(ctx, factors, lambda * 0.25);  // the trial, and the next solve as if it were accepted
//         accepted: w.accept(), lambda *= 0.25;   rejected: w.reject(), lambda *= 100, w.iterate(ctx, zero factors, lambda), w.accept()
#pragma once
#include "WindowSolve.hpp"

namespace dsm_host {

struct StepResult {
  double energy = 0;   // linearizeAll's stats[0] at the trial state
  double energyM = 0;  // calcMEnergy at the trial state
  bool canBreak = false;
};

class WindowStep {
public:
  // what every iteration reads.  req: the solve request WITHOUT precalc, deltaF and deltaX (the call forms them; the calibration
  // fields of req.hes.lin are not read); req.hes.lin.residuals and frameEnergyTH are set from the members below on every call.
  SolveRequest req;
  std::vector<double> worldToCamEval;          // n x 7: {qx, qy, qz, qw, tx, ty, tz}
  std::vector<double> stateZero;               // n x 8
  double calibZero[4] = {0, 0, 0, 0};
  std::vector<float> exposure;                 // n
  std::vector<double> prior, priorZero;        // N each, or both empty
  // what optimize holds across iterations
  std::vector<double> state;                   // n x 8, committed
  double calib[4] = {0, 0, 0, 0};
  std::vector<float> idepth;                   // per point
  std::vector<ActiveResidualData> residuals;   // with the committed state_state / state_energy
  std::vector<float> frameEnergyTH;            // n; the newest frame's is set by every iterate, as setNewFrameEnergyTH does
  std::vector<double> frameStep;               // n x 8: fh->step
  double calibStep[4] = {0, 0, 0, 0};
  std::vector<float> idepthStep;               // per point
  // the trial of the last iterate
  std::vector<double> trialState, trialWorldToCam;
  double trialCalib[4] = {0, 0, 0, 0};
  std::vector<float> trialIdepth;
  float stepSums[6] = {0, 0, 0, 0, 0, 0};
  // what the call formed at the committed state (set by accept(), from the trial's): the FrameFramePrecalc tables and fxl, fyl, cxl,
  // cyl, fxli, fyli, as a caller of the other window calls passes them (host/WindowMarginalize.hpp reads them)
  std::vector<LinearizePrecalc> precalc;
  float cam[6] = {0, 0, 0, 0, 0, 0};

  void backupState() {
    stateBackup_ = state, idepthBackup_ = idepth;
    memcpy(calibBackup_, calib, sizeof calib);
    have_backup_ = true;
  }

  // one iteration on the device; stepfac: C, T, R, A, D
  StepResult iterate(dsm_context *ctx, const float stepfac[5], double lambda, const dsm_linearize_params *lp = nullptr, const dsm_step_params *sp = nullptr) {
    std::vector<WindowStep *> one(1, this);
    return iterateMany(ctx, one, stepfac, lambda, lp, sp)[0];
  }
  // ... for the windows of many sequences in ONE call (the same factors and lambda for all; every window of the same image size)
  static std::vector<StepResult> iterateMany(dsm_context *ctx, const std::vector<WindowStep *> &ws, const float stepfac[5], double lambda,
                                             const dsm_linearize_params *lp = nullptr, const dsm_step_params *sp = nullptr) {
    Params p(lp, sp);
    std::vector<dsm_step_job> jobs(ws.size());
    for (size_t i = 0; i < ws.size(); i++) jobs[i] = ws[i]->fill(stepfac, lambda);
    immature_check(dsm_window_step_batch(ctx, (int)jobs.size(), jobs.data(), p.lp, p.sp), "WindowStep::iterate");
    std::vector<StepResult> out;
    for (WindowStep *w : ws) out.push_back(w->finish());
    return out;
  }
  // ... and through the host form (no device): planes[i] is the level-0 intensity plane of frame_ids[i]
  StepResult iterateHost(int w, int h, const float *const *planes, const float stepfac[5], double lambda, const dsm_linearize_params *lp = nullptr,
                         const dsm_step_params *sp = nullptr) {
    Params p(lp, sp);
    dsm_step_job job = fill(stepfac, lambda);
    immature_check(dsm_window_step_host(w, h, &job, planes, p.lp, p.sp), "WindowStep::iterateHost");
    return finish();
  }

  // the trial becomes the committed state (applyRes_Reductor's copy of the residual states among it), the returned x the step
  void accept() {
    state = trialState, idepth = trialIdepth;
    memcpy(calib, trialCalib, sizeof calib);
    for (size_t r = 0; r < residuals.size(); r++)
      residuals[r].state_state = req.hes.lin.state_NewState[r], residuals[r].state_energy = req.hes.lin.state_NewEnergy[r];
    for (size_t i = 0; i < frameStep.size(); i++) frameStep[i] = -req.lastX[4 + i];
    for (int c = 0; c < 4; c++) calibStep[c] = -req.lastX[c];
    idepthStep = req.pointStep;
    const size_t n2 = pre_[5].size();
    precalc.assign(n2, LinearizePrecalc());
    for (size_t p = 0; p < n2; p++) {
      LinearizePrecalc &P = precalc[p];
      memcpy(P.PRE_RTll_0, &pre_[0][9 * p], 36), memcpy(P.PRE_tTll_0, &pre_[1][3 * p], 12), memcpy(P.PRE_KRKiTll, &pre_[2][9 * p], 36);
      memcpy(P.PRE_KtTll, &pre_[3][3 * p], 12), memcpy(P.PRE_aff_mode, &pre_[4][2 * p], 8), P.PRE_b0_mode = pre_[5][p];
    }
    memcpy(cam, trialCam_, sizeof cam);
    step_valid_ = true;
  }
  // the trial is discarded (loadSateBackup): the committed state stays and the step is void until an iterate with zero factors at
  // the raised lambda has been accepted; until then iterate refuses non-zero factors (std::logic_error), as it does before the first
  // accept
  void reject() { step_valid_ = false; }
  bool stepValid() const { return step_valid_; }

private:
  friend class WindowOptimize; // WindowOptimize.hpp: the whole loop in one call, on the same members
  friend class WindowFinish;   // WindowFinish.hpp: the loop and what follows it in one call
  struct Params {
    dsm_linearize_params l;
    dsm_step_params s;
    const dsm_linearize_params *lp;
    const dsm_step_params *sp;
    Params(const dsm_linearize_params *lp_, const dsm_step_params *sp_) {
      dsm_linearize_params_default(&l), dsm_step_params_default(&s);
      lp = lp_ ? lp_ : &l, sp = sp_ ? sp_ : &s;
    }
  };
  std::vector<double> stateBackup_;
  double calibBackup_[4] = {0, 0, 0, 0};
  std::vector<float> idepthBackup_;
  bool have_backup_ = false, step_valid_ = false;
  solve_detail::Flat flat_;
  int can_break_ = 0;
  double energy_m_ = 0;
  std::vector<float> pre_[6]; // the trial's pre_RTll_0, pre_tTll_0, pre_KRKiTll, pre_KtTll, pre_aff_mode, pre_b0_mode
  float trialCam_[6] = {0, 0, 0, 0, 0, 0};

  dsm_step_job fill(const float stepfac[5], double lambda) {
    const size_t n = req.hes.lin.frame_ids.size(), N = 4 + 8 * n, np = idepth.size();
    if (!have_backup_) backupState();
    if (!step_valid_ && (stepfac[0] != 0 || stepfac[1] != 0 || stepfac[2] != 0 || stepfac[3] != 0 || stepfac[4] != 0))
      throw std::logic_error("WindowStep: no valid step (before the first accept, or after a reject): iterate with zero factors first");
    if (worldToCamEval.size() != 7 * n || stateZero.size() != 8 * n || state.size() != 8 * n || exposure.size() != n ||
        prior.size() != priorZero.size() || (!prior.empty() && prior.size() != N) || !req.hes.lin.points || req.hes.lin.points->size() != np)
      throw std::invalid_argument("WindowStep: an array of the wrong length");
    if (frameStep.size() != 8 * n) frameStep.assign(8 * n, 0.0);
    if (idepthStep.size() != np) idepthStep.assign(np, 0.f);
    req.hes.lin.residuals = &residuals, req.hes.lin.frameEnergyTH = frameEnergyTH;
    req.hes.lin.precalc.assign(n * n, LinearizePrecalc()), req.hes.deltaF.clear(), req.deltaX.clear();
    req.lambda = lambda;
    flat_ = solve_detail::Flat();
    dsm_step_job j;
    memset(&j, 0, sizeof j);
    j.sol = solve_detail::flatten(flat_, req);
    dsm_linearize_job &L = j.sol.hes.lin; // what the call forms must be NULL
    L.pre_RTll_0 = L.pre_tTll_0 = L.pre_KRKiTll = L.pre_KtTll = L.pre_aff_mode = L.pre_b0_mode = nullptr;
    L.idepth_scaled = L.idepth_zero_scaled = nullptr;
    j.world_to_cam_eval = worldToCamEval.data(), j.state_zero = stateZero.data(), j.state_backup = stateBackup_.data(), j.frame_step = frameStep.data();
    j.calib_zero = calibZero, j.calib_backup = calibBackup_, j.calib_step = calibStep;
    j.idepth_backup = idepthBackup_.data(), j.idepth_step = idepthStep.data(), j.exposure = exposure.data();
    memcpy(j.stepfac, stepfac, sizeof j.stepfac);
    j.prior = prior.empty() ? nullptr : prior.data(), j.prior_zero = prior.empty() ? nullptr : priorZero.data();
    trialState.assign(8 * n, 0.0), trialWorldToCam.assign(7 * n, 0.0), trialIdepth.assign(np + 1, 0.f);
    j.state_out = trialState.data(), j.calib_out = trialCalib, j.idepth_out = trialIdepth.data(), j.world_to_cam_out = trialWorldToCam.data();
    j.can_break = &can_break_, j.step_sums = stepSums, j.energy_m = &energy_m_;
    const size_t width[6] = {9, 3, 9, 3, 2, 1};
    for (int k = 0; k < 6; k++) pre_[k].assign(n * n * width[k], 0.f);
    j.cam_out = trialCam_, j.pre_RTll_0_out = pre_[0].data(), j.pre_tTll_0_out = pre_[1].data(), j.pre_KRKiTll_out = pre_[2].data();
    j.pre_KtTll_out = pre_[3].data(), j.pre_aff_mode_out = pre_[4].data(), j.pre_b0_mode_out = pre_[5].data();
    return j;
  }
  StepResult finish() {
    solve_detail::unpack(flat_, req);
    trialIdepth.pop_back();
    if (!frameEnergyTH.empty()) frameEnergyTH.back() = req.hes.lin.newFrameEnergyTH;
    StepResult r;
    r.energy = req.hes.lin.energy, r.energyM = energy_m_, r.canBreak = can_break_ != 0;
    return r;
  }
};

} // namespace dsm_host
