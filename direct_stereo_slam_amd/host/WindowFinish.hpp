// WindowFinish.hpp -- C++ host adaptor with the shape of the whole of FrontEnd::optimize (dso_helpers/FrontEndOptimize.cpp:332-486): the
// loop of WindowOptimize.hpp and, in the SAME call, what follows it: setEvalPT of the newest frame (:455-460), setAdjointsF, setDeltaF,
// setPrecalcValues, the final linearizeAll(true) with numGoodResiduals, maxRelBaseline and lastResiduals (:39-72, :145-176) and
// removeOutliers (:504-523) -- for one window or for the windows of many sequences, on top of the C ABI (include/dsm_hotpath.h).
// Header-only, plain C++11.  Semantics: DESIGN.md section 22 (Z1-Z8).
//
//   WindowFinish f;  ... fill f.optimizer.window as for WindowOptimize, f.points (the window's points: the adaptor owns them), and per
//   point numGoodResiduals, maxRelBaseline, lastResiduals (two residual indices, -1: none) and lastResidualStates ...
//   FinishResult r = f.finishWindow(ctx);          // or WindowFinish::finishWindows(ctx, {&a, &b}), or f.finishWindowHost(w, h, planes)
//   f.optimizer.window now stands at the new evaluation point: worldToCamEval, stateZero, state, adHost / adTarget, precalc, cam, the
//   residuals' states and frameEnergyTH are the finish's; keep, resIndex, pointDropped, pointIndex say what does not survive
//   f.shrink();                                    // erases it: the window's point and residual lists renumbered by Z7's maps
//   MarginalizeRequest m;  m.fromFinished(f);      // host/WindowMarginalize.hpp: everything the marginalisation reads, from the finish
#pragma once
#include "WindowOptimize.hpp"

namespace dsm_host {

struct FinishResult {
  OptimizeResult loop;
  double energy = 0;       // of the final linearisation
  float frameEnergyTH = 0; // the newest frame's, after it
  float rmse = 0;          // what optimize returns
  bool lost = false;
  int residuals = 0, points = 0; // that survive
};

class WindowFinish {
public:
  WindowOptimize optimizer;
  std::vector<ActivePointData> points;           // the window's points; optimizer.window.req.hes.lin.points names them on every call
  std::vector<int> numGoodResiduals;             // per point
  std::vector<float> maxRelBaseline;             // per point
  std::vector<int> lastResiduals;                // per point 2: the index of lastResiduals[0].first, [1].first among the residuals; -1: none
  std::vector<unsigned char> lastResidualStates; // per point 2: lastResiduals[0].second, [1].second as DSM_RES_*
  // what the finish formed on top of the window's members; indexed as the lists were BEFORE shrink()
  std::vector<float> adHTdeltaF;                 // n * n * 8
  float cDeltaF[4] = {0, 0, 0, 0};
  std::vector<double> deltaX;                    // N
  std::vector<float> idepthHessian;              // per point, of the loop's last accumulation (shrunk with the points)
  std::vector<unsigned char> keep;               // per residual: 1 = it survives the final linearisation
  std::vector<float> relBS;                      // per residual
  std::vector<int> resIndex;                     // per residual: its index among the kept ones, -1: removed
  std::vector<int> nResKept;                     // per point
  std::vector<unsigned char> pointDropped;       // per point: removeOutliers takes it
  std::vector<int> pointIndex;                   // per point: its index among those that stay, -1: dropped
  bool shrunk = false;

  FinishResult finishWindow(dsm_context *ctx, const dsm_optimize_params *op = nullptr, const dsm_linearize_params *lp = nullptr,
                            const dsm_step_params *sp = nullptr) {
    std::vector<WindowFinish *> one(1, this);
    return finishWindows(ctx, one, op, lp, sp)[0];
  }
  // ... for the windows of many sequences in ONE call (every window of the same image size; each takes its own decisions)
  static std::vector<FinishResult> finishWindows(dsm_context *ctx, const std::vector<WindowFinish *> &ws, const dsm_optimize_params *op = nullptr,
                                                 const dsm_linearize_params *lp = nullptr, const dsm_step_params *sp = nullptr) {
    WindowStep::Params p(lp, sp);
    dsm_optimize_params defaults;
    dsm_optimize_params_default(&defaults);
    std::vector<dsm_finish_job> jobs(ws.size());
    for (size_t i = 0; i < ws.size(); i++) jobs[i] = ws[i]->fill();
    immature_check(dsm_window_finish_batch(ctx, (int)jobs.size(), jobs.data(), p.lp, p.sp, op ? op : &defaults), "WindowFinish::finishWindow");
    std::vector<FinishResult> out;
    for (WindowFinish *w : ws) out.push_back(w->apply());
    return out;
  }
  // ... and through the host form (no device): planes[i] is the level-0 intensity plane of frame_ids[i]
  FinishResult finishWindowHost(int w, int h, const float *const *planes, const dsm_optimize_params *op = nullptr, const dsm_linearize_params *lp = nullptr,
                                const dsm_step_params *sp = nullptr) {
    WindowStep::Params p(lp, sp);
    dsm_optimize_params defaults;
    dsm_optimize_params_default(&defaults);
    dsm_finish_job job = fill();
    immature_check(dsm_window_finish_host(w, h, &job, planes, p.lp, p.sp, op ? op : &defaults), "WindowFinish::finishWindowHost");
    return apply();
  }

  // Z7's maps applied: the removed residuals and the dropped points leave the window's lists, what stays is renumbered (the residuals'
  // point, lastResiduals), and everything the window holds per point follows
  void shrink() {
    if (shrunk) return;
    WindowStep &w = optimizer.window;
    HessianRequest &H = w.req.hes;
    const size_t np = points.size(), nr = w.residuals.size();
    if (keep.size() != nr || resIndex.size() != nr || pointDropped.size() != np || pointIndex.size() != np)
      throw std::logic_error("WindowFinish::shrink: no finished call on these lists");
    std::vector<ActiveResidualData> res;
    for (size_t r = 0; r < nr; r++)
      if (keep[r]) {
        res.push_back(w.residuals[r]);
        res.back().point = pointIndex[w.residuals[r].point];
      }
    w.residuals.swap(res);
    for (size_t i = 0; i < lastResiduals.size(); i++)
      if (lastResiduals[i] >= 0) lastResiduals[i] = resIndex[lastResiduals[i]];
    std::vector<bool> stay(np);
    for (size_t p = 0; p < np; p++) stay[p] = !pointDropped[p];
    take(points, stay, 1), take(w.idepth, stay, 1), take(w.idepthStep, stay, 1), take(idepthHessian, stay, 1);
    take(H.priorF, stay, 1), take(H.Hdd_accLF, stay, 1), take(H.bd_accLF, stay, 1), take(H.Hcd_accLF, stay, 4);
    take(numGoodResiduals, stay, 1), take(maxRelBaseline, stay, 1), take(lastResiduals, stay, 2), take(lastResidualStates, stay, 2);
    shrunk = true;
  }

private:
  // an array of `width` entries per point (or empty) cut to the points that stay
  template <typename T>
  static void take(std::vector<T> &v, const std::vector<bool> &stay, size_t width) {
    if (v.size() != width * stay.size()) return;
    std::vector<T> out;
    for (size_t p = 0; p < stay.size(); p++)
      if (stay[p]) out.insert(out.end(), v.begin() + p * width, v.begin() + (p + 1) * width);
    v.swap(out);
  }

  std::vector<double> eval_, zero_, state_, adh_, adt_;
  std::vector<float> pre_[6], newEnergy_, newEnergyWithOutlier_, mrbOut_;
  std::vector<unsigned char> newState_, lastStateOut_;
  std::vector<int> ngoodOut_, lastResOut_;
  float cam_[6] = {0, 0, 0, 0, 0, 0}, th_ = 0, rmse_ = 0;
  double energy_ = 0;
  int n_res_ = 0, n_pts_ = 0, lost_ = 0;

  dsm_finish_job fill() {
    WindowStep &w = optimizer.window;
    w.req.hes.lin.points = &points;
    dsm_finish_job j;
    memset(&j, 0, sizeof j);
    j.opt = optimizer.fill();
    const size_t n = w.req.hes.lin.frame_ids.size(), N = 4 + 8 * n, np = points.size(), nr = w.residuals.size(), n2 = n * n;
    if (numGoodResiduals.size() != np || maxRelBaseline.size() != np || lastResiduals.size() != 2 * np || lastResidualStates.size() != 2 * np)
      throw std::invalid_argument("WindowFinish: a per-point array of the wrong length");
    j.n_good_residuals_in = numGoodResiduals.data(), j.max_rel_baseline_in = maxRelBaseline.data(), j.last_res = lastResiduals.data();
    j.last_state_in = lastResidualStates.data();
    eval_.assign(7 * n, 0.0), zero_.assign(8 * n, 0.0), state_.assign(8 * n, 0.0), adh_.assign(64 * n2, 0.0), adt_.assign(64 * n2, 0.0);
    adHTdeltaF.assign(8 * n2, 0.f), deltaX.assign(N, 0.0);
    const size_t width[6] = {9, 3, 9, 3, 2, 1};
    for (int k = 0; k < 6; k++) pre_[k].assign(n2 * width[k], 0.f);
    newState_.assign(nr + 1, 0), newEnergy_.assign(nr + 1, 0.f), newEnergyWithOutlier_.assign(nr + 1, 0.f), keep.assign(nr + 1, 0), relBS.assign(nr + 1, 0.f);
    resIndex.assign(nr + 1, -1), ngoodOut_.assign(np + 1, 0), mrbOut_.assign(np + 1, 0.f), lastResOut_.assign(2 * np + 1, -1), lastStateOut_.assign(2 * np + 1, 0);
    nResKept.assign(np + 1, 0), pointDropped.assign(np + 1, 0), pointIndex.assign(np + 1, -1);
    j.world_to_cam_eval_out = eval_.data(), j.state_zero_out = zero_.data(), j.state_out = state_.data(), j.ad_host_out = adh_.data();
    j.ad_target_out = adt_.data(), j.ad_ht_delta_out = adHTdeltaF.data(), j.c_delta_out = cDeltaF, j.delta_x_out = deltaX.data();
    j.pre_RTll_0_out = pre_[0].data(), j.pre_tTll_0_out = pre_[1].data(), j.pre_KRKiTll_out = pre_[2].data(), j.pre_KtTll_out = pre_[3].data();
    j.pre_aff_mode_out = pre_[4].data(), j.pre_b0_mode_out = pre_[5].data(), j.cam_out = cam_;
    j.new_state = newState_.data(), j.new_energy = newEnergy_.data(), j.new_energy_with_outlier = newEnergyWithOutlier_.data();
    j.keep = keep.data(), j.rel_bs = relBS.data(), j.energy = &energy_, j.frame_energy_th_out = &th_;
    j.n_good_residuals_out = ngoodOut_.data(), j.max_rel_baseline_out = mrbOut_.data(), j.last_res_out = lastResOut_.data();
    j.last_state_out = lastStateOut_.data(), j.n_res_kept = nResKept.data(), j.point_dropped = pointDropped.data();
    j.res_index_out = resIndex.data(), j.point_index_out = pointIndex.data(), j.n_res_out = &n_res_, j.n_pts_out = &n_pts_;
    j.rmse = &rmse_, j.lost = &lost_;
    shrunk = false;
    return j;
  }
  // the loop's last pass becomes the window's committed state (WindowOptimize), then the finish's results on top of it
  FinishResult apply() {
    FinishResult r;
    r.loop = optimizer.finish();
    WindowStep &w = optimizer.window;
    const size_t np = points.size(), nr = w.residuals.size();
    w.worldToCamEval = eval_, w.stateZero = zero_, w.state = state_;
    w.req.hes.adHost = adh_, w.req.hes.adTarget = adt_;
    const size_t n2 = pre_[5].size();
    w.precalc.assign(n2, LinearizePrecalc());
    for (size_t p = 0; p < n2; p++) {
      LinearizePrecalc &P = w.precalc[p];
      memcpy(P.PRE_RTll_0, &pre_[0][9 * p], 36), memcpy(P.PRE_tTll_0, &pre_[1][3 * p], 12), memcpy(P.PRE_KRKiTll, &pre_[2][9 * p], 36);
      memcpy(P.PRE_KtTll, &pre_[3][3 * p], 12), memcpy(P.PRE_aff_mode, &pre_[4][2 * p], 8), P.PRE_b0_mode = pre_[5][p];
    }
    memcpy(w.cam, cam_, sizeof cam_);
    for (size_t i = 0; i < nr; i++) w.residuals[i].state_state = newState_[i], w.residuals[i].state_energy = newEnergy_[i]; // applyRes
    if (!w.frameEnergyTH.empty()) w.frameEnergyTH.back() = th_;
    keep.resize(nr), relBS.resize(nr), resIndex.resize(nr), nResKept.resize(np), pointDropped.resize(np), pointIndex.resize(np);
    numGoodResiduals.assign(ngoodOut_.begin(), ngoodOut_.begin() + np), maxRelBaseline.assign(mrbOut_.begin(), mrbOut_.begin() + np);
    lastResiduals.assign(lastResOut_.begin(), lastResOut_.begin() + 2 * np);
    lastResidualStates.assign(lastStateOut_.begin(), lastStateOut_.begin() + 2 * np);
    idepthHessian = w.req.hes.idepth_hessian;
    r.energy = energy_, r.frameEnergyTH = th_, r.rmse = rmse_, r.lost = lost_ != 0, r.residuals = n_res_, r.points = n_pts_;
    return r;
  }
};

} // namespace dsm_host
