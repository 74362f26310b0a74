// WindowRescale.hpp -- C++ host adaptor with the shape of FrontEnd::optimizeScale behind its scale search (FrontEnd.cpp:1010-1061, called
// from makeKeyFrame at :806 between removeOutliers and flagPointsForRemoval): the accept / reject decision with its trapped and
// fail-count state, the active points' depths divided by the accepted scale, the newest keyframe's pose rebuilt from its tracking
// reference with the translation scaled, and setPrecalcValues -- for one window or for the windows of many sequences in ONE call, on
// top of the C ABI (include/dsm_hotpath.h).  Header-only, plain C++11.  Semantics: DESIGN.md section 25 (S0-S6).
//
//   ScaleState scale;                                  // per sequence: the reference's function statics
//   ... the scale search: all eight guesses if scale.wantGuesses(), otherwise from 1 (:991-1004) -> newScale, scaleError ...
//   WindowRescale r;  r.fromFinished(finish);          // finish: a WindowFinish after finishWindow() and shrink()
//   r.setTrackingRef(refCamToWorld, camToTrackingRef, camToWorld);   // the newest frame's shell poses
//   r.enabled = thres > 0 && keyframes > 4;  r.scaleError = ...;  r.newScale = ...;  r.thres = ...;
//   float err = r.rescaleWindow(ctx, scale);           // or WindowRescale::rescaleWindows(ctx, {&a, &b}, {&sa, &sb}), or rescaleWindowHost(scale)
//   MarginalizeRequest m;  m.fromFinished(finish);  r.applyTo(m);    // the depths, deltaF, tables, cam, adHTdeltaF and cDeltaF
//   r.applyTo(nullspace);  r.applyTo(nextKeyframe);  r.applyTo(tracker);   // tracker: scaleCoarseDepthL0 when accepted (:1032)
// A call that rejects or is disabled returns its inputs, so the applyTo chain may always run.
#pragma once
#include <stdexcept>
#include <vector>

#include "TrackerAndScaler.hpp"
#include "WindowMarginalize.hpp"
#include "WindowNullspace.hpp"

namespace dsm_host {

// scale_trapped and scale_opt_fails (FrontEnd.cpp:977-978), per sequence
struct ScaleState {
  bool trapped = false;
  int fails = 0;
  bool wantGuesses() const { return !trapped; } // :991-1004: untrapped, the search tries every guess
};

// what the call changes: its inputs and, in the same shapes, its results
struct RescaleValues {
  std::vector<float> idepth, idepthScaled, idepthZeroScaled, deltaF; // per point
  std::vector<double> worldToCamEval, state, stateZero;              // n x 7, n x 8, n x 8
  double camToTrackingRef[7], camToWorld[7];                         // the newest frame's shell poses
  std::vector<float> pre[6];                                         // pre_RTll_0, pre_tTll_0, pre_KRKiTll, pre_KtTll, pre_aff_mode, pre_b0_mode
  float cam[6], cDeltaF[4];
  std::vector<double> deltaX;                                        // N
  std::vector<float> adHTdeltaF;                                     // n * n * 8
  std::vector<double> worldToCam, camToWorldAll;                     // n x 7: PRE_worldToCam, PRE_camToWorld (the second may be empty)
  RescaleValues() {
    for (int k = 0; k < 7; k++) camToTrackingRef[k] = camToWorld[k] = k == 3 ? 1.0 : 0.0;
    for (int k = 0; k < 6; k++) cam[k] = 0.f;
    for (int k = 0; k < 4; k++) cDeltaF[k] = 0.f;
  }
  std::vector<LinearizePrecalc> precalc() const {
    std::vector<LinearizePrecalc> out(pre[5].size());
    for (size_t p = 0; p < out.size(); p++) {
      LinearizePrecalc &P = out[p];
      memcpy(P.PRE_RTll_0, &pre[0][9 * p], 36), memcpy(P.PRE_tTll_0, &pre[1][3 * p], 12), memcpy(P.PRE_KRKiTll, &pre[2][9 * p], 36);
      memcpy(P.PRE_KtTll, &pre[3][3 * p], 12), memcpy(P.PRE_aff_mode, &pre[4][2 * p], 8), P.PRE_b0_mode = pre[5][p];
    }
    return out;
  }
};

class WindowRescale {
public:
  // the caller's gate and what the scale search returned
  bool enabled = true;    // scale_opt_thres_ > 0 and more than four keyframes (:806)
  float scaleError = -1;  // -1: no guess gave a positive error
  float newScale = 1;
  float thres = 0;        // scale_opt_thres_
  // what the call reads besides `in`
  RescaleValues in;
  std::vector<float> exposure;         // n
  double refCamToWorld[7] = {0, 0, 0, 1, 0, 0, 0};
  double affG2L[2] = {0, 0};
  double calib[4] = {0, 0, 0, 0}, calibZero[4] = {0, 0, 0, 0};
  std::vector<double> adHost, adTarget; // n * n * 64 each
  // what it returns
  RescaleValues out;
  int decision = DSM_RESCALE_DISABLED;
  float scaleErrorOut = -1; // what optimizeScale returns
  float appliedScale = 1;
  bool accepted() const { return decision == DSM_RESCALE_ACCEPTED; }

  size_t frames() const { return exposure.size(); }

  // Everything of a WindowFinish after finishWindow() and shrink(): the points' depths (idepth_scaled = idepth_zero_scaled =
  // SCALE_IDEPTH idepth, deltaF 0), the frames, the calibration, adHost / adTarget, the tables, cam, cDeltaF, deltaX and adHTdeltaF at
  // the finish's evaluation point; aff_g2l from the newest frame's state (FrontEndOptimize.cpp:479).  worldToCam is the last pass's (it
  // is returned as it is when the scale is not accepted and formed anew when it is).  What remains the caller's: setTrackingRef, the
  // gate and the search's result.
  void fromFinished(const WindowFinish &f, float scaleIdepth = DSM_LINEARIZE_SCALE_IDEPTH, double scaleA = 10.0, double scaleB = 1000.0) {
    const WindowStep &w = f.optimizer.window;
    const size_t n = w.req.hes.lin.frame_ids.size(), np = f.points.size();
    if (!f.shrunk || n == 0 || w.precalc.size() != n * n || w.idepth.size() != np || f.adHTdeltaF.size() != n * n * 8 || f.deltaX.size() != 4 + 8 * n)
      throw std::logic_error("WindowRescale::fromFinished: the window is not finished and shrunk");
    in = RescaleValues();
    in.idepth = w.idepth;
    in.idepthScaled.resize(np);
    for (size_t i = 0; i < np; i++) in.idepthScaled[i] = scaleIdepth * w.idepth[i];
    in.idepthZeroScaled = in.idepthScaled, in.deltaF.assign(np, 0.f);
    in.worldToCamEval = w.worldToCamEval, in.state = w.state, in.stateZero = w.stateZero, exposure = w.exposure;
    const size_t width[6] = {9, 3, 9, 3, 2, 1};
    for (int k = 0; k < 6; k++) in.pre[k].resize(n * n * width[k]);
    for (size_t p = 0; p < n * n; p++) {
      const LinearizePrecalc &P = w.precalc[p];
      memcpy(&in.pre[0][9 * p], P.PRE_RTll_0, 36), memcpy(&in.pre[1][3 * p], P.PRE_tTll_0, 12), memcpy(&in.pre[2][9 * p], P.PRE_KRKiTll, 36);
      memcpy(&in.pre[3][3 * p], P.PRE_KtTll, 12), memcpy(&in.pre[4][2 * p], P.PRE_aff_mode, 8), in.pre[5][p] = P.PRE_b0_mode;
    }
    memcpy(in.cam, w.cam, sizeof in.cam), memcpy(in.cDeltaF, f.cDeltaF, sizeof in.cDeltaF);
    in.deltaX = f.deltaX, in.adHTdeltaF = f.adHTdeltaF;
    in.worldToCam = w.trialWorldToCam.size() == 7 * n ? w.trialWorldToCam : w.worldToCamEval;
    memcpy(calib, w.calib, sizeof calib), memcpy(calibZero, w.calibZero, sizeof calibZero);
    adHost = w.req.hes.adHost, adTarget = w.req.hes.adTarget;
    affG2L[0] = w.state[8 * (n - 1) + 6] * scaleA, affG2L[1] = w.state[8 * (n - 1) + 7] * scaleB;
  }
  // the newest frame's shell: trackingRef->camToWorld, camToTrackingRef as tracked, and its own camToWorld
  void setTrackingRef(const double refCamToWorld_[7], const double camToTrackingRef_[7], const double camToWorld_[7]) {
    memcpy(refCamToWorld, refCamToWorld_, 56), memcpy(in.camToTrackingRef, camToTrackingRef_, 56), memcpy(in.camToWorld, camToWorld_, 56);
  }

  // returns what optimizeScale returns; `scale` is read and updated
  float rescaleWindow(dsm_context *ctx, ScaleState &scale, const dsm_linearize_params *lp = nullptr, const dsm_step_params *sp = nullptr) {
    std::vector<WindowRescale *> one(1, this);
    std::vector<ScaleState *> state(1, &scale);
    rescaleWindows(ctx, one, state, lp, sp);
    return scaleErrorOut;
  }
  // ... for the windows of many sequences in ONE call, each with its own decision and state
  static void rescaleWindows(dsm_context *ctx, const std::vector<WindowRescale *> &ws, const std::vector<ScaleState *> &states,
                             const dsm_linearize_params *lp = nullptr, const dsm_step_params *sp = nullptr) {
    if (ws.size() != states.size()) throw std::invalid_argument("WindowRescale::rescaleWindows: one ScaleState per window");
    std::vector<dsm_rescale_job> jobs(ws.size());
    std::vector<Words> words(ws.size());
    for (size_t i = 0; i < ws.size(); i++) jobs[i] = ws[i]->fill(*states[i], words[i]);
    immature_check(dsm_window_rescale_batch(ctx, (int)jobs.size(), jobs.data(), lp, sp), "WindowRescale::rescaleWindow");
    for (size_t i = 0; i < ws.size(); i++) ws[i]->apply(*states[i], words[i]);
  }
  // ... and through the host form (no device)
  float rescaleWindowHost(ScaleState &scale, const dsm_linearize_params *lp = nullptr, const dsm_step_params *sp = nullptr) {
    Words words;
    dsm_rescale_job job = fill(scale, words);
    immature_check(dsm_window_rescale_host(1, &job, lp, sp), "WindowRescale::rescaleWindowHost");
    apply(scale, words);
    return scaleErrorOut;
  }

  // what dsm_window_marginalize_batch reads: the points' depths and deltaF, the tables, cam, adHTdeltaF and cDeltaF (m: after
  // fromFinished on the same finish)
  void applyTo(MarginalizeRequest &m) const {
    if (m.points.size() != out.idepthScaled.size()) throw std::invalid_argument("WindowRescale::applyTo: another point list");
    for (size_t i = 0; i < m.points.size(); i++) m.points[i].idepth_scaled = out.idepthScaled[i], m.points[i].idepth_zero_scaled = out.idepthZeroScaled[i];
    m.hes.deltaF = out.deltaF;
    m.hes.lin.precalc = out.precalc();
    m.hes.lin.fxl = out.cam[0], m.hes.lin.fyl = out.cam[1], m.hes.lin.cxl = out.cam[2], m.hes.lin.cyl = out.cam[3], m.hes.lin.fxli = out.cam[4], m.hes.lin.fyli = out.cam[5];
    m.adHTdeltaF = out.adHTdeltaF;
    memcpy(m.cDeltaF, out.cDeltaF, sizeof m.cDeltaF);
  }
  // the evaluation poses and zero states getNullspaces reads
  void applyTo(WindowNullspace &ns) const { ns.worldToCamEval = out.worldToCamEval, ns.stateZero = out.stateZero, ns.exposure = exposure; }
  // the window the next keyframe's optimisation starts from (before a frame leaves it): evaluation poses, states and depths
  void applyTo(WindowStep &nextKeyframe) const {
    nextKeyframe.worldToCamEval = out.worldToCamEval, nextKeyframe.stateZero = out.stateZero, nextKeyframe.state = out.state;
    nextKeyframe.idepth = out.idepth, nextKeyframe.precalc = out.precalc();
    memcpy(nextKeyframe.cam, out.cam, sizeof out.cam);
  }
  // scaleCoarseDepthL0(new_scale) on the tracker of the new keyframe (:1032), when accepted
  void applyTo(TrackerAndScaler &tracker) const {
    if (accepted()) tracker.scaleCoarseDepthL0(appliedScale);
  }

private:
  struct Words {
    int decision, trapped, fails;
    float scale_error, applied_scale;
  };
  dsm_rescale_job fill(const ScaleState &scale, Words &words) {
    const size_t n = frames(), n2 = n * n, N = 4 + 8 * n, np = in.idepth.size();
    const size_t width[6] = {9, 3, 9, 3, 2, 1};
    bool ok = n > 0 && in.idepthScaled.size() == np && in.idepthZeroScaled.size() == np && in.deltaF.size() == np && in.worldToCamEval.size() == 7 * n &&
              in.state.size() == 8 * n && in.stateZero.size() == 8 * n && adHost.size() == 64 * n2 && adTarget.size() == 64 * n2 && in.deltaX.size() == N &&
              in.adHTdeltaF.size() == 8 * n2 && in.worldToCam.size() == 7 * n && (in.camToWorldAll.empty() || in.camToWorldAll.size() == 7 * n);
    for (int k = 0; k < 6; k++) ok = ok && in.pre[k].size() == width[k] * n2;
    if (!ok) throw std::invalid_argument("WindowRescale: an array of the wrong length");
    out = in;
    dsm_rescale_job j;
    memset(&j, 0, sizeof j);
    j.n_frames = (int)n, j.n_pts = (int)np, j.enabled = enabled ? 1 : 0, j.scale_error = scaleError, j.new_scale = newScale, j.thres = thres;
    j.trapped = scale.trapped ? 1 : 0, j.fails = scale.fails;
    j.idepth = in.idepth.data(), j.idepth_scaled = in.idepthScaled.data(), j.idepth_zero_scaled = in.idepthZeroScaled.data(), j.delta = in.deltaF.data();
    j.world_to_cam_eval = in.worldToCamEval.data(), j.state = in.state.data(), j.state_zero = in.stateZero.data(), j.exposure = exposure.data();
    j.cam_to_tracking_ref = in.camToTrackingRef, j.ref_cam_to_world = refCamToWorld, j.cam_to_world = in.camToWorld;
    j.aff_g2l[0] = affG2L[0], j.aff_g2l[1] = affG2L[1], j.calib_value = calib, j.calib_zero = calibZero;
    j.ad_host = adHost.data(), j.ad_target = adTarget.data();
    j.pre_RTll_0 = in.pre[0].data(), j.pre_tTll_0 = in.pre[1].data(), j.pre_KRKiTll = in.pre[2].data(), j.pre_KtTll = in.pre[3].data();
    j.pre_aff_mode = in.pre[4].data(), j.pre_b0_mode = in.pre[5].data(), j.cam = in.cam, j.c_delta = in.cDeltaF, j.delta_x = in.deltaX.data();
    j.ad_ht_delta = in.adHTdeltaF.data(), j.world_to_cam = in.worldToCam.data();
    j.cam_to_world_all = in.camToWorldAll.empty() ? nullptr : in.camToWorldAll.data();
    j.idepth_out = out.idepth.data(), j.idepth_scaled_out = out.idepthScaled.data(), j.idepth_zero_scaled_out = out.idepthZeroScaled.data();
    j.delta_out = out.deltaF.data(), j.world_to_cam_eval_out = out.worldToCamEval.data(), j.state_out = out.state.data();
    j.state_zero_out = out.stateZero.data(), j.cam_to_tracking_ref_out = out.camToTrackingRef, j.cam_to_world_out = out.camToWorld;
    j.pre_RTll_0_out = out.pre[0].data(), j.pre_tTll_0_out = out.pre[1].data(), j.pre_KRKiTll_out = out.pre[2].data(), j.pre_KtTll_out = out.pre[3].data();
    j.pre_aff_mode_out = out.pre[4].data(), j.pre_b0_mode_out = out.pre[5].data(), j.cam_out = out.cam, j.c_delta_out = out.cDeltaF;
    j.delta_x_out = out.deltaX.data(), j.ad_ht_delta_out = out.adHTdeltaF.data(), j.world_to_cam_out = out.worldToCam.data();
    j.cam_to_world_out_all = in.camToWorldAll.empty() ? nullptr : out.camToWorldAll.data();
    j.decision = &words.decision, j.scale_error_out = &words.scale_error, j.trapped_out = &words.trapped, j.fails_out = &words.fails;
    j.applied_scale = &words.applied_scale;
    return j;
  }
  void apply(ScaleState &scale, const Words &words) {
    decision = words.decision, scaleErrorOut = words.scale_error, appliedScale = words.applied_scale;
    scale.trapped = words.trapped != 0, scale.fails = words.fails;
  }
};

} // namespace dsm_host
