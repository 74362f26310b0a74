// WindowMarginalize.hpp -- C++ host adaptor for what FrontEnd::makeKeyFrame does right after optimize (FrontEnd.cpp:816-839):
// flagPointsForRemoval (:504-583), EnergyFunctional::marginalizePointsF and, per flagged frame, marginalizeFrame
// (FrontEndMarginalize.cpp:148-153), as ONE call for one window or for the windows of many sequences, on top of the C ABI
// (include/dsm_hotpath.h).  Header-only, plain C++11.  Semantics: DESIGN.md section 21 (C, M1, X1, A1', M2, G1-G7, Z).
//
//   MarginalizeRequest m;  m.fromWindow(o);   // o: a WindowOptimize after optimize(): the committed state, residual states, precalc
//   ... the flags, the points' counters, margFrames and their priors ...;  marginalizeWindow(ctx, m);          -- or, by hand:
//   MarginalizeRequest m;  ... m.hes: the whole window as optimize left it (the committed residual states, the precalc tables and the
//   calibration at the committed state, adHost / adTarget, priorF, deltaF); the flags, the points' counters, HM / bM, margFrames ...
//   m.setDeltaF(state, stateZero, calib, calibZero);                  // adHTdeltaF and cDeltaF, as EnergyFunctional::setDeltaF
//   marginalizeWindow(ctx, m);                                        // or marginalizeWindows(ctx, reqs), or marginalizeWindowHost(w, h, planes, m)
//   m.verdict, m.pointsMarginalized(), m.pointsOut(): what to erase;  m.HM_out / m.bM_out: the next keyframe's SolveRequest::HM / bM
// Erasing the points, residuals and frames and renumbering what stays (dropPointsF, removePoint, makeIDX) stay the caller's.
#pragma once
#include "WindowFinish.hpp" // includes WindowOptimize.hpp

#include "../csrc/delta_math.hpp"

namespace dsm_host {

struct MarginalizeRequest {
  // hes.lin.fixLinearization and hes.lin.wantJacobians must be false; Hdd_accLF, bd_accLF, Hcd_accLF and shiftPriorToZero are not read
  HessianRequest hes;
  std::vector<unsigned char> flaggedForMarginalization; // per frame
  std::vector<int> numGoodResiduals;                    // per point
  std::vector<unsigned char> lastResiduals;             // per point 2: lastResiduals[0].second, [1].second as DSM_RES_*
  std::vector<float> idepthHessian;                     // per point, as optimize's last accumulation left it (HessianRequest::idepth_hessian)
  std::vector<float> adHTdeltaF;                        // n * n * 8, [host][target]: setDeltaF() forms it
  float cDeltaF[4] = {0, 0, 0, 0};
  std::vector<double> HM, bM;                           // N * N and N, or both empty (zeros)
  std::vector<int> margFrames;                          // strictly ascending indices into hes.lin.frame_ids, each flagged
  std::vector<double> framePrior, frameDeltaPrior;      // 8 per marginalised frame: EFFrame::prior, delta_prior
  bool wantDetails = false;                             // HM_points, bM_points, res_toZeroF

  // fromWindow()'s copies of the points (at the committed depths) and of the residuals (with the committed states), which hes.lin
  // then names
  std::vector<ActivePointData> points;
  std::vector<ActiveResidualData> residuals;
  bool ownsWindowData = false;

  // results
  std::vector<unsigned char> verdict;   // per point: 0 keep, 1 PS_MARGINALIZE, 2 PS_DROP
  std::vector<double> HM_out, bM_out;   // over the frames that stay, in order: N' = N - 8 margFrames.size()
  int resInM = 0;                       // the increment of EnergyFunctional::resInM
  std::vector<double> HM_points, bM_points; // wantDetails: the prior after marginalizePointsF, before a frame leaves
  std::vector<float> res_toZeroF;           // wantDetails: 8 per residual, of the marginalised points' active residuals

  // EnergyFunctional::setDeltaF from the committed state (c_delta and delta_f): float products and
  // sums over ascending k from 0, the host's part and the target's part added last, as section 18's R1 forms xAd
  void setDeltaF(const std::vector<double> &state, const std::vector<double> &stateZero, const double calib[4], const double calibZero[4]) {
    const size_t n = hes.lin.frame_ids.size();
    if (state.size() != 8 * n || stateZero.size() != 8 * n || hes.adHost.size() != n * n * 64 || hes.adTarget.size() != n * n * 64)
      throw std::invalid_argument("MarginalizeRequest::setDeltaF: an array of the wrong length");
    for (int c = 0; c < 4; c++) cDeltaF[c] = (float)(calib[c] - calibZero[c]);
    adHTdeltaF.assign(n * n * 8, 0.f);
    for (size_t h = 0; h < n; h++)
      for (size_t t = 0; t < n; t++) {
        if (h == t) continue;
        const double *ah = &hes.adHost[(h * n + t) * 64], *at = &hes.adTarget[(h * n + t) * 64];
        for (int c = 0; c < 8; c++)
          adHTdeltaF[(h * n + t) * 8 + c] = dsm::ad_ht_delta_entry(ah, at, &state[8 * h], &stateZero[8 * h], &state[8 * t], &stateZero[8 * t], c);
      }
  }
  // Everything a WindowOptimize holds after optimize() (or a WindowStep after accept()): the frames, the calibration and the precalc
  // tables at the committed state, frameEnergyTH, the points at the committed depths (idepth_scaled = idepth_zero_scaled =
  // SCALE_IDEPTH idepth, section 19 D3; their deltaF is 0), the residuals with their committed states, adHost / adTarget, priorF,
  // idepth_hessian of the last accumulation, HM / bM, and setDeltaF from state / stateZero / calib / calibZero.  What remains the
  // caller's: flaggedForMarginalization, numGoodResiduals, lastResiduals, margFrames, framePrior, frameDeltaPrior.
  void fromWindow(const WindowOptimize &o, float scaleIdepth = DSM_LINEARIZE_SCALE_IDEPTH) { fromWindow(o.window, scaleIdepth); }
  void fromWindow(const WindowStep &w, float scaleIdepth = DSM_LINEARIZE_SCALE_IDEPTH) {
    const HessianRequest &H = w.req.hes;
    const size_t n = H.lin.frame_ids.size();
    if (!H.lin.points || w.precalc.size() != n * n || w.idepth.size() != H.lin.points->size() || H.idepth_hessian.size() != w.idepth.size())
      throw std::logic_error("MarginalizeRequest::fromWindow: the window holds no committed pass");
    hes = HessianRequest();
    hes.lin.window = H.lin.window, hes.lin.frame_ids = H.lin.frame_ids, hes.lin.precalc = w.precalc, hes.lin.frameEnergyTH = w.frameEnergyTH;
    hes.lin.fxl = w.cam[0], hes.lin.fyl = w.cam[1], hes.lin.cxl = w.cam[2], hes.lin.cyl = w.cam[3], hes.lin.fxli = w.cam[4], hes.lin.fyli = w.cam[5];
    hes.lin.fixLinearization = false, hes.lin.wantJacobians = false;
    points = *H.lin.points, residuals = w.residuals, ownsWindowData = true;
    for (size_t i = 0; i < points.size(); i++) points[i].idepth_scaled = points[i].idepth_zero_scaled = scaleIdepth * w.idepth[i];
    hes.adHost = H.adHost, hes.adTarget = H.adTarget, hes.priorF = H.priorF;
    idepthHessian = H.idepth_hessian;
    HM = w.req.HM, bM = w.req.bM;
    setDeltaF(w.state, w.stateZero, w.calib, w.calibZero);
  }
  // Everything from a WindowFinish after finishWindow() and shrink(): the shrunken point and residual lists with
  // the final linearisation's states, the tables, the calibration and frameEnergyTH at the new evaluation point, adHost / adTarget,
  // adHTdeltaF and cDeltaF as the finish formed them (no setDeltaF here), numGoodResiduals, the last states, priorF, idepth_hessian,
  // HM / bM.  What remains the caller's: flaggedForMarginalization, margFrames, framePrior, frameDeltaPrior.
  void fromFinished(const WindowFinish &f, float scaleIdepth = DSM_LINEARIZE_SCALE_IDEPTH) {
    const WindowStep &w = f.optimizer.window;
    const HessianRequest &H = w.req.hes;
    const size_t n = H.lin.frame_ids.size(), np = f.points.size();
    if (!f.shrunk || w.precalc.size() != n * n || w.idepth.size() != np || f.idepthHessian.size() != np || f.adHTdeltaF.size() != n * n * 8)
      throw std::logic_error("MarginalizeRequest::fromFinished: the window is not finished and shrunk");
    hes = HessianRequest();
    hes.lin.window = H.lin.window, hes.lin.frame_ids = H.lin.frame_ids, hes.lin.precalc = w.precalc, hes.lin.frameEnergyTH = w.frameEnergyTH;
    hes.lin.fxl = w.cam[0], hes.lin.fyl = w.cam[1], hes.lin.cxl = w.cam[2], hes.lin.cyl = w.cam[3], hes.lin.fxli = w.cam[4], hes.lin.fyli = w.cam[5];
    hes.lin.fixLinearization = false, hes.lin.wantJacobians = false;
    points = f.points, residuals = w.residuals, ownsWindowData = true;
    for (size_t i = 0; i < np; i++) points[i].idepth_scaled = points[i].idepth_zero_scaled = scaleIdepth * w.idepth[i];
    hes.adHost = H.adHost, hes.adTarget = H.adTarget, hes.priorF = H.priorF;
    idepthHessian = f.idepthHessian;
    HM = w.req.HM, bM = w.req.bM;
    adHTdeltaF = f.adHTdeltaF;
    memcpy(cDeltaF, f.cDeltaF, sizeof cDeltaF);
    numGoodResiduals = f.numGoodResiduals, lastResiduals = f.lastResidualStates;
  }
  // the points flagPointsForRemoval moves to pointHessiansMarginalized / pointHessiansOut
  std::vector<int> pointsMarginalized() const { return pointsOf(1); }
  std::vector<int> pointsOut() const { return pointsOf(2); }

private:
  std::vector<int> pointsOf(int v) const {
    std::vector<int> out;
    for (size_t p = 0; p < verdict.size(); p++)
      if (verdict[p] == v) out.push_back((int)p);
    return out;
  }
};

namespace marginalize_detail {
inline dsm_marginalize_job flatten(linearize_detail::Flat &f, MarginalizeRequest &r) {
  if (r.hes.lin.fixLinearization || r.hes.lin.wantJacobians) throw std::invalid_argument("marginalizeWindow: fixLinearization / wantJacobians must be false");
  if (r.ownsWindowData) r.hes.lin.points = &r.points, r.hes.lin.residuals = &r.residuals; // (a copy of the request names its own)
  dsm_marginalize_job j;
  memset(&j, 0, sizeof j);
  j.hes = hessian_detail::flatten(f, r.hes);
  j.hes.lin.keep = nullptr, j.hes.lin.rel_bs = nullptr; // must be NULL here
  const size_t nf = r.hes.lin.frame_ids.size(), n = r.hes.lin.points->size(), nr = r.hes.lin.residuals->size(), N = 4 + 8 * nf, nm = r.margFrames.size();
  if (r.flaggedForMarginalization.size() != nf || r.numGoodResiduals.size() != n || r.lastResiduals.size() != 2 * n || r.idepthHessian.size() != n ||
      r.adHTdeltaF.size() != nf * nf * 8 || r.HM.size() != (r.HM.empty() ? 0 : N * N) || r.bM.size() != (r.HM.empty() ? 0 : N) || nm > nf ||
      r.framePrior.size() != 8 * nm || r.frameDeltaPrior.size() != 8 * nm)
    throw std::invalid_argument("marginalizeWindow: an array of the wrong length");
  j.flagged = r.flaggedForMarginalization.data(), j.n_good_residuals = r.numGoodResiduals.data(), j.last_state = r.lastResiduals.data();
  j.idepth_hessian = r.idepthHessian.data(), j.ad_ht_delta = r.adHTdeltaF.data(), j.c_delta = r.cDeltaF;
  j.H_M = r.HM.empty() ? nullptr : r.HM.data(), j.b_M = r.HM.empty() ? nullptr : r.bM.data();
  j.n_marg_frames = (int)nm, j.marg_frames = r.margFrames.data(), j.frame_prior = r.framePrior.data(), j.frame_delta_prior = r.frameDeltaPrior.data();
  const size_t Nn = N - 8 * nm;
  r.verdict.assign(n + 1, 0), r.HM_out.assign(Nn * Nn, 0.0), r.bM_out.assign(Nn, 0.0), r.resInM = 0;
  j.verdict = r.verdict.data(), j.H_M_out = r.HM_out.data(), j.b_M_out = r.bM_out.data(), j.n_res_marg = &r.resInM;
  r.HM_points.clear(), r.bM_points.clear(), r.res_toZeroF.clear();
  if (r.wantDetails) {
    r.HM_points.assign(N * N, 0.0), r.bM_points.assign(N, 0.0), r.res_toZeroF.assign(8 * nr + 1, 0.f);
    j.H_M_points = r.HM_points.data(), j.b_M_points = r.bM_points.data(), j.res_to_zero = r.res_toZeroF.data();
  }
  return j;
}
inline void unpack(const linearize_detail::Flat &f, MarginalizeRequest &r) {
  hessian_detail::unpack(f, r.hes);
  r.verdict.pop_back();
  if (r.wantDetails) r.res_toZeroF.pop_back();
}
struct Params {
  dsm_linearize_params l;
  dsm_marginalize_params m;
  const dsm_linearize_params *lp;
  const dsm_marginalize_params *mp;
  Params(const dsm_linearize_params *lp_, const dsm_marginalize_params *mp_) {
    dsm_linearize_params_default(&l), dsm_marginalize_params_default(&m);
    lp = lp_ ? lp_ : &l, mp = mp_ ? mp_ : &m;
  }
};
} // namespace marginalize_detail

// flagPointsForRemoval + marginalizePointsF + marginalizeFrame for the windows of many sequences in ONE call; every window must have
// the same image size.  Fills the results of every request.  Null parameters: the defaults.
inline void marginalizeWindows(dsm_context *ctx, std::vector<MarginalizeRequest *> &reqs, const dsm_linearize_params *lp = nullptr,
                               const dsm_marginalize_params *mp = nullptr) {
  if (reqs.empty()) return;
  marginalize_detail::Params p(lp, mp);
  std::vector<linearize_detail::Flat> flat(reqs.size());
  std::vector<dsm_marginalize_job> jobs(reqs.size());
  for (size_t i = 0; i < reqs.size(); i++) jobs[i] = marginalize_detail::flatten(flat[i], *reqs[i]);
  immature_check(dsm_window_marginalize_batch(ctx, (int)jobs.size(), jobs.data(), p.lp, p.mp), "marginalizeWindows");
  for (size_t i = 0; i < reqs.size(); i++) marginalize_detail::unpack(flat[i], *reqs[i]);
}

// ... for one window
inline void marginalizeWindow(dsm_context *ctx, MarginalizeRequest &req, const dsm_linearize_params *lp = nullptr, const dsm_marginalize_params *mp = nullptr) {
  std::vector<MarginalizeRequest *> one(1, &req);
  marginalizeWindows(ctx, one, lp, mp);
}

// ... and through the host form (no device): planes[i] is the level-0 intensity plane of frame_ids[i]
inline void marginalizeWindowHost(int w, int h, const float *const *planes, MarginalizeRequest &req, const dsm_linearize_params *lp = nullptr,
                                  const dsm_marginalize_params *mp = nullptr) {
  marginalize_detail::Params p(lp, mp);
  linearize_detail::Flat flat;
  dsm_marginalize_job job = marginalize_detail::flatten(flat, req);
  immature_check(dsm_window_marginalize_host(w, h, &job, planes, p.lp, p.mp), "marginalizeWindowHost");
  marginalize_detail::unpack(flat, req);
}

} // namespace dsm_host
