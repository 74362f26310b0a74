// window_case_requests.hpp -- a case file (window_case.hpp) as the adaptors' requests, for the demos of this directory.  fill() sets
// what the file holds; the window, and the pointers to points and residuals where a request has them, stay with the caller.
#pragma once
#include "WindowMarginalize.hpp" // includes WindowFinish.hpp, WindowOptimize.hpp, WindowStep.hpp, WindowSolve.hpp, WindowHessian.hpp
#include "window_case.hpp"

namespace window_case {
using namespace dsm_host;

template <typename T>
std::vector<T> vec(const T *p, size_t n) { // (a null block: the file has none)
  return p ? std::vector<T>(p, p + n) : std::vector<T>();
}

inline std::vector<ActivePointData> points(const Case &c) {
  std::vector<ActivePointData> out(c.n);
  for (size_t i = 0; i < c.n; i++) {
    out[i].host = c.host[i], out[i].u = c.u[i], out[i].v = c.v[i];
    out[i].idepth_scaled = c.idepth_scaled[i], out[i].idepth_zero_scaled = c.idepth_zero_scaled[i];
    memcpy(out[i].color, c.color + 8 * i, 32), memcpy(out[i].weights, c.weights + 8 * i, 32);
  }
  return out;
}
inline std::vector<ActiveResidualData> residuals(const Case &c) {
  std::vector<ActiveResidualData> out(c.nr);
  for (size_t i = 0; i < c.nr; i++) {
    out[i].point = c.point[i], out[i].target = c.target[i], out[i].state_state = c.state_in[i];
    out[i].state_energy = c.energy_in[i], out[i].isNew = c.is_new[i] != 0;
  }
  return out;
}
inline std::vector<const float *> planes(const Case &c) { return std::vector<const float *>(c.planes, c.planes + c.nf); }
inline void put_planes(const Case &c, KeyframeWindow &window, bool reversed = false) { // (the store's order is not the window's)
  for (size_t i = 0; i < c.nf; i++) {
    const size_t k = reversed ? c.nf - 1 - i : i;
    window.put(c.frame_ids[k], c.planes[k]);
  }
}

inline void fill(LinearizeRequest &lin, const Case &c) {
  lin.frame_ids = vec(c.frame_ids, c.nf);
  lin.fixLinearization = !c.formed() && c.kind != MARGINALIZE && c.fix_linearization != 0; // optimize's loop and the marginalisation run linearizeAll(false)
  if (c.formed()) return; // the step forms the rest; its thresholds are WindowStep's
  lin.fxl = c.cam[0], lin.fyl = c.cam[1], lin.cxl = c.cam[2], lin.cyl = c.cam[3], lin.fxli = c.cam[4], lin.fyli = c.cam[5];
  lin.frameEnergyTH = vec(c.frame_energy_th, c.nf);
  lin.precalc.resize(c.nf * c.nf);
  for (size_t k = 0; k < c.nf * c.nf; k++) {
    LinearizePrecalc &P = lin.precalc[k];
    memcpy(P.PRE_RTll_0, c.pre[0] + 9 * k, 36), memcpy(P.PRE_tTll_0, c.pre[1] + 3 * k, 12), memcpy(P.PRE_KRKiTll, c.pre[2] + 9 * k, 36);
    memcpy(P.PRE_KtTll, c.pre[3] + 3 * k, 12), memcpy(P.PRE_aff_mode, c.pre[4] + 2 * k, 8), P.PRE_b0_mode = c.pre[5][k];
  }
}
inline void fill(HessianRequest &H, const Case &c) {
  fill(H.lin, c);
  H.lin.wantJacobians = false; // the rows stay on the device
  H.adHost = vec(c.ad_host, c.nf * c.nf * 64), H.adTarget = vec(c.ad_target, c.nf * c.nf * 64);
  H.priorF = vec(c.prior, c.n);
  if (!c.formed()) H.deltaF = vec(c.delta, c.n);
  if (c.kind == MARGINALIZE) return;
  H.Hdd_accLF = vec(c.hdd_lin, c.n), H.bd_accLF = vec(c.bd_lin, c.n), H.Hcd_accLF = vec(c.hcd_lin, 4 * c.n);
  H.shiftPriorToZero = c.shift_prior_to_zero != 0;
}
inline void fill(SolveRequest &S, const Case &c) {
  fill(S.hes, c);
  S.H_L = vec(c.H_L, c.N * c.N), S.b_L = vec(c.b_L, c.N), S.HM = vec(c.H_M, c.N * c.N), S.bM = vec(c.b_M, c.N);
  S.nullBasis = vec(c.null_basis, c.N * c.n_null), S.nullPinv = vec(c.null_pinv, c.N * c.n_null);
  if (!c.formed()) S.deltaX = vec(c.delta_x, c.N), S.lambda = c.lambda;
}
// the file's state_backup, calib_backup and idepth_backup are the state a loop starts from; its steps, factors and lambda are not used
inline void fill(WindowStep &w, const Case &c) {
  fill(w.req, c);
  w.residuals = residuals(c);
  w.frameEnergyTH = vec(c.frame_energy_th, c.nf);
  w.worldToCamEval = vec(c.world_to_cam_eval, 7 * c.nf), w.stateZero = vec(c.state_zero, 8 * c.nf), w.exposure = vec(c.exposure, c.nf);
  w.prior = vec(c.state_prior, c.N), w.priorZero = vec(c.state_prior_zero, c.N);
  w.state = vec(c.state_backup, 8 * c.nf), w.idepth = vec(c.idepth_backup, c.n);
  memcpy(w.calibZero, c.calib_zero, 32), memcpy(w.calib, c.calib_backup, 32);
}
inline void fill(WindowFinish &f, const Case &c) {
  fill(f.optimizer.window, c);
  f.numGoodResiduals = vec(c.n_good_residuals_in, c.n), f.maxRelBaseline = vec(c.max_rel_baseline_in, c.n);
  f.lastResiduals = vec(c.last_res, 2 * c.n), f.lastResidualStates = vec(c.last_state_in, 2 * c.n);
}
inline void fill(MarginalizeRequest &m, const Case &c) {
  fill(m.hes, c);
  m.flaggedForMarginalization = vec(c.flagged, c.nf), m.numGoodResiduals = vec(c.n_good_residuals, c.n), m.lastResiduals = vec(c.last_state, 2 * c.n);
  m.idepthHessian = vec(c.idepth_hessian, c.n), m.adHTdeltaF = vec(c.ad_ht_delta, c.nf * c.nf * 8), m.HM = vec(c.H_M, c.N * c.N), m.bM = vec(c.b_M, c.N);
  m.margFrames = vec(c.marg_frames, c.nm), m.framePrior = vec(c.frame_prior, 8 * c.nm), m.frameDeltaPrior = vec(c.frame_delta_prior, 8 * c.nm);
  memcpy(m.cDeltaF, c.c_delta, 16);
}

// pose record `which` of a nullspace file into a WindowNullspace (a template: host/WindowNullspace.hpp is the nullspace demo's alone)
template <typename Nullspace>
void fill_poses(Nullspace &ns, const Case &c, int which) {
  const Pose &p = c.poses[which];
  ns.worldToCamEval = vec(p.world_to_cam_eval, 7 * c.nf), ns.stateZero = vec(p.state_zero, 8 * c.nf), ns.exposure = vec(p.exposure, c.nf);
}

// The next keyframe's window after a marginalisation, as makeKeyFrame leaves it: frame `leaves` of `was` dropped; the points of verdict
// 0 kept, with their residuals against the frames that stay; H_L / b_L, the priors, the states and adHost / adTarget cut to those
// frames; HM_out / bM_out as the new prior.  Returns where each old frame, point and residual went (-1: gone).
struct Shrunk {
  std::vector<int> stay, kept, new_frame, new_point, new_res;
};
inline Shrunk shrink_window(const WindowStep &was, const std::vector<ActivePointData> &was_points, const MarginalizeRequest &m, int leaves,
                            KeyframeWindow *kw, WindowStep &w, std::vector<ActivePointData> &points) {
  const size_t nf = was.req.hes.lin.frame_ids.size(), N = 4 + 8 * nf;
  Shrunk s;
  s.new_frame.assign(nf, -1), s.new_point.assign(was_points.size(), -1), s.new_res.assign(was.residuals.size(), -1);
  for (size_t k = 0; k < nf; k++)
    if ((int)k != leaves) s.new_frame[k] = (int)s.stay.size(), s.stay.push_back((int)k);
  for (size_t p = 0; p < was_points.size(); p++)
    if (m.verdict[p] == 0) s.new_point[p] = (int)s.kept.size(), s.kept.push_back((int)p);
  const HessianRequest &Hw = was.req.hes;
  HessianRequest &H = w.req.hes;
  for (int p : s.kept) {
    points.push_back(was_points[p]);
    points.back().host = s.new_frame[was_points[p].host];
    w.idepth.push_back(was.idepth[p]);
    H.priorF.push_back(Hw.priorF[p]), H.Hdd_accLF.push_back(Hw.Hdd_accLF[p]), H.bd_accLF.push_back(Hw.bd_accLF[p]);
    H.Hcd_accLF.insert(H.Hcd_accLF.end(), Hw.Hcd_accLF.begin() + 4 * p, Hw.Hcd_accLF.begin() + 4 * p + 4);
  }
  for (size_t r = 0; r < was.residuals.size(); r++) { // with the states they have now
    const ActiveResidualData &q = was.residuals[r];
    if (s.new_point[q.point] < 0 || s.new_frame[q.target] < 0) continue;
    s.new_res[r] = (int)w.residuals.size();
    w.residuals.push_back(q);
    w.residuals.back().point = s.new_point[q.point], w.residuals.back().target = s.new_frame[q.target];
  }
  H.lin.window = kw, H.lin.fixLinearization = false, H.lin.wantJacobians = false;
  H.lin.frame_ids = per_frame(Hw.lin.frame_ids, s.stay, 1);
  w.frameEnergyTH = per_frame(was.frameEnergyTH, s.stay, 1);
  H.shiftPriorToZero = Hw.shiftPriorToZero;
  for (int h : s.stay)
    for (int t : s.stay) {
      const size_t at = ((size_t)h * nf + t) * 64;
      H.adHost.insert(H.adHost.end(), Hw.adHost.begin() + at, Hw.adHost.begin() + at + 64);
      H.adTarget.insert(H.adTarget.end(), Hw.adTarget.begin() + at, Hw.adTarget.begin() + at + 64);
    }
  w.req.H_L = cut(was.req.H_L, s.stay, N, true), w.req.b_L = cut(was.req.b_L, s.stay, N, false);
  w.req.HM = m.HM_out, w.req.bM = m.bM_out; // the returned prior
  w.prior = cut(was.prior, s.stay, N, false), w.priorZero = cut(was.priorZero, s.stay, N, false);
  w.worldToCamEval = per_frame(was.worldToCamEval, s.stay, 7), w.stateZero = per_frame(was.stateZero, s.stay, 8), w.exposure = per_frame(was.exposure, s.stay, 1);
  w.state = per_frame(was.state, s.stay, 8);
  memcpy(w.calib, was.calib, 32), memcpy(w.calibZero, was.calibZero, 32);
  return s;
}

} // namespace window_case
