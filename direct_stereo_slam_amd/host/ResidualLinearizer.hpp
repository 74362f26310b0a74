// ResidualLinearizer.hpp -- C++ host adaptor for FrontEnd::linearizeAll (dso_helpers/FrontEndOptimize.cpp:121-179): the loop over
// PointFrameResidual::linearize with the energy sum, setNewFrameEnergyTH and the fixLinearization verdicts around it, as ONE call for the
// active residuals of one window or of the windows of many sequences, on top of the C ABI (include/dsm_hotpath.h).  Header-only, plain
// C++11; the DSO types are reduced to the fields this path reads.  Semantics: DESIGN.md section 16 (L1-L8, B1-B4).
// The call is stateless: the caller keeps state_state / state_energy, applies applyRes with what comes back (applyRes_Reductor) and
// decides whether the step is accepted.
#pragma once
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "ImmaturePoints.hpp" // KeyframeWindow

namespace dsm_host {

// the fields of dso::PointHessian that linearize reads; host: index into the window's frames
struct ActivePointData {
  int host;
  float u, v, idepth_scaled, idepth_zero_scaled;
  float color[8], weights[8];
};

// a dso::PointFrameResidual: its point (index into the request's points), its target (index into the window's frames) and its
// committed state
struct ActiveResidualData {
  int point, target;
  int state_state; // DSM_RES_IN / _OOB / _OUTLIER
  float state_energy;
  bool isNew;
};

// FrameFramePrecalc of one [host][target] pair, cast to float (3 x 3 row-major)
struct LinearizePrecalc {
  float PRE_RTll_0[9], PRE_tTll_0[3];
  float PRE_KRKiTll[9], PRE_KtTll[3];
  float PRE_aff_mode[2], PRE_b0_mode;
};

// dso::RawResidualJacobian, 74 floats in field order; the 2 x 2 blocks row-major (00, 01, 10, 11)
struct RawResidualJacobian {
  float resF[8];
  float Jpdxi[2][6];
  float Jpdc[2][4];
  float Jpdd[2];
  float JIdx[2][8];
  float JabF[2][8];
  float JIdx2[4], JabJIdx[4], Jab2[4];
};
static_assert(sizeof(RawResidualJacobian) == sizeof(float) * DSM_LINEARIZE_J_FLOATS, "RawResidualJacobian is one row of J_out");

// One window: its frames' ids in frame_hessians_ order, the calibration, the precalc of every [host][target] pair (n_frames *
// n_frames entries, the diagonal is not read), frameEnergyTH of every frame, the points and their active residuals in the order
// linearizeAll walks them.
struct LinearizeRequest {
  KeyframeWindow *window = nullptr;
  float fxl = 0, fyl = 0, cxl = 0, cyl = 0, fxli = 0, fyli = 0;
  std::vector<int> frame_ids;
  std::vector<LinearizePrecalc> precalc;
  std::vector<float> frameEnergyTH;
  const std::vector<ActivePointData> *points = nullptr;
  const std::vector<ActiveResidualData> *residuals = nullptr;
  bool fixLinearization = false;
  bool wantJacobians = true; // J, centerProjectedTo, projectedTo: what applyRes copies when the step is accepted

  // results, per residual: state_NewState, state_NewEnergy (the value linearize returned), state_NewEnergyWithOutlier; J,
  // centerProjectedTo (3 floats) and projectedTo (8 x 2 floats) of a residual whose new state is OOB are left as they were
  std::vector<unsigned char> state_NewState;
  std::vector<float> state_NewEnergy, state_NewEnergyWithOutlier;
  std::vector<RawResidualJacobian> J;
  std::vector<float> centerProjectedTo, projectedTo;
  double energy = 0;          // stats[0]: the sum of the returned values
  float newFrameEnergyTH = 0; // setNewFrameEnergyTH: the next frameEnergyTH of frame_hessians_.back()
  // with fixLinearization: the residuals that stay active / go to toRemove, and per point the updates of :55-66
  // (p->maxRelBaseline = max(p->maxRelBaseline, maxRelBaseline[p]), p->numGoodResiduals += numGoodResiduals[p])
  std::vector<int> kept, toRemove;
  std::vector<float> maxRelBaseline;
  std::vector<int> numGoodResiduals;
};

namespace linearize_detail {
struct Flat {
  std::vector<float> R0, t0, M, Kt, aff, b0, u, v, id, idz, color, weights, ein, rel;
  std::vector<int> host, point, target;
  std::vector<unsigned char> sin, isnew, keep;
};
inline dsm_linearize_job flatten(Flat &f, LinearizeRequest &r) {
  const size_t nf = r.frame_ids.size();
  if (!r.window || !r.points || !r.residuals || r.precalc.size() != nf * nf || r.frameEnergyTH.size() != nf)
    throw std::invalid_argument("linearizeAll: incomplete request");
  for (const LinearizePrecalc &p : r.precalc) {
    f.R0.insert(f.R0.end(), p.PRE_RTll_0, p.PRE_RTll_0 + 9), f.t0.insert(f.t0.end(), p.PRE_tTll_0, p.PRE_tTll_0 + 3);
    f.M.insert(f.M.end(), p.PRE_KRKiTll, p.PRE_KRKiTll + 9), f.Kt.insert(f.Kt.end(), p.PRE_KtTll, p.PRE_KtTll + 3);
    f.aff.insert(f.aff.end(), p.PRE_aff_mode, p.PRE_aff_mode + 2), f.b0.push_back(p.PRE_b0_mode);
  }
  for (const ActivePointData &p : *r.points) {
    f.host.push_back(p.host), f.u.push_back(p.u), f.v.push_back(p.v), f.id.push_back(p.idepth_scaled), f.idz.push_back(p.idepth_zero_scaled);
    f.color.insert(f.color.end(), p.color, p.color + 8);
    f.weights.insert(f.weights.end(), p.weights, p.weights + 8);
  }
  for (const ActiveResidualData &q : *r.residuals) {
    f.point.push_back(q.point), f.target.push_back(q.target), f.sin.push_back((unsigned char)q.state_state);
    f.ein.push_back(q.state_energy), f.isnew.push_back(q.isNew ? 1 : 0);
  }
  const size_t n = r.residuals->size();
  r.state_NewState.assign(n, 0), r.state_NewEnergy.assign(n, 0.f), r.state_NewEnergyWithOutlier.assign(n, 0.f);
  f.keep.assign(n + 1, 0), f.rel.assign(n + 1, 0.f);
  if (r.wantJacobians) r.J.resize(n), r.centerProjectedTo.resize(3 * n), r.projectedTo.resize(16 * n);
  dsm_linearize_job j;
  memset(&j, 0, sizeof j);
  j.window = r.window->handle();
  j.cam[0] = r.fxl, j.cam[1] = r.fyl, j.cam[2] = r.cxl, j.cam[3] = r.cyl, j.cam_inv[0] = r.fxli, j.cam_inv[1] = r.fyli;
  j.n_frames = (int)nf, j.frame_ids = r.frame_ids.data();
  j.pre_RTll_0 = f.R0.data(), j.pre_tTll_0 = f.t0.data(), j.pre_KRKiTll = f.M.data(), j.pre_KtTll = f.Kt.data();
  j.pre_aff_mode = f.aff.data(), j.pre_b0_mode = f.b0.data(), j.frame_energy_th = r.frameEnergyTH.data();
  j.n_pts = (int)r.points->size(), j.host = f.host.data(), j.u = f.u.data(), j.v = f.v.data();
  j.idepth_scaled = f.id.data(), j.idepth_zero_scaled = f.idz.data(), j.color = f.color.data(), j.weights = f.weights.data();
  j.n_res = (int)n, j.point = f.point.data(), j.target = f.target.data(), j.state_in = f.sin.data(), j.energy_in = f.ein.data();
  j.is_new = f.isnew.data(), j.fix_linearization = r.fixLinearization ? 1 : 0;
  j.new_state = r.state_NewState.data(), j.new_energy = r.state_NewEnergy.data(), j.new_energy_with_outlier = r.state_NewEnergyWithOutlier.data();
  if (r.wantJacobians && n) {
    j.J_out = reinterpret_cast<float *>(r.J.data());
    j.center_projected_to = r.centerProjectedTo.data(), j.projected_to = r.projectedTo.data();
  }
  j.keep = f.keep.data(), j.rel_bs = f.rel.data();
  j.energy_out = &r.energy, j.new_frame_energy_th_out = &r.newFrameEnergyTH;
  return j;
}
inline void unpack(const Flat &f, LinearizeRequest &r) {
  r.kept.clear(), r.toRemove.clear();
  r.maxRelBaseline.assign(r.points->size(), 0.f), r.numGoodResiduals.assign(r.points->size(), 0);
  if (!r.fixLinearization) return;
  for (size_t i = 0; i < r.residuals->size(); i++) { // :46-70
    if (!f.keep[i]) {
      r.toRemove.push_back((int)i);
      continue;
    }
    r.kept.push_back((int)i);
    const ActiveResidualData &q = (*r.residuals)[i];
    if (!q.isNew) continue;
    if (f.rel[i] > r.maxRelBaseline[q.point]) r.maxRelBaseline[q.point] = f.rel[i];
    r.numGoodResiduals[q.point]++;
  }
}
} // namespace linearize_detail

// linearizeAll for the windows of many sequences in ONE call (one staged copy, one launch, one host wait); every window must have
// the same image size.  Fills the results of every request.  params: null = the upstream defaults.
inline void linearizeAll(dsm_context *ctx, std::vector<LinearizeRequest> &reqs, const dsm_linearize_params *params = nullptr) {
  if (reqs.empty()) return;
  dsm_linearize_params defaults;
  dsm_linearize_params_default(&defaults);
  std::vector<linearize_detail::Flat> flat(reqs.size());
  std::vector<dsm_linearize_job> jobs(reqs.size());
  for (size_t i = 0; i < reqs.size(); i++) jobs[i] = linearize_detail::flatten(flat[i], reqs[i]);
  immature_check(dsm_linearize_residuals_batch(ctx, (int)jobs.size(), jobs.data(), params ? params : &defaults), "linearizeAll");
  for (size_t i = 0; i < reqs.size(); i++) linearize_detail::unpack(flat[i], reqs[i]);
}

// ... and for one window
inline void linearizeAll(dsm_context *ctx, LinearizeRequest &req, const dsm_linearize_params *params = nullptr) {
  dsm_linearize_params defaults;
  dsm_linearize_params_default(&defaults);
  linearize_detail::Flat flat;
  dsm_linearize_job job = linearize_detail::flatten(flat, req);
  immature_check(dsm_linearize_residuals_batch(ctx, 1, &job, params ? params : &defaults), "linearizeAll");
  linearize_detail::unpack(flat, req);
}

} // namespace dsm_host
