// ImmaturePoints.hpp -- C++ host adaptor for the second half of FrontEnd::activatePointsMT (FrontEnd.cpp:458-468): the loop over
// FrontEnd::optimizeImmaturePoint (dso_helpers/FrontEndOptPoint.cpp:35-179) as ONE call for the selected points of one window or of
// the windows of many sequences, on top of the C ABI (include/dsm_hotpath.h).  Header-only, plain C++11; the DSO types are reduced
// to the fields this path reads.  Semantics: DESIGN.md section 13 (M1-M8, U1-U9).
#pragma once
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/dsm_hotpath.h"

namespace dsm_host {

inline void immature_check(int rc, const char *what) {
  if (rc != DSM_OK) throw std::runtime_error(std::string(what) + ": " + dsm_last_error());
}

// the fields of dso::ImmaturePoint that optimizeImmaturePoint and linearizeResidual read; host: index into the window's frames
struct ImmaturePointData {
  int host;
  float u, v, idepth_min, idepth_max, energyTH;
  float color[8], weights[8];
};

// FrameFramePrecalc of one [host][target] pair, cast to float: PRE_RTll (row-major), PRE_tTll, PRE_aff_mode
struct FramePrecalc {
  float PRE_RTll[9];
  float PRE_tTll[3];
  float PRE_aff_mode[2];
};

// frame_hessians_ on the device: the level-0 intensity plane of every keyframe of the window, keyed by the frame's id
class KeyframeWindow {
public:
  KeyframeWindow(dsm_context *ctx, int w, int h, int capacity = 8) : w_(w), h_(h) {
    immature_check(dsm_window_create(ctx, w, h, capacity, &win_), "dsm_window_create");
  }
  ~KeyframeWindow() { dsm_window_destroy(win_); }
  KeyframeWindow(const KeyframeWindow &) = delete;
  KeyframeWindow &operator=(const KeyframeWindow &) = delete;
  // a new keyframe from host memory: I = channel 0 of dI, w * h floats
  void put(int frame_id, const float *I) { immature_check(dsm_window_put_host(win_, frame_id, I), "dsm_window_put_host"); }
  // ... or from the tracker slot it was handed to (the frame that has just become a keyframe)
  void putFromTracker(int frame_id, dsm_tracker *owner, int slot) {
    immature_check(dsm_window_put_from_tracker(win_, frame_id, owner, slot), "dsm_window_put_from_tracker");
  }
  // marginalisation
  void drop(int frame_id) { immature_check(dsm_window_drop(win_, frame_id), "dsm_window_drop"); }
  dsm_window *handle() const { return win_; }
  int w() const { return w_; }
  int h() const { return h_; }

private:
  dsm_window *win_ = nullptr;
  int w_, h_;
};

// What :140-173 needs of one point.  status: 0 = `return 0` (the point stays immature), 1 = build the PointHessian at `idepth`
// (setIdepthZero / setIdepth, :150-151), 2 = (PointHessian*)-1 (delete the point).  in_targets: the positions in frame_hessians_ of
// the residuals with state IN, in residual order: one PointFrameResidual(p, p->host, frame_hessians_[t]) each (:154-161).
// last_residual[0] / [1]: the index into in_targets of the residual whose target is frame_hessians_.back() / the frame before it,
// or -1 (:163-172; lastResiduals then keeps {0, OOB}).
struct OptimizedPoint {
  int status = 0;
  float idepth = 0.f;
  std::vector<int> in_targets;
  int last_residual[2] = {-1, -1};
};

// One window: its frames' ids in frame_hessians_ order, the calibration (fxl, fyl, cxl, cyl, fxli, fyli of CalibHessian), the
// precalc of every [host][target] pair (n_frames * n_frames entries, the diagonal is not read) and the points selected for it.
struct ImmatureRequest {
  KeyframeWindow *window = nullptr;
  float fxl = 0, fyl = 0, cxl = 0, cyl = 0, fxli = 0, fyli = 0;
  std::vector<int> frame_ids;
  std::vector<FramePrecalc> precalc;
  const std::vector<ImmaturePointData> *points = nullptr;
  int min_obs = 1; // FrontEnd.cpp:336
  std::vector<OptimizedPoint> results;
};

namespace immature_detail {
struct Flat {
  std::vector<float> R, t, aff, u, v, dmin, dmax, eth, color, weights, idepth;
  std::vector<int> host;
  std::vector<unsigned char> status, states;
};
inline dsm_immature_job flatten(Flat &f, const ImmatureRequest &r) {
  const size_t nf = r.frame_ids.size();
  if (!r.window || !r.points || r.precalc.size() != nf * nf) throw std::invalid_argument("optimizeImmaturePoints: incomplete request");
  for (const FramePrecalc &p : r.precalc) {
    f.R.insert(f.R.end(), p.PRE_RTll, p.PRE_RTll + 9);
    f.t.insert(f.t.end(), p.PRE_tTll, p.PRE_tTll + 3);
    f.aff.insert(f.aff.end(), p.PRE_aff_mode, p.PRE_aff_mode + 2);
  }
  for (const ImmaturePointData &p : *r.points) {
    f.host.push_back(p.host), f.u.push_back(p.u), f.v.push_back(p.v), f.dmin.push_back(p.idepth_min), f.dmax.push_back(p.idepth_max);
    f.eth.push_back(p.energyTH);
    f.color.insert(f.color.end(), p.color, p.color + 8);
    f.weights.insert(f.weights.end(), p.weights, p.weights + 8);
  }
  const size_t n = r.points->size();
  f.status.assign(n + 1, 0), f.idepth.assign(n + 1, 0.f), f.states.assign(n * nf + 1, 0);
  dsm_immature_job j;
  memset(&j, 0, sizeof j);
  j.window = r.window->handle();
  j.cam[0] = r.fxl, j.cam[1] = r.fyl, j.cam[2] = r.cxl, j.cam[3] = r.cyl, j.cam_inv[0] = r.fxli, j.cam_inv[1] = r.fyli;
  j.n_frames = (int)nf, j.frame_ids = r.frame_ids.data();
  j.pre_R = f.R.data(), j.pre_t = f.t.data(), j.pre_aff = f.aff.data();
  j.n_pts = (int)n, j.host = f.host.data(), j.u = f.u.data(), j.v = f.v.data(), j.idepth_min = f.dmin.data(), j.idepth_max = f.dmax.data();
  j.energy_th = f.eth.data(), j.color = f.color.data(), j.weights = f.weights.data(), j.min_obs = r.min_obs;
  j.status = f.status.data(), j.idepth_out = f.idepth.data(), j.res_state = f.states.data();
  return j;
}
inline void unpack(const Flat &f, ImmatureRequest &r) {
  const int nf = (int)r.frame_ids.size();
  r.results.assign(r.points->size(), OptimizedPoint());
  for (size_t i = 0; i < r.results.size(); i++) {
    OptimizedPoint &o = r.results[i];
    o.status = f.status[i], o.idepth = f.idepth[i];
    if (o.status != 1) continue;
    for (int t = 0; t < nf; t++) { // residual order = frame order without the host (:38-46)
      if (f.states[i * nf + t] != DSM_RES_IN) continue;
      if (t == nf - 1) o.last_residual[0] = (int)o.in_targets.size();
      else if (t == nf - 2) o.last_residual[1] = (int)o.in_targets.size();
      o.in_targets.push_back(t);
    }
  }
}
} // namespace immature_detail

// FrontEnd.cpp:458-468 for the windows of many sequences in ONE call (one staged copy, one launch, one host wait); every window
// must have the same image size.  Fills reqs[i].results.
inline void optimizeImmaturePoints(dsm_context *ctx, std::vector<ImmatureRequest> &reqs, float huber_th = DSM_IMMATURE_HUBER_TH,
                                   float min_idepth_h_act = DSM_IMMATURE_MIN_IDEPTH_H_ACT, int gn_iterations = DSM_IMMATURE_GN_ITERATIONS) {
  if (reqs.empty()) return;
  std::vector<immature_detail::Flat> flat(reqs.size());
  std::vector<dsm_immature_job> jobs(reqs.size());
  for (size_t i = 0; i < reqs.size(); i++) jobs[i] = immature_detail::flatten(flat[i], reqs[i]);
  immature_check(dsm_optimize_immature_points_batch(ctx, (int)jobs.size(), jobs.data(), huber_th, min_idepth_h_act, gn_iterations),
                 "optimizeImmaturePoints");
  for (size_t i = 0; i < reqs.size(); i++) immature_detail::unpack(flat[i], reqs[i]);
}

// ... and for one window
inline void optimizeImmaturePoints(dsm_context *ctx, ImmatureRequest &req, float huber_th = DSM_IMMATURE_HUBER_TH,
                                   float min_idepth_h_act = DSM_IMMATURE_MIN_IDEPTH_H_ACT, int gn_iterations = DSM_IMMATURE_GN_ITERATIONS) {
  std::vector<immature_detail::Flat> flat(1);
  dsm_immature_job job = immature_detail::flatten(flat[0], req);
  immature_check(dsm_optimize_immature_points_batch(ctx, 1, &job, huber_th, min_idepth_h_act, gn_iterations), "optimizeImmaturePoints");
  immature_detail::unpack(flat[0], req);
}

} // namespace dsm_host
