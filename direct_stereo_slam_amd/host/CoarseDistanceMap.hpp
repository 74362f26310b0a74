// CoarseDistanceMap.hpp -- C++ host adaptor that keeps the public surface of the reference's dso::CoarseDistanceMap
// (src/scale_optimization/TrackerAndScaler.h:139-170) on top of the C ABI (include/dsm_hotpath.h), so the call sites of
// FrontEnd::activatePointsMT (FrontEnd.cpp:56, :374-375, :389-392, :439, :443) keep their shape -- and activatePoints(), the walk of
// FrontEnd.cpp:431-449 for the windows of many sequences in one call, in the style of setCoarseTrackingRefs.  Header-only, plain
// C++11; the DSO types are reduced to the fields this path reads.  Semantics: DESIGN.md section 12 (D1-D6).
#pragma once
#include <cmath>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/dsm_hotpath.h"

namespace dsm_host {

inline void distmap_check(int rc, const char *what) {
  if (rc != DSM_OK) throw std::runtime_error(std::string(what) + ": " + dsm_last_error());
}

// Eigen's Mat33f as this path uses it: row-major storage here, element access (r, c)
struct Mat33f {
  float m[9];
  Mat33f() {
    for (float &x : m) x = 0.f;
  }
  float &operator()(int r, int c) { return m[3 * r + c]; }
  float operator()(int r, int c) const { return m[3 * r + c]; }
};
// a * b with each element ((a0 b0 + a1 b1) + a2 b2) in float.  Eigen's own evaluation order of K[1] * R * Ki[0] is not pinned
// (DESIGN.md section 5): a caller that needs Eigen's bits passes its own KRKi / Kt through DistMapHost::set_krki
inline Mat33f mul(const Mat33f &a, const Mat33f &b) {
  Mat33f o;
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) o(r, c) = (a(r, 0) * b(0, c) + a(r, 1) * b(1, c)) + a(r, 2) * b(2, c);
  return o;
}

// A frame of the window other than the newest, as makeDistanceMap (:1212-1214) and activatePointsMT (FrontEnd.cpp:387-392) read it:
// fhToNew = newest->PRE_worldToCam * host->PRE_camToWorld, rotationMatrix().cast<float>() (row-major) and translation().cast<float>()
struct DistMapHost {
  Mat33f R;
  float t[3] = {0, 0, 0};
  bool have_krki = false; // set_krki: use these instead of K[1] R Ki[0] / K[1] t
  Mat33f KRKi;
  float Kt[3] = {0, 0, 0};
  void set_krki(const Mat33f &krki, const float kt[3]) {
    KRKi = krki;
    for (int i = 0; i < 3; i++) Kt[i] = kt[i];
    have_krki = true;
  }
};
// an active PointHessian of a host frame: u, v, idepth_scaled (:1218)
struct DistMapPoint {
  int host;
  float u, v, idepth;
};
// an ImmaturePoint that passed the canActivate filter (FrontEnd.cpp:400-429), in the reference's order
struct ImmatureCandidate {
  int host;
  float u, v, idepth_min, idepth_max, my_type;
};

class CoarseDistanceMap {
public:
  Mat33f K[DSM_MAX_LEVELS];
  Mat33f Ki[DSM_MAX_LEVELS];
  // host mirror of the device map, (ww >> 1) * (hh >> 1) floats, refreshed after every call that changes the map
  float *fwdWarpedIDDistFinal;

  // reference: CoarseDistanceMap(int ww, int hh) (:1174-1187)
  CoarseDistanceMap(dsm_context *ctx, int ww, int hh, int pyrLevelsUsed = 5)
      : fwdWarpedIDDistFinal(nullptr), ctx_(ctx), levels_(pyrLevelsUsed), mirror_((size_t)(ww >> 1) * (hh >> 1), 1000.0f) {
    if (pyrLevelsUsed < 2 || pyrLevelsUsed > DSM_MAX_LEVELS) throw std::invalid_argument("pyrLevelsUsed must be in [2, DSM_MAX_LEVELS]");
    distmap_check(dsm_distmap_create(ctx, ww, hh, &map_), "dsm_distmap_create");
    fwdWarpedIDDistFinal = mirror_.data();
    ww_ = ww, hh_ = hh;
    w_[0] = h_[0] = 0; // :1186
  }
  ~CoarseDistanceMap() { dsm_distmap_destroy(map_); }
  CoarseDistanceMap(const CoarseDistanceMap &) = delete;
  CoarseDistanceMap &operator=(const CoarseDistanceMap &) = delete;

  // reference: makeK(CalibHessian*) reads fxl(), fyl(), cxl(), cyl() (:1334-1362).  Ki is the closed-form inverse of the
  // upper-triangular K; Eigen's .inverse() may differ from it in the last bit.
  void makeK(float fxl, float fyl, float cxl, float cyl) {
    w_[0] = ww_, h_[0] = hh_;
    float fx[DSM_MAX_LEVELS], fy[DSM_MAX_LEVELS], cx[DSM_MAX_LEVELS], cy[DSM_MAX_LEVELS];
    fx[0] = fxl, fy[0] = fyl, cx[0] = cxl, cy[0] = cyl;
    for (int level = 1; level < levels_; ++level) {
      w_[level] = w_[0] >> level;
      h_[level] = h_[0] >> level;
      fx[level] = fx[level - 1] * 0.5;
      fy[level] = fy[level - 1] * 0.5;
      cx[level] = (cx[0] + 0.5) / ((int)1 << level) - 0.5;
      cy[level] = (cy[0] + 0.5) / ((int)1 << level) - 0.5;
    }
    for (int level = 0; level < levels_; ++level) {
      K[level] = Mat33f();
      K[level](0, 0) = fx[level], K[level](0, 2) = cx[level], K[level](1, 1) = fy[level], K[level](1, 2) = cy[level], K[level](2, 2) = 1.0f;
      Ki[level] = Mat33f();
      Ki[level](0, 0) = 1.0f / fx[level], Ki[level](0, 2) = -cx[level] / fx[level];
      Ki[level](1, 1) = 1.0f / fy[level], Ki[level](1, 2) = -cy[level] / fy[level], Ki[level](2, 2) = 1.0f;
    }
  }

  // reference: makeDistanceMap(std::vector<FrameHessian*> frameHessians, FrameHessian* frame) (:1197-1230) -- the caller flattens
  // the window: `hosts` are the frames other than `frame`, `points` their active points
  void makeDistanceMap(const std::vector<DistMapHost> &hosts, const std::vector<DistMapPoint> &points) {
    Flat f;
    dsm_activation_job job = flatten(f, hosts, points, nullptr);
    distmap_check(dsm_distmaps_make(ctx_, 1, &job), "makeDistanceMap");
    refresh();
  }

  // reference: addIntoDistFinal(int u, int v) (:1326-1332); a no-op before makeK (:1327)
  void addIntoDistFinal(int u, int v) {
    if (w_[0] == 0) return;
    distmap_check(dsm_distmap_add(map_, u, v), "addIntoDistFinal");
    refresh();
  }

  // KRKi = K[1] R Ki[0] and Kt = K[1] t of a host (:1213-1214, FrontEnd.cpp:388-392)
  void krki_of(const DistMapHost &h, float krki[9], float kt[3]) const {
    if (h.have_krki) {
      for (int i = 0; i < 9; i++) krki[i] = h.KRKi.m[i];
      for (int i = 0; i < 3; i++) kt[i] = h.Kt[i];
      return;
    }
    const Mat33f M = mul(mul(K[1], h.R), Ki[0]);
    for (int i = 0; i < 9; i++) krki[i] = M.m[i];
    for (int r = 0; r < 3; r++) kt[r] = (K[1](r, 0) * h.t[0] + K[1](r, 1) * h.t[1]) + K[1](r, 2) * h.t[2];
  }

  int w1() const { return ww_ >> 1; }
  int h1() const { return hh_ >> 1; }
  dsm_distmap *handle() { return map_; }
  void refresh() { distmap_check(dsm_distmap_get(map_, mirror_.data()), "dsm_distmap_get"); }

  // (used by activatePoints below) the window as the flat arrays of a dsm_activation_job
  struct Flat {
    std::vector<float> krki, kt, su, sv, sd, cu, cv, cd, ct;
    std::vector<int> sh, ch;
  };
  dsm_activation_job flatten(Flat &f, const std::vector<DistMapHost> &hosts, const std::vector<DistMapPoint> &points,
                             const std::vector<ImmatureCandidate> *cands) const {
    if (w_[0] == 0) throw std::logic_error("CoarseDistanceMap: makeK has not been called"); // growDistBFS asserts w_[0] != 0 (:1236)
    f.krki.resize(9 * hosts.size()), f.kt.resize(3 * hosts.size());
    for (size_t i = 0; i < hosts.size(); i++) krki_of(hosts[i], &f.krki[9 * i], &f.kt[3 * i]);
    for (const DistMapPoint &p : points) f.sh.push_back(p.host), f.su.push_back(p.u), f.sv.push_back(p.v), f.sd.push_back(p.idepth);
    if (cands)
      for (const ImmatureCandidate &c : *cands) {
        f.ch.push_back(c.host), f.cu.push_back(c.u), f.cv.push_back(c.v), f.ct.push_back(c.my_type);
        f.cd.push_back(0.5f * (c.idepth_max + c.idepth_min)); // FrontEnd.cpp:433
      }
    dsm_activation_job j;
    j.map = map_;
    j.n_hosts = (int)hosts.size(), j.krki = f.krki.data(), j.kt = f.kt.data();
    j.n_seeds = (int)points.size(), j.seed_host = f.sh.data(), j.seed_u = f.su.data(), j.seed_v = f.sv.data(), j.seed_idepth = f.sd.data();
    j.n_cand = (int)f.ch.size(), j.cand_host = f.ch.data(), j.cand_u = f.cu.data(), j.cand_v = f.cv.data(), j.cand_idepth = f.cd.data();
    j.cand_type = f.ct.data();
    j.min_act_dist = 0.f, j.decision_out = nullptr, j.n_activated_out = nullptr;
    return j;
  }

private:
  dsm_context *ctx_;
  dsm_distmap *map_ = nullptr;
  int levels_;
  int ww_, hh_;
  int w_[DSM_MAX_LEVELS], h_[DSM_MAX_LEVELS];
  std::vector<float> mirror_;
};

// One window of activatePoints: the map (makeK called), the window's frames other than the newest, their active points, the
// candidates, current_min_act_dist_.  Outputs: decisions (0 keep, 1 activate -> toOptimize, 2 out of bounds -> the reference deletes
// the point) and their count of 1s; the map and its mirror then hold the state after the last activation.
struct ActivationRequest {
  CoarseDistanceMap *map = nullptr;
  const std::vector<DistMapHost> *hosts = nullptr;
  const std::vector<DistMapPoint> *points = nullptr;
  const std::vector<ImmatureCandidate> *candidates = nullptr;
  float min_act_dist = 0.f;
  std::vector<unsigned char> decisions;
  int n_activated = 0;
};

// makeDistanceMap + the walk of FrontEnd.cpp:431-449 for many sequences in ONE call (one launch sequence, one host wait); every
// map must have the same size
inline void activatePoints(dsm_context *ctx, std::vector<ActivationRequest> &reqs) {
  if (reqs.empty()) return;
  std::vector<CoarseDistanceMap::Flat> flat(reqs.size());
  std::vector<dsm_activation_job> jobs(reqs.size());
  for (size_t i = 0; i < reqs.size(); i++) {
    ActivationRequest &r = reqs[i];
    if (!r.map || !r.hosts || !r.points || !r.candidates) throw std::invalid_argument("activatePoints: incomplete request");
    jobs[i] = r.map->flatten(flat[i], *r.hosts, *r.points, r.candidates);
    r.decisions.assign(r.candidates->size() + 1, 0);
    jobs[i].min_act_dist = r.min_act_dist, jobs[i].decision_out = r.decisions.data(), jobs[i].n_activated_out = &r.n_activated;
  }
  distmap_check(dsm_activate_points_batch(ctx, (int)jobs.size(), jobs.data()), "activatePoints");
  for (ActivationRequest &r : reqs) {
    r.decisions.resize(r.candidates->size());
    r.map->refresh();
  }
}

} // namespace dsm_host
