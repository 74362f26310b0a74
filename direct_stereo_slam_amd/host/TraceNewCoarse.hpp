// TraceNewCoarse.hpp -- C++ host adaptor for the loop of FrontEnd::traceNewCoarse (FrontEnd.cpp:276-327): ImmaturePoint::traceOn for
// every immature point of every frame of the window against the frame just tracked, as ONE call for one sequence or for many, on top
// of the C ABI (include/dsm_hotpath.h).  Header-only, plain C++11; the DSO types are reduced to the fields this path reads and
// writes.  Semantics: DESIGN.md section 14 (T1-T16).
#pragma once
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "ImmaturePoints.hpp"

namespace dsm_host {

// ImmaturePointData and the further fields of dso::ImmaturePoint that traceOn reads (gradH) and writes back
struct TracedPointData : ImmaturePointData {
  float gradH[4];                 // row-major
  float quality;                  // 10000 at creation
  int lastTraceStatus;            // DSM_IPS_*; IPS_UNINITIALIZED at creation
  float lastTraceUV[2];
  float lastTracePixelInterval;
};

// one host frame against the new frame (:290-297): K R K^-1 and K t of host-to-new, fromToVecExposure(host, new) cast to float
struct HostToNew {
  float KRKi[9]; // row-major
  float Kt[3];
  float aff[2];
};

// One sequence: where its new frame lies on the device (a tracker slot, :717 / :730, or a frame of a KeyframeWindow), its hosts
// (frame_hessians_ in order) and its immature points (host: index into `hosts`), which the call updates in place.
struct TraceRequest {
  dsm_tracker *tracker = nullptr;
  int slot = 0;
  KeyframeWindow *window = nullptr;
  int frame_id = 0;
  std::vector<HostToNew> hosts;
  std::vector<TracedPointData> *points = nullptr;
  int counts[6] = {0, 0, 0, 0, 0, 0}; // trace_good, trace_oob, trace_out, trace_skip, trace_badcondition, trace_uninitialized (:302-313)
  std::vector<int> steps;             // numSteps searched per point
};

namespace trace_detail {
struct Flat {
  std::vector<float> krki, kt, aff, u, v, eth, gradH, color, weights, dmin, dmax, quality, uv, interval;
  std::vector<int> host, steps;
  std::vector<unsigned char> status;
  int counts[6];
};
inline dsm_trace_job flatten(Flat &f, TraceRequest &r) {
  if (!r.points || ((r.tracker != nullptr) == (r.window != nullptr))) throw std::invalid_argument("traceNewCoarse: incomplete request");
  for (const HostToNew &h : r.hosts) {
    f.krki.insert(f.krki.end(), h.KRKi, h.KRKi + 9);
    f.kt.insert(f.kt.end(), h.Kt, h.Kt + 3);
    f.aff.insert(f.aff.end(), h.aff, h.aff + 2);
  }
  for (const TracedPointData &p : *r.points) {
    f.host.push_back(p.host), f.u.push_back(p.u), f.v.push_back(p.v), f.eth.push_back(p.energyTH);
    f.gradH.insert(f.gradH.end(), p.gradH, p.gradH + 4);
    f.color.insert(f.color.end(), p.color, p.color + 8);
    f.weights.insert(f.weights.end(), p.weights, p.weights + 8);
    f.status.push_back((unsigned char)p.lastTraceStatus);
    f.dmin.push_back(p.idepth_min), f.dmax.push_back(p.idepth_max), f.quality.push_back(p.quality);
    f.uv.push_back(p.lastTraceUV[0]), f.uv.push_back(p.lastTraceUV[1]), f.interval.push_back(p.lastTracePixelInterval);
  }
  const size_t n = r.points->size();
  f.steps.assign(n + 1, 0);
  dsm_trace_job j;
  memset(&j, 0, sizeof j);
  j.target_tracker = r.tracker, j.target_slot = r.slot;
  j.target_window = r.window ? r.window->handle() : nullptr, j.target_frame_id = r.frame_id;
  j.n_hosts = (int)r.hosts.size(), j.krki = f.krki.data(), j.kt = f.kt.data(), j.aff = f.aff.data();
  j.n_pts = (int)n, j.host = f.host.data(), j.u = f.u.data(), j.v = f.v.data(), j.energy_th = f.eth.data(), j.grad_h = f.gradH.data();
  j.color = f.color.data(), j.weights = f.weights.data();
  j.status = f.status.data(), j.idepth_min = f.dmin.data(), j.idepth_max = f.dmax.data(), j.quality = f.quality.data();
  j.trace_uv = f.uv.data(), j.trace_interval = f.interval.data(), j.steps_out = f.steps.data(), j.counts_out = f.counts;
  return j;
}
inline void unpack(const Flat &f, TraceRequest &r) {
  for (size_t i = 0; i < r.points->size(); i++) {
    TracedPointData &p = (*r.points)[i];
    p.lastTraceStatus = f.status[i], p.idepth_min = f.dmin[i], p.idepth_max = f.dmax[i], p.quality = f.quality[i];
    p.lastTraceUV[0] = f.uv[2 * i], p.lastTraceUV[1] = f.uv[2 * i + 1], p.lastTracePixelInterval = f.interval[i];
  }
  memcpy(r.counts, f.counts, sizeof r.counts);
  r.steps.assign(f.steps.begin(), f.steps.begin() + r.points->size());
}
} // namespace trace_detail

inline dsm_trace_params traceDefaults() {
  dsm_trace_params p;
  immature_check(dsm_trace_params_default(&p), "dsm_trace_params_default");
  return p;
}

// FrontEnd.cpp:276-327 for many sequences in ONE call (one staged copy, one launch, one host wait); every new frame must have the same
// size.  Writes the traced fields back into the points and fills counts and steps.
inline void traceNewCoarse(dsm_context *ctx, std::vector<TraceRequest> &reqs, const dsm_trace_params &params = traceDefaults()) {
  if (reqs.empty()) return;
  std::vector<trace_detail::Flat> flat(reqs.size());
  std::vector<dsm_trace_job> jobs(reqs.size());
  for (size_t i = 0; i < reqs.size(); i++) jobs[i] = trace_detail::flatten(flat[i], reqs[i]);
  immature_check(dsm_trace_points_batch(ctx, (int)jobs.size(), jobs.data(), &params), "traceNewCoarse");
  for (size_t i = 0; i < reqs.size(); i++) trace_detail::unpack(flat[i], reqs[i]);
}

// ... and for one sequence
inline void traceNewCoarse(dsm_context *ctx, TraceRequest &req, const dsm_trace_params &params = traceDefaults()) {
  trace_detail::Flat flat;
  dsm_trace_job job = trace_detail::flatten(flat, req);
  immature_check(dsm_trace_points_batch(ctx, 1, &job, &params), "traceNewCoarse");
  trace_detail::unpack(flat, req);
}

} // namespace dsm_host
