// trace_new_coarse_demo.cpp -- the loop of FrontEnd::traceNewCoarse (FrontEnd.cpp:276-327) through the C++ adaptor
// host/TraceNewCoarse.hpp, on a sequence read from a file: its points through traceNewCoarse for one sequence (the new frame in a
// KeyframeWindow), then the same sequence twice in one call of the many-sequence form, then through the host form
// dsm_trace_points_host; all three must agree bit for bit.  A second frame follows, traced from the state the first left.
// Input file (native byte order): int32 w, h, n_frames (1 or 2), n_hosts, n_pts; n_frames planes of w * h floats; per host 14 floats
// (K R K^-1 row-major, K t, aff); per point int32 host, int32 status and 30 floats (u, v, energyTH, gradH[4], color[8], weights[8],
// idepth_min, idepth_max, quality, lastTraceUV[2], lastTracePixelInterval).
// Usage: trace_new_coarse_demo FILE.  Prints one JSON line: per frame the statuses as a digit string, the counts, the FNV-1a hash of
// the traced floats and the number of steps summed, and whether the three forms agreed; exit status 0 when they did.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "TraceNewCoarse.hpp"
#include "window_case.hpp" // fnv1a, rd

using namespace dsm_host;
using window_case::fnv1a;
using window_case::rd;

// idepth_min, idepth_max, quality, lastTraceUV, lastTracePixelInterval of every point, NaNs made canonical
static std::vector<float> traced(const std::vector<TracedPointData> &pts) {
  std::vector<float> out;
  for (const TracedPointData &p : pts) {
    const float v[6] = {p.idepth_min, p.idepth_max, p.quality, p.lastTraceUV[0], p.lastTraceUV[1], p.lastTracePixelInterval};
    for (float x : v) {
      if (x != x) {
        const uint32_t q = 0x7fc00000u;
        memcpy(&x, &q, 4);
      }
      out.push_back(x);
    }
  }
  return out;
}

static bool same(const std::vector<TracedPointData> &a, const std::vector<TracedPointData> &b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); i++)
    if (a[i].lastTraceStatus != b[i].lastTraceStatus) return false;
  const std::vector<float> x = traced(a), y = traced(b);
  return x.empty() || memcmp(x.data(), y.data(), 4 * x.size()) == 0;
}

int main(int argc, char **argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: trace_new_coarse_demo FILE\n");
    return 2;
  }
  FILE *f = fopen(argv[1], "rb");
  int hd[5] = {0, 0, 0, 0, 0};
  std::vector<float> planes, hosts;
  std::vector<int32_t> rec;
  bool good = f && fread(hd, sizeof(int), 5, f) == 5 && hd[0] > 0 && hd[1] > 0 && hd[2] >= 1 && hd[2] <= 2 && hd[3] >= 0 &&
              hd[3] <= DSM_TRACE_MAX_HOSTS && hd[4] >= 0;
  const int w = hd[0], h = hd[1], n_frames = hd[2], n_hosts = hd[3], n_pts = hd[4];
  const size_t npx = good ? (size_t)w * h : 0;
  good = good && rd(f, planes, n_frames * npx) && rd(f, hosts, (size_t)n_hosts * 14) && rd(f, rec, (size_t)n_pts * 32);
  if (!good) {
    fprintf(stderr, "trace_new_coarse_demo: cannot read %s\n", argv[1]);
    return 2;
  }
  fclose(f);
  std::vector<TracedPointData> points(n_pts);
  for (int i = 0; i < n_pts; i++) {
    const int32_t *q = &rec[(size_t)32 * i];
    float v[30];
    memcpy(v, q + 2, sizeof v);
    TracedPointData &p = points[i];
    p.host = q[0], p.lastTraceStatus = q[1];
    p.u = v[0], p.v = v[1], p.energyTH = v[2];
    memcpy(p.gradH, v + 3, 16), memcpy(p.color, v + 7, 32), memcpy(p.weights, v + 15, 32);
    p.idepth_min = v[23], p.idepth_max = v[24], p.quality = v[25], p.lastTraceUV[0] = v[26], p.lastTraceUV[1] = v[27];
    p.lastTracePixelInterval = v[28];
  }
  std::vector<HostToNew> h2n(n_hosts);
  for (int k = 0; k < n_hosts; k++) {
    memcpy(h2n[k].KRKi, &hosts[14 * k], 36), memcpy(h2n[k].Kt, &hosts[14 * k + 9], 12), memcpy(h2n[k].aff, &hosts[14 * k + 12], 8);
  }

  dsm_context *ctx = nullptr;
  immature_check(dsm_context_create(0, &ctx), "dsm_context_create");
  int forms_equal = 1;
  std::string out = "[";
  {
    KeyframeWindow window(ctx, w, h, n_frames);
    for (int k = 0; k < n_frames; k++) window.put(k, &planes[k * npx]);
    for (int k = 0; k < n_frames; k++) { // frame after frame: the points carry the state on
      std::vector<TracedPointData> one = points, many0 = points, many1 = points, on_host = points;
      TraceRequest req;
      req.window = &window, req.frame_id = k, req.hosts = h2n, req.points = &one;
      traceNewCoarse(ctx, req); // one sequence

      std::vector<TraceRequest> reqs(2, req); // two sequences in one call
      reqs[0].points = &many0, reqs[1].points = &many1;
      traceNewCoarse(ctx, reqs);
      forms_equal = forms_equal && same(many0, one) && same(many1, one) && memcmp(reqs[1].counts, req.counts, sizeof req.counts) == 0;

      TraceRequest hreq = req; // the host form on the same job
      hreq.points = &on_host;
      trace_detail::Flat flat;
      dsm_trace_job job = trace_detail::flatten(flat, hreq);
      const dsm_trace_params params = traceDefaults();
      immature_check(dsm_trace_points_host(w, h, &planes[k * npx], &job, &params), "dsm_trace_points_host");
      trace_detail::unpack(flat, hreq);
      forms_equal = forms_equal && same(on_host, one) && hreq.steps == req.steps;

      std::string statuses;
      long long steps = 0;
      for (int i = 0; i < n_pts; i++) statuses += (char)('0' + one[i].lastTraceStatus), steps += req.steps[i];
      const std::vector<float> t = traced(one);
      char buf[256];
      snprintf(buf, sizeof buf, "\", \"counts\": [%d, %d, %d, %d, %d, %d], \"hash\": \"%016llx\", \"steps\": %lld}", req.counts[0], req.counts[1],
               req.counts[2], req.counts[3], req.counts[4], req.counts[5], (unsigned long long)fnv1a(t.data(), 4 * t.size()), steps);
      out += std::string(k ? ", " : "") + "{\"statuses\": \"" + statuses + buf;
      points = one;
    }
  }
  dsm_context_destroy(ctx);
  printf("{\"n_pts\": %d, \"frames\": %s], \"forms_equal\": %d}\n", n_pts, out.c_str(), forms_equal);
  return forms_equal ? 0 : 1;
}
