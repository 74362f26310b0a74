// immature_points_demo.cpp -- the second half of FrontEnd::activatePointsMT (FrontEnd.cpp:458-468) through the C++ adaptor
// host/ImmaturePoints.hpp, on a window read from a file: the window's points through optimizeImmaturePoints for one window, then
// the same window twice in one call of the many-window form, then through the host form dsm_optimize_immature_points_host; all
// three must agree.
// Input file (native byte order): int32 w, h; float fxl, fyl, cxl, cyl, fxli, fyli; int32 n_frames, min_obs; n_frames int32 frame
// ids; n_frames planes of w * h floats; n_frames * n_frames precalc entries of 14 floats (R row-major, t, aff), [host][target];
// int32 n_pts; per point int32 host and 21 floats (u, v, idepth_min, idepth_max, energyTH, color[8], weights[8]).
// Usage: immature_points_demo FILE.  Prints one JSON line: the statuses as a digit string, the FNV-1a hash of the idepth floats, per
// point the IN-target list and the lastResiduals indices, and whether the three forms agreed; exit status 0 when they did.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "ImmaturePoints.hpp"
#include "window_case.hpp" // fnv1a, rd

using namespace dsm_host;
using window_case::fnv1a;
using window_case::rd;

static bool same(const std::vector<OptimizedPoint> &a, const std::vector<OptimizedPoint> &b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); i++)
    if (a[i].status != b[i].status || memcmp(&a[i].idepth, &b[i].idepth, 4) || a[i].in_targets != b[i].in_targets ||
        a[i].last_residual[0] != b[i].last_residual[0] || a[i].last_residual[1] != b[i].last_residual[1])
      return false;
  return true;
}

int main(int argc, char **argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: immature_points_demo FILE\n");
    return 2;
  }
  FILE *f = fopen(argv[1], "rb");
  int wh[2], nfm[2] = {0, 0}, n_pts = 0;
  float cal[6];
  std::vector<int> ids;
  std::vector<float> planes, pre, rec;
  bool good = f && fread(wh, sizeof(int), 2, f) == 2 && fread(cal, sizeof(float), 6, f) == 6 && fread(nfm, sizeof(int), 2, f) == 2 &&
              nfm[0] >= 1 && nfm[0] <= DSM_IMMATURE_MAX_FRAMES && wh[0] > 0 && wh[1] > 0;
  const size_t nf = good ? nfm[0] : 0, npx = good ? (size_t)wh[0] * wh[1] : 0;
  good = good && rd(f, ids, nf) && rd(f, planes, nf * npx) && rd(f, pre, nf * nf * 14) && fread(&n_pts, sizeof(int), 1, f) == 1 && n_pts >= 0 &&
         rd(f, rec, (size_t)n_pts * 22);
  if (!good) {
    fprintf(stderr, "immature_points_demo: cannot read %s\n", argv[1]);
    return 2;
  }
  fclose(f);
  std::vector<ImmaturePointData> points(n_pts);
  for (int i = 0; i < n_pts; i++) {
    const float *q = &rec[(size_t)22 * i];
    memcpy(&points[i].host, q, 4);
    points[i].u = q[1], points[i].v = q[2], points[i].idepth_min = q[3], points[i].idepth_max = q[4], points[i].energyTH = q[5];
    memcpy(points[i].color, q + 6, 32);
    memcpy(points[i].weights, q + 14, 32);
  }

  dsm_context *ctx = nullptr;
  immature_check(dsm_context_create(0, &ctx), "dsm_context_create");
  int forms_equal = 0;
  std::vector<OptimizedPoint> res;
  {
    KeyframeWindow window(ctx, wh[0], wh[1], (int)nf), window2(ctx, wh[0], wh[1], (int)nf);
    for (size_t k = 0; k < nf; k++) {
      window.put(ids[k], &planes[k * npx]);
      window2.put(ids[nf - 1 - k], &planes[(nf - 1 - k) * npx]); // (the store's order is not the window's)
    }
    ImmatureRequest req;
    req.window = &window;
    req.fxl = cal[0], req.fyl = cal[1], req.cxl = cal[2], req.cyl = cal[3], req.fxli = cal[4], req.fyli = cal[5];
    req.frame_ids = ids, req.points = &points, req.min_obs = nfm[1];
    req.precalc.resize(nf * nf);
    for (size_t k = 0; k < nf * nf; k++) {
      memcpy(req.precalc[k].PRE_RTll, &pre[14 * k], 36);
      memcpy(req.precalc[k].PRE_tTll, &pre[14 * k + 9], 12);
      memcpy(req.precalc[k].PRE_aff_mode, &pre[14 * k + 12], 8);
    }
    optimizeImmaturePoints(ctx, req); // one window
    res = req.results;

    std::vector<ImmatureRequest> reqs(2, req); // the windows of two sequences in one call
    reqs[1].window = &window2;
    optimizeImmaturePoints(ctx, reqs);
    forms_equal = same(reqs[0].results, res) && same(reqs[1].results, res);

    // the host form on the same job
    immature_detail::Flat flat;
    dsm_immature_job job = immature_detail::flatten(flat, req);
    std::vector<const float *> frame_I(nf);
    for (size_t k = 0; k < nf; k++) frame_I[k] = &planes[k * npx];
    immature_check(dsm_optimize_immature_points_host(wh[0], wh[1], &job, frame_I.data(), DSM_IMMATURE_HUBER_TH, DSM_IMMATURE_MIN_IDEPTH_H_ACT,
                                                     DSM_IMMATURE_GN_ITERATIONS),
                   "dsm_optimize_immature_points_host");
    immature_detail::unpack(flat, req);
    forms_equal = forms_equal && same(req.results, res);
  }
  dsm_context_destroy(ctx);

  std::string statuses, targets = "[", last = "[";
  std::vector<float> idepths;
  for (size_t i = 0; i < res.size(); i++) {
    statuses += (char)('0' + res[i].status);
    idepths.push_back(res[i].idepth);
    targets += i ? ", [" : "[";
    for (size_t k = 0; k < res[i].in_targets.size(); k++) targets += (k ? ", " : "") + std::to_string(ids[res[i].in_targets[k]]);
    targets += "]";
    last += (i ? ", [" : "[") + std::to_string(res[i].last_residual[0]) + ", " + std::to_string(res[i].last_residual[1]) + "]";
  }
  targets += "]", last += "]";
  printf("{\"n_pts\": %d, \"statuses\": \"%s\", \"idepth_hash\": \"%016llx\", \"in_targets\": %s, \"last_residuals\": %s, \"forms_equal\": %d}\n",
         n_pts, statuses.c_str(), (unsigned long long)fnv1a(idepths.data(), 4 * idepths.size()), targets.c_str(), last.c_str(), forms_equal);
  return forms_equal ? 0 : 1;
}
