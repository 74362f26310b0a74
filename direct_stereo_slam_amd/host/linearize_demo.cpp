// linearize_demo.cpp -- FrontEnd::linearizeAll (dso_helpers/FrontEndOptimize.cpp:121-179) through the C++ adaptor
// host/ResidualLinearizer.hpp, on a window read from a file: the window's active residuals through linearizeAll for one window, then
// the same window twice in one call of the many-window form, then through the host form dsm_linearize_residuals_host; all three must
// agree.
// Input file (native byte order): int32 w, h; float fxl, fyl, cxl, cyl, fxli, fyli; int32 n_frames, fix_linearization; n_frames int32
// frame ids; n_frames planes of w * h floats; n_frames * n_frames precalc entries of 27 floats (PRE_RTll_0, PRE_tTll_0, PRE_KRKiTll,
// PRE_KtTll, PRE_aff_mode, PRE_b0_mode), [host][target]; n_frames floats frameEnergyTH; int32 n_pts; per point int32 host and 20 floats
// (u, v, idepth_scaled, idepth_zero_scaled, color[8], weights[8]); int32 n_res; per residual int32 point, target, state, float energy,
// int32 isNew.
// Usage: linearize_demo FILE.  Prints one JSON line: the new states as a digit string, the FNV-1a hashes of the energies and of the
// Jacobian rows of the residuals that did not end OOB, the bits of the energy sum and of the new threshold, the kept list, the points
// with a new good residual, and whether the three forms agreed; exit status 0 when they did.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "ResidualLinearizer.hpp"

using namespace dsm_host;

static uint64_t fnv1a(const void *p, size_t n, uint64_t hsh = 1469598103934665603ull) {
  for (size_t i = 0; i < n; i++) hsh = (hsh ^ ((const unsigned char *)p)[i]) * 1099511628211ull;
  return hsh;
}

template <typename T>
static bool rd(FILE *f, std::vector<T> &v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

static uint64_t row_hash(const LinearizeRequest &r) {
  uint64_t hsh = 1469598103934665603ull;
  for (size_t i = 0; i < r.J.size(); i++)
    if (r.state_NewState[i] != DSM_RES_OOB) {
      hsh = fnv1a(&r.J[i], sizeof(RawResidualJacobian), hsh);
      hsh = fnv1a(&r.centerProjectedTo[3 * i], 12, hsh);
      hsh = fnv1a(&r.projectedTo[16 * i], 64, hsh);
    }
  return hsh;
}

static bool same(const LinearizeRequest &a, const LinearizeRequest &b) {
  return a.state_NewState == b.state_NewState && a.state_NewEnergy.size() == b.state_NewEnergy.size() &&
         !memcmp(a.state_NewEnergy.data(), b.state_NewEnergy.data(), 4 * a.state_NewEnergy.size()) &&
         !memcmp(a.state_NewEnergyWithOutlier.data(), b.state_NewEnergyWithOutlier.data(), 4 * a.state_NewEnergy.size()) &&
         row_hash(a) == row_hash(b) && !memcmp(&a.energy, &b.energy, 8) && !memcmp(&a.newFrameEnergyTH, &b.newFrameEnergyTH, 4) &&
         a.kept == b.kept && a.toRemove == b.toRemove && a.numGoodResiduals == b.numGoodResiduals &&
         !memcmp(a.maxRelBaseline.data(), b.maxRelBaseline.data(), 4 * a.maxRelBaseline.size());
}

int main(int argc, char **argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: linearize_demo FILE\n");
    return 2;
  }
  FILE *f = fopen(argv[1], "rb");
  int wh[2], nff[2] = {0, 0}, n_pts = 0, n_res = 0;
  float cal[6];
  std::vector<int> ids;
  std::vector<float> planes, pre, eth, prec, rrec;
  bool good = f && fread(wh, sizeof(int), 2, f) == 2 && fread(cal, sizeof(float), 6, f) == 6 && fread(nff, sizeof(int), 2, f) == 2 &&
              nff[0] >= 1 && nff[0] <= DSM_WINDOW_MAX_FRAMES && wh[0] > 0 && wh[1] > 0;
  const size_t nf = good ? nff[0] : 0, npx = good ? (size_t)wh[0] * wh[1] : 0;
  good = good && rd(f, ids, nf) && rd(f, planes, nf * npx) && rd(f, pre, nf * nf * 27) && rd(f, eth, nf) && fread(&n_pts, sizeof(int), 1, f) == 1 &&
         n_pts >= 0 && rd(f, prec, (size_t)n_pts * 21) && fread(&n_res, sizeof(int), 1, f) == 1 && n_res >= 0 && rd(f, rrec, (size_t)n_res * 5);
  if (!good) {
    fprintf(stderr, "linearize_demo: cannot read %s\n", argv[1]);
    return 2;
  }
  fclose(f);
  std::vector<ActivePointData> points(n_pts);
  for (int i = 0; i < n_pts; i++) {
    const float *q = &prec[(size_t)21 * i];
    memcpy(&points[i].host, q, 4);
    points[i].u = q[1], points[i].v = q[2], points[i].idepth_scaled = q[3], points[i].idepth_zero_scaled = q[4];
    memcpy(points[i].color, q + 5, 32);
    memcpy(points[i].weights, q + 13, 32);
  }
  std::vector<ActiveResidualData> residuals(n_res);
  for (int i = 0; i < n_res; i++) {
    const float *q = &rrec[(size_t)5 * i];
    int isnew;
    memcpy(&residuals[i].point, q, 4), memcpy(&residuals[i].target, q + 1, 4), memcpy(&residuals[i].state_state, q + 2, 4);
    residuals[i].state_energy = q[3];
    memcpy(&isnew, q + 4, 4);
    residuals[i].isNew = isnew != 0;
  }

  dsm_context *ctx = nullptr;
  immature_check(dsm_context_create(0, &ctx), "dsm_context_create");
  int forms_equal = 0;
  LinearizeRequest res;
  {
    KeyframeWindow window(ctx, wh[0], wh[1], (int)nf), window2(ctx, wh[0], wh[1], (int)nf);
    for (size_t k = 0; k < nf; k++) {
      window.put(ids[k], &planes[k * npx]);
      window2.put(ids[nf - 1 - k], &planes[(nf - 1 - k) * npx]); // (the store's order is not the window's)
    }
    LinearizeRequest req;
    req.window = &window;
    req.fxl = cal[0], req.fyl = cal[1], req.cxl = cal[2], req.cyl = cal[3], req.fxli = cal[4], req.fyli = cal[5];
    req.frame_ids = ids, req.frameEnergyTH = eth, req.points = &points, req.residuals = &residuals, req.fixLinearization = nff[1] != 0;
    req.precalc.resize(nf * nf);
    for (size_t k = 0; k < nf * nf; k++) {
      const float *q = &pre[27 * k];
      memcpy(req.precalc[k].PRE_RTll_0, q, 36), memcpy(req.precalc[k].PRE_tTll_0, q + 9, 12);
      memcpy(req.precalc[k].PRE_KRKiTll, q + 12, 36), memcpy(req.precalc[k].PRE_KtTll, q + 21, 12);
      memcpy(req.precalc[k].PRE_aff_mode, q + 24, 8), req.precalc[k].PRE_b0_mode = q[26];
    }
    linearizeAll(ctx, req); // one window
    res = req;

    std::vector<LinearizeRequest> reqs(2, req); // the windows of two sequences in one call
    reqs[1].window = &window2;
    linearizeAll(ctx, reqs);
    forms_equal = same(reqs[0], res) && same(reqs[1], res);

    // the host form on the same job
    dsm_linearize_params params;
    dsm_linearize_params_default(&params);
    linearize_detail::Flat flat;
    dsm_linearize_job job = linearize_detail::flatten(flat, req);
    std::vector<const float *> frame_I(nf);
    for (size_t k = 0; k < nf; k++) frame_I[k] = &planes[k * npx];
    immature_check(dsm_linearize_residuals_host(wh[0], wh[1], &job, frame_I.data(), &params), "dsm_linearize_residuals_host");
    linearize_detail::unpack(flat, req);
    forms_equal = forms_equal && same(req, res);
  }
  dsm_context_destroy(ctx);

  std::string states, kept = "[", goodp = "[";
  for (size_t i = 0; i < res.state_NewState.size(); i++) states += (char)('0' + res.state_NewState[i]);
  for (size_t i = 0; i < res.kept.size(); i++) kept += (i ? ", " : "") + std::to_string(res.kept[i]);
  bool first = true;
  for (size_t p = 0; p < res.numGoodResiduals.size(); p++)
    if (res.numGoodResiduals[p]) {
      uint32_t bits;
      memcpy(&bits, &res.maxRelBaseline[p], 4);
      goodp += std::string(first ? "[" : ", [") + std::to_string(p) + ", " + std::to_string(res.numGoodResiduals[p]) + ", " + std::to_string(bits) + "]";
      first = false;
    }
  kept += "]", goodp += "]";
  uint64_t ebits;
  uint32_t tbits;
  memcpy(&ebits, &res.energy, 8), memcpy(&tbits, &res.newFrameEnergyTH, 4);
  uint64_t eh = fnv1a(res.state_NewEnergy.data(), 4 * res.state_NewEnergy.size());
  eh = fnv1a(res.state_NewEnergyWithOutlier.data(), 4 * res.state_NewEnergyWithOutlier.size(), eh);
  printf("{\"n_res\": %d, \"states\": \"%s\", \"energy_hash\": \"%016llx\", \"row_hash\": \"%016llx\", \"energy_bits\": \"%016llx\", "
         "\"threshold_bits\": \"%08x\", \"kept\": %s, \"good_points\": %s, \"forms_equal\": %d}\n",
         n_res, states.c_str(), (unsigned long long)eh, (unsigned long long)row_hash(res), (unsigned long long)ebits, tbits, kept.c_str(),
         goodp.c_str(), forms_equal);
  return forms_equal ? 0 : 1;
}
