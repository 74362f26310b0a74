// hessian_demo.cpp -- accumulateAF_MT / accumulateSCF_MT of FrontEnd::optimize (dso_helpers/FrontEndOptimize.cpp:332-486) through
// the C++ adaptor host/WindowHessian.hpp, on a window read from a file: linearisation and accumulation for one window, then the same
// window twice in one call of the many-window form, then through the host form dsm_window_hessian_host; all three must agree.
// Input file (native byte order): the file of linearize_demo.cpp, then n_frames * n_frames * 64 doubles adHost, as many adTarget,
// per point 8 floats (priorF, deltaF, Hdd_accLF, bd_accLF, Hcd_accLF[4]) and int32 shiftPriorToZero.
// Usage: hessian_demo FILE.  Prints one JSON line: the new states as a digit string, the active flags as a digit string, the FNV-1a
// hashes of H_A, b_A, H_sc, b_sc, of JpJdF and of (HdiF, bdSumF, idepth_hessian), the bits of the energy sum, and whether the three
// forms agreed; exit status 0 when they did.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "WindowHessian.hpp"

using namespace dsm_host;

static uint64_t fnv1a(const void *p, size_t n, uint64_t hsh = 1469598103934665603ull) {
  for (size_t i = 0; i < n; i++) hsh = (hsh ^ ((const unsigned char *)p)[i]) * 1099511628211ull;
  return hsh;
}
template <typename T>
static uint64_t vhash(const std::vector<T> &v, uint64_t hsh = 1469598103934665603ull) {
  return fnv1a(v.data(), sizeof(T) * v.size(), hsh);
}

template <typename T>
static bool rd(FILE *f, std::vector<T> &v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

static bool same(const HessianRequest &a, const HessianRequest &b) {
  return a.lin.state_NewState == b.lin.state_NewState && vhash(a.lin.state_NewEnergy) == vhash(b.lin.state_NewEnergy) &&
         !memcmp(&a.lin.energy, &b.lin.energy, 8) && a.lin.kept == b.lin.kept && a.isActive == b.isActive && vhash(a.H_A) == vhash(b.H_A) &&
         vhash(a.b_A) == vhash(b.b_A) && vhash(a.H_sc) == vhash(b.H_sc) && vhash(a.b_sc) == vhash(b.b_sc) && vhash(a.JpJdF) == vhash(b.JpJdF) &&
         vhash(a.HdiF) == vhash(b.HdiF) && vhash(a.bdSumF) == vhash(b.bdSumF) && vhash(a.idepth_hessian) == vhash(b.idepth_hessian);
}

int main(int argc, char **argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: hessian_demo FILE\n");
    return 2;
  }
  FILE *f = fopen(argv[1], "rb");
  int wh[2], nff[2] = {0, 0}, n_pts = 0, n_res = 0, shift = 1;
  float cal[6];
  std::vector<int> ids;
  std::vector<float> planes, pre, eth, prec, rrec, pin;
  std::vector<double> adh, adt;
  bool good = f && fread(wh, sizeof(int), 2, f) == 2 && fread(cal, sizeof(float), 6, f) == 6 && fread(nff, sizeof(int), 2, f) == 2 &&
              nff[0] >= 1 && nff[0] <= DSM_WINDOW_MAX_FRAMES && wh[0] > 0 && wh[1] > 0;
  const size_t nf = good ? nff[0] : 0, npx = good ? (size_t)wh[0] * wh[1] : 0;
  good = good && rd(f, ids, nf) && rd(f, planes, nf * npx) && rd(f, pre, nf * nf * 27) && rd(f, eth, nf) && fread(&n_pts, sizeof(int), 1, f) == 1 &&
         n_pts >= 0 && rd(f, prec, (size_t)n_pts * 21) && fread(&n_res, sizeof(int), 1, f) == 1 && n_res >= 0 && rd(f, rrec, (size_t)n_res * 5) &&
         rd(f, adh, nf * nf * 64) && rd(f, adt, nf * nf * 64) && rd(f, pin, (size_t)n_pts * 8) && fread(&shift, sizeof(int), 1, f) == 1;
  if (!good) {
    fprintf(stderr, "hessian_demo: cannot read %s\n", argv[1]);
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
  HessianRequest res;
  {
    KeyframeWindow window(ctx, wh[0], wh[1], (int)nf), window2(ctx, wh[0], wh[1], (int)nf);
    for (size_t k = 0; k < nf; k++) {
      window.put(ids[k], &planes[k * npx]);
      window2.put(ids[nf - 1 - k], &planes[(nf - 1 - k) * npx]); // (the store's order is not the window's)
    }
    HessianRequest req;
    LinearizeRequest &lin = req.lin;
    lin.window = &window;
    lin.fxl = cal[0], lin.fyl = cal[1], lin.cxl = cal[2], lin.cyl = cal[3], lin.fxli = cal[4], lin.fyli = cal[5];
    lin.frame_ids = ids, lin.frameEnergyTH = eth, lin.points = &points, lin.residuals = &residuals, lin.fixLinearization = nff[1] != 0;
    lin.wantJacobians = false; // the rows stay on the device
    lin.precalc.resize(nf * nf);
    for (size_t k = 0; k < nf * nf; k++) {
      const float *q = &pre[27 * k];
      memcpy(lin.precalc[k].PRE_RTll_0, q, 36), memcpy(lin.precalc[k].PRE_tTll_0, q + 9, 12);
      memcpy(lin.precalc[k].PRE_KRKiTll, q + 12, 36), memcpy(lin.precalc[k].PRE_KtTll, q + 21, 12);
      memcpy(lin.precalc[k].PRE_aff_mode, q + 24, 8), lin.precalc[k].PRE_b0_mode = q[26];
    }
    req.adHost = adh, req.adTarget = adt, req.shiftPriorToZero = shift != 0;
    for (int i = 0; i < n_pts; i++) {
      const float *q = &pin[(size_t)8 * i];
      req.priorF.push_back(q[0]), req.deltaF.push_back(q[1]), req.Hdd_accLF.push_back(q[2]), req.bd_accLF.push_back(q[3]);
      req.Hcd_accLF.insert(req.Hcd_accLF.end(), q + 4, q + 8);
    }
    accumulateWindow(ctx, req); // one window
    res = req;

    std::vector<HessianRequest> reqs(2, req); // the windows of two sequences in one call
    reqs[1].lin.window = &window2;
    accumulateWindows(ctx, reqs);
    forms_equal = same(reqs[0], res) && same(reqs[1], res);

    // the host form on the same job
    dsm_linearize_params params;
    dsm_linearize_params_default(&params);
    linearize_detail::Flat flat;
    dsm_hessian_job job = hessian_detail::flatten(flat, req);
    std::vector<const float *> frame_I(nf);
    for (size_t k = 0; k < nf; k++) frame_I[k] = &planes[k * npx];
    immature_check(dsm_window_hessian_host(wh[0], wh[1], &job, frame_I.data(), &params), "dsm_window_hessian_host");
    hessian_detail::unpack(flat, req);
    forms_equal = forms_equal && same(req, res);
  }
  dsm_context_destroy(ctx);

  std::string states, active;
  for (size_t i = 0; i < res.lin.state_NewState.size(); i++) states += (char)('0' + res.lin.state_NewState[i]);
  for (size_t i = 0; i < res.isActive.size(); i++) active += (char)('0' + res.isActive[i]);
  uint64_t ebits;
  memcpy(&ebits, &res.lin.energy, 8);
  printf("{\"n_res\": %d, \"states\": \"%s\", \"active\": \"%s\", \"H_A\": \"%016llx\", \"b_A\": \"%016llx\", \"H_sc\": \"%016llx\", "
         "\"b_sc\": \"%016llx\", \"JpJdF\": \"%016llx\", \"points\": \"%016llx\", \"energy_bits\": \"%016llx\", \"forms_equal\": %d}\n",
         n_res, states.c_str(), active.c_str(), (unsigned long long)vhash(res.H_A), (unsigned long long)vhash(res.b_A),
         (unsigned long long)vhash(res.H_sc), (unsigned long long)vhash(res.b_sc), (unsigned long long)vhash(res.JpJdF),
         (unsigned long long)vhash(res.idepth_hessian, vhash(res.bdSumF, vhash(res.HdiF))), (unsigned long long)ebits, forms_equal);
  return forms_equal ? 0 : 1;
}
