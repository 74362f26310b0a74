// solve_demo.cpp -- one trial step of FrontEnd::optimize (dso_helpers/FrontEndOptimize.cpp:332-486) through the C++ adaptor
// host/WindowSolve.hpp, on a window read from a file: one window, then the same window twice in one call of the many-window form,
// then through the host form dsm_window_solve_host; all three must agree.
// Input file (native byte order): the file of hessian_demo.cpp, then with N = 4 + 8 n_frames: N * N doubles H_L, N b_L, N * N HM,
// N bM, N deltaX, one double lambda, int32 n_null, N * n_null doubles nullBasis and as many nullPinv.
// Usage: solve_demo FILE.  Prints one JSON line: the FNV-1a hashes of lastX, of the points' steps, of lastHS and lastbS, the step of
// the calibration as four doubles' bits hashed, the two finite flags, and whether the three forms agreed; exit status 0 when they did.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "WindowSolve.hpp"

using namespace dsm_host;

static uint64_t fnv1a(const void *p, size_t n, uint64_t hsh = 1469598103934665603ull) {
  for (size_t i = 0; i < n; i++) hsh = (hsh ^ ((const unsigned char *)p)[i]) * 1099511628211ull;
  return hsh;
}
template <typename T>
static uint64_t vhash(const std::vector<T> &v) {
  return fnv1a(v.data(), sizeof(T) * v.size());
}
template <typename T>
static bool rd(FILE *f, std::vector<T> &v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

static bool same(const SolveRequest &a, const SolveRequest &b) {
  return vhash(a.lastX) == vhash(b.lastX) && vhash(a.pointStep) == vhash(b.pointStep) && vhash(a.lastHS) == vhash(b.lastHS) &&
         vhash(a.lastbS) == vhash(b.lastbS) && a.xFinite == b.xFinite && a.stepsFinite == b.stepsFinite && vhash(a.hes.H_A) == vhash(b.hes.H_A) &&
         vhash(a.hes.H_sc) == vhash(b.hes.H_sc) && a.hes.isActive == b.hes.isActive && a.hes.lin.state_NewState == b.hes.lin.state_NewState;
}

int main(int argc, char **argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: solve_demo FILE\n");
    return 2;
  }
  FILE *f = fopen(argv[1], "rb");
  int wh[2], nff[2] = {0, 0}, n_pts = 0, n_res = 0, shift = 1, n_null = 0;
  float cal[6];
  double lambda = 0;
  std::vector<int> ids;
  std::vector<float> planes, pre, eth, prec, rrec, pin;
  std::vector<double> adh, adt, HL, bL, HM, bM, dx, basis, pinv;
  bool good = f && fread(wh, sizeof(int), 2, f) == 2 && fread(cal, sizeof(float), 6, f) == 6 && fread(nff, sizeof(int), 2, f) == 2 &&
              nff[0] >= 1 && nff[0] <= DSM_WINDOW_MAX_FRAMES && wh[0] > 0 && wh[1] > 0;
  const size_t nf = good ? nff[0] : 0, npx = good ? (size_t)wh[0] * wh[1] : 0, N = 4 + 8 * nf;
  good = good && rd(f, ids, nf) && rd(f, planes, nf * npx) && rd(f, pre, nf * nf * 27) && rd(f, eth, nf) && fread(&n_pts, sizeof(int), 1, f) == 1 &&
         n_pts >= 0 && rd(f, prec, (size_t)n_pts * 21) && fread(&n_res, sizeof(int), 1, f) == 1 && n_res >= 0 && rd(f, rrec, (size_t)n_res * 5) &&
         rd(f, adh, nf * nf * 64) && rd(f, adt, nf * nf * 64) && rd(f, pin, (size_t)n_pts * 8) && fread(&shift, sizeof(int), 1, f) == 1;
  good = good && rd(f, HL, N * N) && rd(f, bL, N) && rd(f, HM, N * N) && rd(f, bM, N) && rd(f, dx, N) && fread(&lambda, sizeof(double), 1, f) == 1 &&
         fread(&n_null, sizeof(int), 1, f) == 1 && n_null >= 0 && n_null <= DSM_SOLVE_MAX_NULL && rd(f, basis, N * n_null) && rd(f, pinv, N * n_null);
  if (!good) {
    fprintf(stderr, "solve_demo: cannot read %s\n", argv[1]);
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
  SolveRequest res;
  {
    KeyframeWindow window(ctx, wh[0], wh[1], (int)nf), window2(ctx, wh[0], wh[1], (int)nf);
    for (size_t k = 0; k < nf; k++) {
      window.put(ids[k], &planes[k * npx]);
      window2.put(ids[nf - 1 - k], &planes[(nf - 1 - k) * npx]); // (the store's order is not the window's)
    }
    SolveRequest req;
    LinearizeRequest &lin = req.hes.lin;
    lin.window = &window;
    lin.fxl = cal[0], lin.fyl = cal[1], lin.cxl = cal[2], lin.cyl = cal[3], lin.fxli = cal[4], lin.fyli = cal[5];
    lin.frame_ids = ids, lin.frameEnergyTH = eth, lin.points = &points, lin.residuals = &residuals, lin.fixLinearization = nff[1] != 0;
    lin.wantJacobians = false;
    lin.precalc.resize(nf * nf);
    for (size_t k = 0; k < nf * nf; k++) {
      const float *q = &pre[27 * k];
      memcpy(lin.precalc[k].PRE_RTll_0, q, 36), memcpy(lin.precalc[k].PRE_tTll_0, q + 9, 12);
      memcpy(lin.precalc[k].PRE_KRKiTll, q + 12, 36), memcpy(lin.precalc[k].PRE_KtTll, q + 21, 12);
      memcpy(lin.precalc[k].PRE_aff_mode, q + 24, 8), lin.precalc[k].PRE_b0_mode = q[26];
    }
    req.hes.adHost = adh, req.hes.adTarget = adt, req.hes.shiftPriorToZero = shift != 0;
    for (int i = 0; i < n_pts; i++) {
      const float *q = &pin[(size_t)8 * i];
      req.hes.priorF.push_back(q[0]), req.hes.deltaF.push_back(q[1]), req.hes.Hdd_accLF.push_back(q[2]), req.hes.bd_accLF.push_back(q[3]);
      req.hes.Hcd_accLF.insert(req.hes.Hcd_accLF.end(), q + 4, q + 8);
    }
    req.H_L = HL, req.b_L = bL, req.HM = HM, req.bM = bM, req.deltaX = dx, req.lambda = lambda, req.nullBasis = basis, req.nullPinv = pinv;
    req.wantStitched = true;
    solveWindow(ctx, req); // one window
    res = req;

    std::vector<SolveRequest> reqs(2, req); // the windows of two sequences in one call
    reqs[1].hes.lin.window = &window2;
    solveWindows(ctx, reqs);
    forms_equal = same(reqs[0], res) && same(reqs[1], res);

    // x and the steps alone are the same x and steps
    SolveRequest lean = req;
    lean.wantStitched = false;
    solveWindow(ctx, lean);
    forms_equal = forms_equal && vhash(lean.lastX) == vhash(res.lastX) && vhash(lean.pointStep) == vhash(res.pointStep) && lean.hes.H_A.empty();

    // the host form on the same job
    dsm_linearize_params params;
    dsm_linearize_params_default(&params);
    solve_detail::Flat flat;
    dsm_solve_job job = solve_detail::flatten(flat, req);
    std::vector<const float *> frame_I(nf);
    for (size_t k = 0; k < nf; k++) frame_I[k] = &planes[k * npx];
    immature_check(dsm_window_solve_host(wh[0], wh[1], &job, frame_I.data(), &params), "dsm_window_solve_host");
    solve_detail::unpack(flat, req);
    forms_equal = forms_equal && same(req, res);
  }
  dsm_context_destroy(ctx);

  double c[4];
  res.stepC(c);
  printf("{\"n_res\": %d, \"x\": \"%016llx\", \"step\": \"%016llx\", \"last_HS\": \"%016llx\", \"last_bS\": \"%016llx\", \"step_c\": \"%016llx\", "
         "\"x_finite\": %d, \"steps_finite\": %d, \"forms_equal\": %d}\n",
         n_res, (unsigned long long)vhash(res.lastX), (unsigned long long)vhash(res.pointStep), (unsigned long long)vhash(res.lastHS),
         (unsigned long long)vhash(res.lastbS), (unsigned long long)fnv1a(c, sizeof c), (int)res.xFinite, (int)res.stepsFinite, forms_equal);
  return forms_equal ? 0 : 1;
}
