// nullspace_demo.cpp -- what FrontEnd::solveSystem does before a solve (dso_helpers/FrontEndOptimize.cpp:488-494: getNullspaces, :525-574)
// through the C++ adaptor host/WindowNullspace.hpp, on a window read from a file: one window, then two windows (this one and a second
// set of poses) in one call, then the device's basis fed to host/WindowSolve.hpp as rule F7 reads it, then the host form.
// Input file (native byte order): the file of solve_demo.cpp (its n_null, nullBasis and nullPinv are read and not used), then n_frames * 7
// doubles worldToCamEval, n_frames * 8 stateZero, n_frames floats exposure, and the same three arrays of a second window of n_frames.
// Usage: nullspace_demo FILE OUT.  Writes to OUT the device's nullBasis (N * 7 doubles), nullPinv (7 * N) and frameNull (n_frames * 42) of
// the first window.  Prints one JSON line: the rank and flags of both windows, the hash of lastX of the solve with the device's basis,
// whether the two-window call repeated the one-window call, whether the host form given the device's frameNull repeated the device's
// basis, pseudo-inverse, singular values, rank and flags bit for bit, and the hashes of the host form's own nullBasis and nullPinv from
// the poses; exit status 0 when the forms agreed.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "WindowNullspace.hpp"

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
static bool same(const WindowNullspace &a, const WindowNullspace &b) {
  return vhash(a.nullBasis) == vhash(b.nullBasis) && vhash(a.nullPinv) == vhash(b.nullPinv) && a.rank == b.rank && a.flags == b.flags &&
         memcmp(a.singularValues, b.singularValues, sizeof a.singularValues) == 0;
}

int main(int argc, char **argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: nullspace_demo FILE OUT\n");
    return 2;
  }
  FILE *f = fopen(argv[1], "rb");
  int wh[2], nff[2] = {0, 0}, n_pts = 0, n_res = 0, shift = 1, n_null = 0;
  float cal[6];
  double lambda = 0;
  std::vector<int> ids;
  std::vector<float> planes, pre, eth, prec, rrec, pin;
  std::vector<double> adh, adt, HL, bL, HM, bM, dx, basis, pinv;
  WindowNullspace ns, ns2;
  bool good = f && fread(wh, sizeof(int), 2, f) == 2 && fread(cal, sizeof(float), 6, f) == 6 && fread(nff, sizeof(int), 2, f) == 2 &&
              nff[0] >= 1 && nff[0] <= DSM_WINDOW_MAX_FRAMES && wh[0] > 0 && wh[1] > 0;
  const size_t nf = good ? nff[0] : 0, npx = good ? (size_t)wh[0] * wh[1] : 0, N = 4 + 8 * nf;
  good = good && rd(f, ids, nf) && rd(f, planes, nf * npx) && rd(f, pre, nf * nf * 27) && rd(f, eth, nf) && fread(&n_pts, sizeof(int), 1, f) == 1 &&
         n_pts >= 0 && rd(f, prec, (size_t)n_pts * 21) && fread(&n_res, sizeof(int), 1, f) == 1 && n_res >= 0 && rd(f, rrec, (size_t)n_res * 5) &&
         rd(f, adh, nf * nf * 64) && rd(f, adt, nf * nf * 64) && rd(f, pin, (size_t)n_pts * 8) && fread(&shift, sizeof(int), 1, f) == 1;
  good = good && rd(f, HL, N * N) && rd(f, bL, N) && rd(f, HM, N * N) && rd(f, bM, N) && rd(f, dx, N) && fread(&lambda, sizeof(double), 1, f) == 1 &&
         fread(&n_null, sizeof(int), 1, f) == 1 && n_null >= 0 && n_null <= DSM_SOLVE_MAX_NULL && rd(f, basis, N * n_null) && rd(f, pinv, N * n_null);
  good = good && rd(f, ns.worldToCamEval, 7 * nf) && rd(f, ns.stateZero, 8 * nf) && rd(f, ns.exposure, nf) && rd(f, ns2.worldToCamEval, 7 * nf) &&
         rd(f, ns2.stateZero, 8 * nf) && rd(f, ns2.exposure, nf);
  if (!good) {
    fprintf(stderr, "nullspace_demo: cannot read %s\n", argv[1]);
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
  int windows_equal = 0, host_repeats_device = 0;
  WindowNullspace dev, host_own;
  SolveRequest req;
  {
    ns.compute(ctx); // one window
    dev = ns;
    WindowNullspace a = ns, b = ns2; // the windows of two sequences in one call
    std::vector<WindowNullspace *> both;
    both.push_back(&a), both.push_back(&b);
    WindowNullspace::computeMany(ctx, both);
    ns2.compute(ctx);
    windows_equal = same(a, dev) && same(b, ns2) && vhash(a.frameNull) == vhash(dev.frameNull) && vhash(b.nullspacesX0Pre) == vhash(ns2.nullspacesX0Pre);

    // the device's basis where rule F7 reads it
    KeyframeWindow window(ctx, wh[0], wh[1], (int)nf);
    for (size_t k = 0; k < nf; k++) window.put(ids[k], &planes[k * npx]);
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
    req.H_L = HL, req.b_L = bL, req.HM = HM, req.bM = bM, req.deltaX = dx, req.lambda = lambda;
    dev.applyTo(req);
    solveWindow(ctx, req);

    // the host form: behind the device's blocks it repeats the device bit for bit; from the poses it is the C library's atan and tan
    WindowNullspace given = ns;
    given.frameNullIn = dev.frameNull;
    given.computeHost();
    host_repeats_device = same(given, dev) && vhash(given.nullspacesX0Pre) == vhash(dev.nullspacesX0Pre);
    host_own = ns;
    host_own.computeHost();
  }
  dsm_context_destroy(ctx);

  FILE *o = fopen(argv[2], "wb");
  if (!o || fwrite(dev.nullBasis.data(), 8, dev.nullBasis.size(), o) != dev.nullBasis.size() ||
      fwrite(dev.nullPinv.data(), 8, dev.nullPinv.size(), o) != dev.nullPinv.size() ||
      fwrite(dev.frameNull.data(), 8, dev.frameNull.size(), o) != dev.frameNull.size() || fclose(o) != 0) {
    fprintf(stderr, "nullspace_demo: cannot write %s\n", argv[2]);
    return 2;
  }
  printf("{\"rank\": [%d, %d], \"flags\": [%d, %d], \"x\": \"%016llx\", \"x_finite\": %d, \"windows_equal\": %d, \"host_repeats_device\": %d, "
         "\"host_basis\": \"%016llx\", \"host_pinv\": \"%016llx\", \"host_pre\": \"%016llx\", \"scale_column\": \"%016llx\"}\n",
         dev.rank, ns2.rank, dev.flags, ns2.flags, (unsigned long long)vhash(req.lastX), (int)req.xFinite, windows_equal, host_repeats_device,
         (unsigned long long)vhash(host_own.nullBasis), (unsigned long long)vhash(host_own.nullPinv), (unsigned long long)vhash(host_own.nullspacesX0Pre),
         (unsigned long long)vhash(host_own.nullspaceScale()));
  return windows_equal && host_repeats_device ? 0 : 1;
}
