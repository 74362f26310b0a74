// optimize_demo.cpp -- the loop of FrontEnd::optimize (dso_helpers/FrontEndOptimize.cpp:362-371, :382-453) as ONE call through the C++
// adaptor host/WindowOptimize.hpp, on two windows read from files: window A alone on the device, A and B -- two DIFFERENT windows -- in
// one call, where each takes its own decisions, and both through the host form.
// Input files (native byte order): the step file host/step_demo.cpp reads (tests/_step_ref.py, write_case); a file's state_backup,
// calib_backup and idepth_backup are the state the loop starts from, its step and factors are not used.
// Usage: optimize_demo FILE_A FILE_B [MAX_ITERATIONS = 6].  Prints one JSON line: per run the accept / reject pattern, the passes, the
// FNV-1a hashes of the final state, calibration and inverse depths and of the last energy, and that energy.  Exit status 0 when A in
// the call of two equalled A alone, B in the call of two equalled B alone, and A and B decided differently.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "WindowOptimize.hpp"

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

struct Outcome {
  std::string pattern;
  int passes = 0;
  uint64_t state = 0, calib = 0, idepth = 0, energy = 0;
  double last = 0;
  bool operator==(const Outcome &o) const {
    return pattern == o.pattern && passes == o.passes && state == o.state && calib == o.calib && idepth == o.idepth && energy == o.energy;
  }
};

static Outcome outcome(const WindowOptimize &o, const OptimizeResult &r) {
  Outcome out;
  out.pattern = r.pattern, out.passes = r.passes, out.last = r.lastEnergy + r.lastEnergyM;
  out.state = fnv1a(o.window.state.data(), 8 * o.window.state.size()), out.calib = fnv1a(o.window.calib, 32);
  out.idepth = fnv1a(o.window.idepth.data(), 4 * o.window.idepth.size()), out.energy = fnv1a(&out.last, 8);
  return out;
}

// a window of a step file: the prototype of its WindowOptimize, its planes and its points
struct Case {
  int wh[2] = {0, 0};
  std::vector<int> ids;
  std::vector<float> planes;
  std::vector<ActivePointData> points;
  WindowOptimize proto;
  size_t nf = 0, npx = 0;
};

static bool load(const char *path, Case &c) {
  FILE *f = fopen(path, "rb");
  int nff[2] = {0, 0}, n_pts = 0, n_res = 0, shift = 1, n_null = 0, has_hm = 0, has_prior = 0;
  float cal[6];
  double lambda = 0;
  std::vector<float> pre, eth, prec, rrec, pin, idb, ids_step, expo, fac;
  std::vector<double> adh, adt, HL, bL, HM, bM, basis, pinv, ev, zero, backup, fstep, cz, cb, cs, prior, pzero;
  bool good = f && fread(c.wh, sizeof(int), 2, f) == 2 && fread(cal, sizeof(float), 6, f) == 6 && fread(nff, sizeof(int), 2, f) == 2 && nff[0] >= 1 &&
              nff[0] <= DSM_WINDOW_MAX_FRAMES && c.wh[0] > 0 && c.wh[1] > 0;
  const size_t nf = good ? nff[0] : 0, npx = good ? (size_t)c.wh[0] * c.wh[1] : 0, N = 4 + 8 * nf;
  good = good && rd(f, c.ids, nf) && rd(f, c.planes, nf * npx) && rd(f, pre, nf * nf * 27) && rd(f, eth, nf) && fread(&n_pts, sizeof(int), 1, f) == 1 &&
         n_pts >= 0 && rd(f, prec, (size_t)n_pts * 21) && fread(&n_res, sizeof(int), 1, f) == 1 && n_res >= 0 && rd(f, rrec, (size_t)n_res * 5) &&
         rd(f, adh, nf * nf * 64) && rd(f, adt, nf * nf * 64) && rd(f, pin, (size_t)n_pts * 8) && fread(&shift, sizeof(int), 1, f) == 1;
  good = good && rd(f, HL, N * N) && rd(f, bL, N) && fread(&has_hm, sizeof(int), 1, f) == 1 && (!has_hm || (rd(f, HM, N * N) && rd(f, bM, N))) &&
         fread(&lambda, sizeof(double), 1, f) == 1 && fread(&n_null, sizeof(int), 1, f) == 1 && n_null >= 0 && n_null <= DSM_SOLVE_MAX_NULL &&
         rd(f, basis, N * n_null) && rd(f, pinv, N * n_null);
  good = good && rd(f, ev, 7 * nf) && rd(f, zero, 8 * nf) && rd(f, backup, 8 * nf) && rd(f, fstep, 8 * nf) && rd(f, cz, 4) && rd(f, cb, 4) && rd(f, cs, 4) &&
         rd(f, idb, n_pts) && rd(f, ids_step, n_pts) && rd(f, expo, nf) && rd(f, fac, 5) && fread(&has_prior, sizeof(int), 1, f) == 1 &&
         (!has_prior || (rd(f, prior, N) && rd(f, pzero, N)));
  if (f) fclose(f);
  if (!good) return false;
  c.nf = nf, c.npx = npx;
  c.points.resize(n_pts);
  for (int i = 0; i < n_pts; i++) {
    const float *q = &prec[(size_t)21 * i];
    memcpy(&c.points[i].host, q, 4);
    c.points[i].u = q[1], c.points[i].v = q[2], c.points[i].idepth_scaled = 0, c.points[i].idepth_zero_scaled = 0;
    memcpy(c.points[i].color, q + 5, 32);
    memcpy(c.points[i].weights, q + 13, 32);
  }
  WindowStep &w = c.proto.window;
  w.residuals.resize(n_res);
  for (int i = 0; i < n_res; i++) {
    const float *q = &rrec[(size_t)5 * i];
    int isnew;
    ActiveResidualData &r = w.residuals[i];
    memcpy(&r.point, q, 4), memcpy(&r.target, q + 1, 4), memcpy(&r.state_state, q + 2, 4);
    r.state_energy = q[3];
    memcpy(&isnew, q + 4, 4);
    r.isNew = isnew != 0;
  }
  LinearizeRequest &lin = w.req.hes.lin;
  lin.frame_ids = c.ids, lin.points = &c.points, lin.fixLinearization = false, lin.wantJacobians = false; // optimize's loop runs linearizeAll(false)
  w.frameEnergyTH = eth;
  w.req.hes.adHost = adh, w.req.hes.adTarget = adt, w.req.hes.shiftPriorToZero = shift != 0;
  for (int i = 0; i < n_pts; i++) {
    const float *q = &pin[(size_t)8 * i];
    w.req.hes.priorF.push_back(q[0]), w.req.hes.Hdd_accLF.push_back(q[2]), w.req.hes.bd_accLF.push_back(q[3]);
    w.req.hes.Hcd_accLF.insert(w.req.hes.Hcd_accLF.end(), q + 4, q + 8);
  }
  w.req.H_L = HL, w.req.b_L = bL, w.req.HM = HM, w.req.bM = bM, w.req.nullBasis = basis, w.req.nullPinv = pinv;
  w.worldToCamEval = ev, w.stateZero = zero, w.exposure = expo, w.prior = prior, w.priorZero = pzero;
  w.state = backup, w.idepth = idb;
  memcpy(w.calibZero, cz.data(), 32), memcpy(w.calib, cb.data(), 32);
  return true;
}

int main(int argc, char **argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: optimize_demo FILE_A FILE_B [MAX_ITERATIONS]\n");
    return 2;
  }
  const int max_its = argc > 3 ? atoi(argv[3]) : 6;
  Case A, B;
  if (!load(argv[1], A) || !load(argv[2], B) || A.wh[0] != B.wh[0] || A.wh[1] != B.wh[1]) {
    fprintf(stderr, "optimize_demo: cannot read the files, or two image sizes\n");
    return 2;
  }
  A.proto.maxIterations = B.proto.maxIterations = max_its;
  // (load() moved nothing: the prototypes point at the points of their cases)
  A.proto.window.req.hes.lin.points = &A.points, B.proto.window.req.hes.lin.points = &B.points;

  dsm_context *ctx = nullptr;
  immature_check(dsm_context_create(0, &ctx), "dsm_context_create");
  Outcome alone_a, alone_b, many_a, many_b, host_a, host_b;
  {
    KeyframeWindow wa(ctx, A.wh[0], A.wh[1], (int)A.nf), wb(ctx, B.wh[0], B.wh[1], (int)B.nf);
    for (size_t k = 0; k < A.nf; k++) wa.put(A.ids[k], &A.planes[k * A.npx]);
    for (size_t k = 0; k < B.nf; k++) wb.put(B.ids[k], &B.planes[k * B.npx]);

    WindowOptimize a = A.proto, b = B.proto;
    a.window.req.hes.lin.window = &wa, b.window.req.hes.lin.window = &wb;
    alone_a = outcome(a, a.optimize(ctx));
    alone_b = outcome(b, b.optimize(ctx));

    WindowOptimize a2 = A.proto, b2 = B.proto; // the windows of two sequences in ONE call
    a2.window.req.hes.lin.window = &wa, b2.window.req.hes.lin.window = &wb;
    std::vector<WindowOptimize *> two = {&a2, &b2};
    std::vector<OptimizeResult> r2 = WindowOptimize::optimizeMany(ctx, two);
    many_a = outcome(a2, r2[0]), many_b = outcome(b2, r2[1]);

    WindowOptimize ha = A.proto, hb = B.proto; // the host form (the request still names a window; the host form does not read it)
    ha.window.req.hes.lin.window = &wa, hb.window.req.hes.lin.window = &wb;
    std::vector<const float *> pa(A.nf), pb(B.nf);
    for (size_t k = 0; k < A.nf; k++) pa[k] = &A.planes[k * A.npx];
    for (size_t k = 0; k < B.nf; k++) pb[k] = &B.planes[k * B.npx];
    host_a = outcome(ha, ha.optimizeHost(A.wh[0], A.wh[1], pa.data()));
    host_b = outcome(hb, hb.optimizeHost(B.wh[0], B.wh[1], pb.data()));
  }
  dsm_context_destroy(ctx);
  auto show = [](const char *name, const Outcome &o) {
    printf("\"%s\": {\"pattern\": \"%s\", \"passes\": %d, \"state\": \"%016llx\", \"calib\": \"%016llx\", \"idepth\": \"%016llx\", \"energy\": \"%016llx\", "
           "\"last\": %.17g}, ",
           name, o.pattern.c_str(), o.passes, (unsigned long long)o.state, (unsigned long long)o.calib, (unsigned long long)o.idepth,
           (unsigned long long)o.energy, o.last);
  };
  const int windows_equal = many_a == alone_a && many_b == alone_b, differ = many_a.pattern != many_b.pattern;
  printf("{");
  show("device_a", alone_a), show("device_b", alone_b), show("many_a", many_a), show("many_b", many_b), show("host_a", host_a), show("host_b", host_b);
  printf("\"windows_equal\": %d, \"decide_differently\": %d, \"device_equals_host\": %d}\n", windows_equal, differ,
         (int)(alone_a == host_a && alone_b == host_b));
  return windows_equal && differ ? 0 : 1;
}
