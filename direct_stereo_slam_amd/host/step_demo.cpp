// step_demo.cpp -- the loop of FrontEnd::optimize (dso_helpers/FrontEndOptimize.cpp:382-453: lambda 0.1, x 0.25 on an accepted step,
// x 100 on a rejected one, setting_minOptIterations = 1, step size 1) through the C++ adaptor host/WindowStep.hpp, on a window read
// from a file: one window on the device, the same window twice in one call per iteration, and through the host form.
// Input file (native byte order): the step file tools/step_host_standalone.cpp reads (tests/_step_ref.py, write_case); the file's
// state_backup, calib_backup and idepth_backup are the state the loop starts from, its step and factors are not used.
// Usage: step_demo FILE [MAX_ITERATIONS = 6].  Prints one JSON line: per form the accept / reject pattern, the FNV-1a hashes of the
// final state, calibration and inverse depths and of the last energy, and that energy; whether the two windows of one call equalled the
// single window, and whether the device equalled the host form (its sincos and exp may differ in the last place: reported, not
// required); and how often an iterate with non-zero factors was refused while the step was void (before the first accept, after a
// reject: 2).  Exit status 0 when the two windows equalled the single one and both were refused.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "WindowStep.hpp"

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

struct Outcome {
  std::string pattern; // A / R per iteration
  uint64_t state = 0, calib = 0, idepth = 0, energy = 0;
  double last = 0; // the last energy itself
  bool operator==(const Outcome &o) const { return pattern == o.pattern && state == o.state && calib == o.calib && idepth == o.idepth && energy == o.energy; }
};

// the loop; `call` runs one iteration on every window of ws and returns their results
template <typename Call>
static std::vector<Outcome> optimize(std::vector<WindowStep *> ws, int max_its, Call call) {
  const float zero[5] = {0, 0, 0, 0, 0}, one[5] = {1, 1, 1, 1, 1};
  std::vector<Outcome> out(ws.size());
  double lambda = 1e-1;
  for (WindowStep *w : ws) w->backupState();
  std::vector<StepResult> r = call(zero, lambda); // linearizeAll and applyRes before the loop (:362-371), and solveSystem(0, lambda)
  std::vector<double> last(ws.size());
  for (size_t i = 0; i < ws.size(); i++) ws[i]->accept(), last[i] = r[i].energy + r[i].energyM;
  for (int it = 0; it < max_its; it++) {
    for (WindowStep *w : ws) w->backupState();
    r = call(one, lambda * 0.25); // the trial, and the next solve as if it were accepted
    // the windows of the demo are copies of one window: one decision serves all
    const bool accepted = r[0].energy + r[0].energyM < last[0];
    if (accepted) {
      for (size_t i = 0; i < ws.size(); i++) ws[i]->accept(), last[i] = r[i].energy + r[i].energyM;
      lambda *= 0.25;
    } else {
      lambda *= 1e2;
      for (WindowStep *w : ws) w->reject();
      std::vector<StepResult> b = call(zero, lambda); // loadSateBackup + linearizeAll (:444-448), and the next solve
      for (size_t i = 0; i < ws.size(); i++) ws[i]->accept(), last[i] = b[i].energy + b[i].energyM;
    }
    for (Outcome &o : out) o.pattern += accepted ? 'A' : 'R';
    if (r[0].canBreak && it >= 1) break; // setting_minOptIterations
  }
  for (size_t i = 0; i < ws.size(); i++) {
    out[i].state = vhash(ws[i]->state), out[i].calib = fnv1a(ws[i]->calib, 32), out[i].idepth = vhash(ws[i]->idepth);
    out[i].energy = fnv1a(&last[i], 8), out[i].last = last[i];
  }
  return out;
}

int main(int argc, char **argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: step_demo FILE [MAX_ITERATIONS]\n");
    return 2;
  }
  const int max_its = argc > 2 ? atoi(argv[2]) : 6;
  FILE *f = fopen(argv[1], "rb");
  int wh[2], nff[2] = {0, 0}, n_pts = 0, n_res = 0, shift = 1, n_null = 0, has_hm = 0, has_prior = 0;
  float cal[6];
  double lambda = 0;
  std::vector<int> ids;
  std::vector<float> planes, pre, eth, prec, rrec, pin, idb, ids_step, expo, fac;
  std::vector<double> adh, adt, HL, bL, HM, bM, basis, pinv, ev, zero, backup, fstep, cz, cb, cs, prior, pzero;
  bool good = f && fread(wh, sizeof(int), 2, f) == 2 && fread(cal, sizeof(float), 6, f) == 6 && fread(nff, sizeof(int), 2, f) == 2 &&
              nff[0] >= 1 && nff[0] <= DSM_WINDOW_MAX_FRAMES && wh[0] > 0 && wh[1] > 0;
  const size_t nf = good ? nff[0] : 0, npx = good ? (size_t)wh[0] * wh[1] : 0, N = 4 + 8 * nf;
  good = good && rd(f, ids, nf) && rd(f, planes, nf * npx) && rd(f, pre, nf * nf * 27) && rd(f, eth, nf) && fread(&n_pts, sizeof(int), 1, f) == 1 &&
         n_pts >= 0 && rd(f, prec, (size_t)n_pts * 21) && fread(&n_res, sizeof(int), 1, f) == 1 && n_res >= 0 && rd(f, rrec, (size_t)n_res * 5) &&
         rd(f, adh, nf * nf * 64) && rd(f, adt, nf * nf * 64) && rd(f, pin, (size_t)n_pts * 8) && fread(&shift, sizeof(int), 1, f) == 1;
  good = good && rd(f, HL, N * N) && rd(f, bL, N) && fread(&has_hm, sizeof(int), 1, f) == 1 && (!has_hm || (rd(f, HM, N * N) && rd(f, bM, N))) &&
         fread(&lambda, sizeof(double), 1, f) == 1 && fread(&n_null, sizeof(int), 1, f) == 1 && n_null >= 0 && n_null <= DSM_SOLVE_MAX_NULL &&
         rd(f, basis, N * n_null) && rd(f, pinv, N * n_null);
  good = good && rd(f, ev, 7 * nf) && rd(f, zero, 8 * nf) && rd(f, backup, 8 * nf) && rd(f, fstep, 8 * nf) && rd(f, cz, 4) && rd(f, cb, 4) && rd(f, cs, 4) &&
         rd(f, idb, n_pts) && rd(f, ids_step, n_pts) && rd(f, expo, nf) && rd(f, fac, 5) && fread(&has_prior, sizeof(int), 1, f) == 1 &&
         (!has_prior || (rd(f, prior, N) && rd(f, pzero, N)));
  if (!good) {
    fprintf(stderr, "step_demo: cannot read %s\n", argv[1]);
    return 2;
  }
  fclose(f);
  std::vector<ActivePointData> points(n_pts);
  for (int i = 0; i < n_pts; i++) {
    const float *q = &prec[(size_t)21 * i];
    memcpy(&points[i].host, q, 4);
    points[i].u = q[1], points[i].v = q[2], points[i].idepth_scaled = 0, points[i].idepth_zero_scaled = 0;
    memcpy(points[i].color, q + 5, 32);
    memcpy(points[i].weights, q + 13, 32);
  }
  WindowStep proto;
  proto.residuals.resize(n_res);
  for (int i = 0; i < n_res; i++) {
    const float *q = &rrec[(size_t)5 * i];
    int isnew;
    ActiveResidualData &r = proto.residuals[i];
    memcpy(&r.point, q, 4), memcpy(&r.target, q + 1, 4), memcpy(&r.state_state, q + 2, 4);
    r.state_energy = q[3];
    memcpy(&isnew, q + 4, 4);
    r.isNew = isnew != 0;
  }
  LinearizeRequest &lin = proto.req.hes.lin;
  lin.frame_ids = ids, lin.points = &points, lin.fixLinearization = false, lin.wantJacobians = false; // optimize's loop runs linearizeAll(false)
  proto.frameEnergyTH = eth;
  proto.req.hes.adHost = adh, proto.req.hes.adTarget = adt, proto.req.hes.shiftPriorToZero = shift != 0;
  for (int i = 0; i < n_pts; i++) {
    const float *q = &pin[(size_t)8 * i];
    proto.req.hes.priorF.push_back(q[0]), proto.req.hes.Hdd_accLF.push_back(q[2]), proto.req.hes.bd_accLF.push_back(q[3]);
    proto.req.hes.Hcd_accLF.insert(proto.req.hes.Hcd_accLF.end(), q + 4, q + 8);
  }
  proto.req.H_L = HL, proto.req.b_L = bL, proto.req.HM = HM, proto.req.bM = bM, proto.req.nullBasis = basis, proto.req.nullPinv = pinv;
  proto.worldToCamEval = ev, proto.stateZero = zero, proto.exposure = expo, proto.prior = prior, proto.priorZero = pzero;
  proto.state = backup, proto.idepth = idb;
  memcpy(proto.calibZero, cz.data(), 32), memcpy(proto.calib, cb.data(), 32);

  dsm_context *ctx = nullptr;
  immature_check(dsm_context_create(0, &ctx), "dsm_context_create");
  Outcome dev, host;
  int windows_equal = 0, stale_refused = 0;
  {
    KeyframeWindow window(ctx, wh[0], wh[1], (int)nf), window2(ctx, wh[0], wh[1], (int)nf);
    for (size_t k = 0; k < nf; k++) {
      window.put(ids[k], &planes[k * npx]);
      window2.put(ids[nf - 1 - k], &planes[(nf - 1 - k) * npx]); // (the store's order is not the window's)
    }
    WindowStep a = proto;
    a.req.hes.lin.window = &window;
    dev = optimize({&a}, max_its, [&](const float *fac5, double lam) { return std::vector<StepResult>(1, a.iterate(ctx, fac5, lam)); })[0];

    WindowStep b = proto, c = proto; // the windows of two sequences in one call per iteration
    b.req.hes.lin.window = &window, c.req.hes.lin.window = &window2;
    std::vector<WindowStep *> two = {&b, &c};
    std::vector<Outcome> o2 = optimize(two, max_its, [&](const float *fac5, double lam) { return WindowStep::iterateMany(ctx, two, fac5, lam); });
    windows_equal = o2[0] == dev && o2[1] == dev;

    WindowStep g = proto; // a step that is void is refused: before the first accept, and after a reject
    g.req.hes.lin.window = &window;
    const float zero5[5] = {0, 0, 0, 0, 0}, one5[5] = {1, 1, 1, 1, 1};
    for (int after_reject = 0; after_reject < 2; after_reject++) {
      if (after_reject) g.iterate(ctx, zero5, 1e-1), g.accept(), g.backupState(), g.iterate(ctx, one5, 1e-1), g.reject();
      try {
        g.iterate(ctx, one5, 1e-1);
      } catch (const std::logic_error &) {
        stale_refused++;
      }
    }

    WindowStep h = proto; // the host form
    h.req.hes.lin.window = &window;
    std::vector<const float *> frame_I(nf);
    for (size_t k = 0; k < nf; k++) frame_I[k] = &planes[k * npx];
    host = optimize({&h}, max_its, [&](const float *fac5, double lam) {
      return std::vector<StepResult>(1, h.iterateHost(wh[0], wh[1], frame_I.data(), fac5, lam));
    })[0];
  }
  dsm_context_destroy(ctx);
  auto show = [](const char *name, const Outcome &o) {
    printf("\"%s\": {\"pattern\": \"%s\", \"state\": \"%016llx\", \"calib\": \"%016llx\", \"idepth\": \"%016llx\", \"energy\": \"%016llx\", "
           "\"last\": %.17g}, ",
           name, o.pattern.c_str(), (unsigned long long)o.state, (unsigned long long)o.calib, (unsigned long long)o.idepth, (unsigned long long)o.energy,
           o.last);
  };
  printf("{\"n_res\": %d, ", n_res);
  show("device", dev), show("host", host);
  printf("\"windows_equal\": %d, \"device_equals_host\": %d, \"stale_step_refused\": %d}\n", windows_equal, (int)(dev == host), stale_refused);
  return windows_equal && stale_refused == 2 ? 0 : 1;
}
