// step_demo.cpp -- the loop of FrontEnd::optimize (dso_helpers/FrontEndOptimize.cpp:382-453: lambda 0.1, x 0.25 on an accepted step,
// x 100 on a rejected one, setting_minOptIterations = 1, step size 1) through the C++ adaptor host/WindowStep.hpp, on a window read
// from a file: one window on the device, the same window twice in one call per iteration, and through the host form.
// Input file: a step file (window_case.hpp, kind STEP; tests/_step_ref.py writes the checker's scenes); the file's
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

#include "window_case_requests.hpp"

using namespace dsm_host;
using window_case::fnv1a;
using window_case::vhash;

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
  window_case::Case c;
  if (!window_case::read_case(argv[1], window_case::STEP, c)) {
    fprintf(stderr, "step_demo: cannot read %s\n", argv[1]);
    return 2;
  }
  const std::vector<ActivePointData> points = window_case::points(c);
  const int n_res = (int)c.nr;
  WindowStep proto;
  window_case::fill(proto, c);
  proto.req.hes.lin.points = &points;

  dsm_context *ctx = nullptr;
  immature_check(dsm_context_create(0, &ctx), "dsm_context_create");
  Outcome dev, host;
  int windows_equal = 0, stale_refused = 0;
  {
    KeyframeWindow window(ctx, c.w, c.h, (int)c.nf), window2(ctx, c.w, c.h, (int)c.nf);
    window_case::put_planes(c, window), window_case::put_planes(c, window2, true);
    WindowStep a = proto;
    a.req.hes.lin.window = &window;
    dev = optimize({&a}, max_its, [&](const float *fac5, double lam) { return std::vector<StepResult>(1, a.iterate(ctx, fac5, lam)); })[0];

    WindowStep b = proto, b2 = proto; // the windows of two sequences in one call per iteration
    b.req.hes.lin.window = &window, b2.req.hes.lin.window = &window2;
    std::vector<WindowStep *> two = {&b, &b2};
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
    host = optimize({&h}, max_its, [&](const float *fac5, double lam) {
      return std::vector<StepResult>(1, h.iterateHost(c.w, c.h, c.planes, fac5, lam));
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
