// optimize_demo.cpp -- the loop of FrontEnd::optimize (dso_helpers/FrontEndOptimize.cpp:362-371, :382-453) as ONE call through the C++
// adaptor host/WindowOptimize.hpp, on two windows read from files: window A alone on the device, A and B -- two DIFFERENT windows -- in
// one call, where each takes its own decisions, and both through the host form.
// Input files: step files (window_case.hpp, kind STEP; tests/_step_ref.py writes the checker's scenes); a file's state_backup,
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

#include "window_case_requests.hpp"

using namespace dsm_host;
using window_case::fnv1a;

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

// a window of a step file: the prototype of its WindowOptimize and its points
struct Case {
  window_case::Case file;
  std::vector<ActivePointData> points;
  WindowOptimize proto;
};

static bool load(const char *path, Case &c) {
  if (!window_case::read_case(path, window_case::STEP, c.file)) return false;
  c.points = window_case::points(c.file);
  window_case::fill(c.proto.window, c.file);
  return true;
}

int main(int argc, char **argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: optimize_demo FILE_A FILE_B [MAX_ITERATIONS]\n");
    return 2;
  }
  const int max_its = argc > 3 ? atoi(argv[3]) : 6;
  Case A, B;
  if (!load(argv[1], A) || !load(argv[2], B) || A.file.w != B.file.w || A.file.h != B.file.h) {
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
    KeyframeWindow wa(ctx, A.file.w, A.file.h, (int)A.file.nf), wb(ctx, B.file.w, B.file.h, (int)B.file.nf);
    window_case::put_planes(A.file, wa), window_case::put_planes(B.file, wb);

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
    host_a = outcome(ha, ha.optimizeHost(A.file.w, A.file.h, A.file.planes));
    host_b = outcome(hb, hb.optimizeHost(B.file.w, B.file.h, B.file.planes));
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
