// nullspace_demo.cpp -- what FrontEnd::solveSystem does before a solve (dso_helpers/FrontEndOptimize.cpp:488-494: getNullspaces, :525-574)
// through the C++ adaptor host/WindowNullspace.hpp, on a window read from a file: one window, then two windows (this one and a second
// set of poses) in one call, then the device's basis fed to host/WindowSolve.hpp as rule F7 reads it, then the host form.
// Input file: a nullspace file (window_case.hpp, kind NULLSPACE): a solve file, whose n_null, nullBasis and nullPinv are not used, then
// the poses of two windows.
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
#include "window_case_requests.hpp"

using namespace dsm_host;
using window_case::vhash;

static bool same(const WindowNullspace &a, const WindowNullspace &b) {
  return vhash(a.nullBasis) == vhash(b.nullBasis) && vhash(a.nullPinv) == vhash(b.nullPinv) && a.rank == b.rank && a.flags == b.flags &&
         memcmp(a.singularValues, b.singularValues, sizeof a.singularValues) == 0;
}

int main(int argc, char **argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: nullspace_demo FILE OUT\n");
    return 2;
  }
  window_case::Case c;
  if (!window_case::read_case(argv[1], window_case::NULLSPACE, c)) {
    fprintf(stderr, "nullspace_demo: cannot read %s\n", argv[1]);
    return 2;
  }
  const std::vector<ActivePointData> points = window_case::points(c);
  const std::vector<ActiveResidualData> residuals = window_case::residuals(c);
  WindowNullspace ns, ns2;
  window_case::fill_poses(ns, c, 0), window_case::fill_poses(ns2, c, 1);

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
    KeyframeWindow window(ctx, c.w, c.h, (int)c.nf);
    window_case::put_planes(c, window);
    window_case::fill(req, c);
    req.hes.lin.window = &window, req.hes.lin.points = &points, req.hes.lin.residuals = &residuals;
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
