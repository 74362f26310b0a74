// solve_demo.cpp -- one trial step of FrontEnd::optimize (dso_helpers/FrontEndOptimize.cpp:332-486) through the C++ adaptor
// host/WindowSolve.hpp, on a window read from a file: one window, then the same window twice in one call of the many-window form,
// then through the host form dsm_window_solve_host; all three must agree.
// Input file: a solve file (window_case.hpp, kind SOLVE).
// Usage: solve_demo FILE.  Prints one JSON line: the FNV-1a hashes of lastX, of the points' steps, of lastHS and lastbS, the step of
// the calibration as four doubles' bits hashed, the two finite flags, and whether the three forms agreed; exit status 0 when they did.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "window_case_requests.hpp"

using namespace dsm_host;
using window_case::fnv1a;
using window_case::vhash;

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
  window_case::Case c;
  if (!window_case::read_case(argv[1], window_case::SOLVE, c)) {
    fprintf(stderr, "solve_demo: cannot read %s\n", argv[1]);
    return 2;
  }
  const std::vector<ActivePointData> points = window_case::points(c);
  const std::vector<ActiveResidualData> residuals = window_case::residuals(c);
  const int n_res = (int)c.nr;

  dsm_context *ctx = nullptr;
  immature_check(dsm_context_create(0, &ctx), "dsm_context_create");
  int forms_equal = 0;
  SolveRequest res;
  {
    KeyframeWindow window(ctx, c.w, c.h, (int)c.nf), window2(ctx, c.w, c.h, (int)c.nf);
    window_case::put_planes(c, window), window_case::put_planes(c, window2, true);
    SolveRequest req;
    window_case::fill(req, c);
    req.hes.lin.window = &window, req.hes.lin.points = &points, req.hes.lin.residuals = &residuals;
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
    immature_check(dsm_window_solve_host(c.w, c.h, &job, c.planes, &params), "dsm_window_solve_host");
    solve_detail::unpack(flat, req);
    forms_equal = forms_equal && same(req, res);
  }
  dsm_context_destroy(ctx);

  double step_c[4];
  res.stepC(step_c);
  printf("{\"n_res\": %d, \"x\": \"%016llx\", \"step\": \"%016llx\", \"last_HS\": \"%016llx\", \"last_bS\": \"%016llx\", \"step_c\": \"%016llx\", "
         "\"x_finite\": %d, \"steps_finite\": %d, \"forms_equal\": %d}\n",
         n_res, (unsigned long long)vhash(res.lastX), (unsigned long long)vhash(res.pointStep), (unsigned long long)vhash(res.lastHS),
         (unsigned long long)vhash(res.lastbS), (unsigned long long)fnv1a(step_c, sizeof step_c), (int)res.xFinite, (int)res.stepsFinite, forms_equal);
  return forms_equal ? 0 : 1;
}
