// hessian_demo.cpp -- accumulateAF_MT / accumulateSCF_MT of FrontEnd::optimize (dso_helpers/FrontEndOptimize.cpp:332-486) through
// the C++ adaptor host/WindowHessian.hpp, on a window read from a file: linearisation and accumulation for one window, then the same
// window twice in one call of the many-window form, then through the host form dsm_window_hessian_host; all three must agree.
// Input file: a hessian file (window_case.hpp, kind HESSIAN).
// Usage: hessian_demo FILE.  Prints one JSON line: the new states as a digit string, the active flags as a digit string, the FNV-1a
// hashes of H_A, b_A, H_sc, b_sc, of JpJdF and of (HdiF, bdSumF, idepth_hessian), the bits of the energy sum, and whether the three
// forms agreed; exit status 0 when they did.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "window_case_requests.hpp"

using namespace dsm_host;
using window_case::vhash;

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
  window_case::Case c;
  if (!window_case::read_case(argv[1], window_case::HESSIAN, c)) {
    fprintf(stderr, "hessian_demo: cannot read %s\n", argv[1]);
    return 2;
  }
  const std::vector<ActivePointData> points = window_case::points(c);
  const std::vector<ActiveResidualData> residuals = window_case::residuals(c);
  const int n_res = (int)c.nr;

  dsm_context *ctx = nullptr;
  immature_check(dsm_context_create(0, &ctx), "dsm_context_create");
  int forms_equal = 0;
  HessianRequest res;
  {
    KeyframeWindow window(ctx, c.w, c.h, (int)c.nf), window2(ctx, c.w, c.h, (int)c.nf);
    window_case::put_planes(c, window), window_case::put_planes(c, window2, true);
    HessianRequest req;
    window_case::fill(req, c);
    req.lin.window = &window, req.lin.points = &points, req.lin.residuals = &residuals;
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
    immature_check(dsm_window_hessian_host(c.w, c.h, &job, c.planes, &params), "dsm_window_hessian_host");
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
