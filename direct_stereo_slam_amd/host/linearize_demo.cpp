// linearize_demo.cpp -- FrontEnd::linearizeAll (dso_helpers/FrontEndOptimize.cpp:121-179) through the C++ adaptor
// host/ResidualLinearizer.hpp, on a window read from a file: the window's active residuals through linearizeAll for one window, then
// the same window twice in one call of the many-window form, then through the host form dsm_linearize_residuals_host; all three must
// agree.
// Input file: a window file (window_case.hpp, kind WINDOW).
// Usage: linearize_demo FILE.  Prints one JSON line: the new states as a digit string, the FNV-1a hashes of the energies and of the
// Jacobian rows of the residuals that did not end OOB, the bits of the energy sum and of the new threshold, the kept list, the points
// with a new good residual, and whether the three forms agreed; exit status 0 when they did.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "window_case_requests.hpp"

using namespace dsm_host;
using window_case::fnv1a;

static uint64_t row_hash(const LinearizeRequest &r) {
  uint64_t hsh = 1469598103934665603ull;
  for (size_t i = 0; i < r.J.size(); i++)
    if (r.state_NewState[i] != DSM_RES_OOB) {
      hsh = fnv1a(&r.J[i], sizeof(RawResidualJacobian), hsh);
      hsh = fnv1a(&r.centerProjectedTo[3 * i], 12, hsh);
      hsh = fnv1a(&r.projectedTo[16 * i], 64, hsh);
    }
  return hsh;
}

static bool same(const LinearizeRequest &a, const LinearizeRequest &b) {
  return a.state_NewState == b.state_NewState && a.state_NewEnergy.size() == b.state_NewEnergy.size() &&
         !memcmp(a.state_NewEnergy.data(), b.state_NewEnergy.data(), 4 * a.state_NewEnergy.size()) &&
         !memcmp(a.state_NewEnergyWithOutlier.data(), b.state_NewEnergyWithOutlier.data(), 4 * a.state_NewEnergy.size()) &&
         row_hash(a) == row_hash(b) && !memcmp(&a.energy, &b.energy, 8) && !memcmp(&a.newFrameEnergyTH, &b.newFrameEnergyTH, 4) &&
         a.kept == b.kept && a.toRemove == b.toRemove && a.numGoodResiduals == b.numGoodResiduals &&
         !memcmp(a.maxRelBaseline.data(), b.maxRelBaseline.data(), 4 * a.maxRelBaseline.size());
}

int main(int argc, char **argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: linearize_demo FILE\n");
    return 2;
  }
  window_case::Case c;
  if (!window_case::read_case(argv[1], window_case::WINDOW, c)) {
    fprintf(stderr, "linearize_demo: cannot read %s\n", argv[1]);
    return 2;
  }
  const std::vector<ActivePointData> points = window_case::points(c);
  const std::vector<ActiveResidualData> residuals = window_case::residuals(c);
  const int n_res = (int)c.nr;

  dsm_context *ctx = nullptr;
  immature_check(dsm_context_create(0, &ctx), "dsm_context_create");
  int forms_equal = 0;
  LinearizeRequest res;
  {
    KeyframeWindow window(ctx, c.w, c.h, (int)c.nf), window2(ctx, c.w, c.h, (int)c.nf);
    window_case::put_planes(c, window), window_case::put_planes(c, window2, true);
    LinearizeRequest req;
    window_case::fill(req, c);
    req.window = &window, req.points = &points, req.residuals = &residuals;
    linearizeAll(ctx, req); // one window
    res = req;

    std::vector<LinearizeRequest> reqs(2, req); // the windows of two sequences in one call
    reqs[1].window = &window2;
    linearizeAll(ctx, reqs);
    forms_equal = same(reqs[0], res) && same(reqs[1], res);

    // the host form on the same job
    dsm_linearize_params params;
    dsm_linearize_params_default(&params);
    linearize_detail::Flat flat;
    dsm_linearize_job job = linearize_detail::flatten(flat, req);
    immature_check(dsm_linearize_residuals_host(c.w, c.h, &job, c.planes, &params), "dsm_linearize_residuals_host");
    linearize_detail::unpack(flat, req);
    forms_equal = forms_equal && same(req, res);
  }
  dsm_context_destroy(ctx);

  std::string states, kept = "[", goodp = "[";
  for (size_t i = 0; i < res.state_NewState.size(); i++) states += (char)('0' + res.state_NewState[i]);
  for (size_t i = 0; i < res.kept.size(); i++) kept += (i ? ", " : "") + std::to_string(res.kept[i]);
  bool first = true;
  for (size_t p = 0; p < res.numGoodResiduals.size(); p++)
    if (res.numGoodResiduals[p]) {
      uint32_t bits;
      memcpy(&bits, &res.maxRelBaseline[p], 4);
      goodp += std::string(first ? "[" : ", [") + std::to_string(p) + ", " + std::to_string(res.numGoodResiduals[p]) + ", " + std::to_string(bits) + "]";
      first = false;
    }
  kept += "]", goodp += "]";
  uint64_t ebits;
  uint32_t tbits;
  memcpy(&ebits, &res.energy, 8), memcpy(&tbits, &res.newFrameEnergyTH, 4);
  uint64_t eh = fnv1a(res.state_NewEnergy.data(), 4 * res.state_NewEnergy.size());
  eh = fnv1a(res.state_NewEnergyWithOutlier.data(), 4 * res.state_NewEnergyWithOutlier.size(), eh);
  printf("{\"n_res\": %d, \"states\": \"%s\", \"energy_hash\": \"%016llx\", \"row_hash\": \"%016llx\", \"energy_bits\": \"%016llx\", "
         "\"threshold_bits\": \"%08x\", \"kept\": %s, \"good_points\": %s, \"forms_equal\": %d}\n",
         n_res, states.c_str(), (unsigned long long)eh, (unsigned long long)row_hash(res), (unsigned long long)ebits, tbits, kept.c_str(),
         goodp.c_str(), forms_equal);
  return forms_equal ? 0 : 1;
}
