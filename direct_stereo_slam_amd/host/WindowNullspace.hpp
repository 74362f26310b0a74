// WindowNullspace.hpp -- C++ host adaptor with the shape of FrontEnd::getNullspaces (dso_helpers/FrontEndOptimize.cpp:525-574, which
// solveSystem calls before every solve, :488-494) plus the basis of EnergyFunctional::orthogonalize: from the frames' evaluation poses
// the nine vectors, the normalised basis N of the pose and scale vectors and its pseudo-inverse, for one window or for the windows of
// many sequences in ONE call, on top of the C ABI (include/dsm_hotpath.h).  Header-only, plain C++11.  Semantics: DESIGN.md section 23
// (G1-G7).
//
//   WindowNullspace ns;  ns.worldToCamEval = finish.worldToCamEval; ns.stateZero = ...; ns.exposure = ...;
//   ns.compute(ctx);                                   // after every setEvalPT
//   ns.applyTo(solveRequest);                          // nullBasis / nullPinv of host/WindowSolve.hpp: rule F7 projects with them
#pragma once
#include <stdexcept>
#include <vector>

#include "WindowSolve.hpp"

namespace dsm_host {

class WindowNullspace {
public:
  // what the call reads
  std::vector<double> worldToCamEval; // n x 7: {qx, qy, qz, qw, tx, ty, tz}
  std::vector<double> stateZero;      // n x 8
  std::vector<float> exposure;        // n
  std::vector<double> frameNullIn;    // empty, or n x 42: the frames' nullspaces_pose (columns 0-5) and nullspaces_scale (6), used as they are
  // what it returns
  std::vector<double> nullBasis;      // N x 7
  std::vector<double> nullPinv;       // 7 x N
  std::vector<double> frameNull;      // n x 42
  std::vector<double> nullspacesX0Pre; // N x 9: getNullspaces' return value (pose 0-5, affA, affB, scale)
  double singularValues[7] = {0, 0, 0, 0, 0, 0, 0};
  int rank = 0, flags = 0;

  size_t frames() const { return exposure.size(); }
  // getNullspaces' four output lists, as columns of nullspacesX0Pre
  std::vector<double> column(int c) const {
    const size_t N = 4 + 8 * frames();
    std::vector<double> v(N);
    for (size_t i = 0; i < N; i++) v[i] = nullspacesX0Pre[9 * i + c];
    return v;
  }
  std::vector<double> nullspacePose(int i) const { return column(i); }
  std::vector<double> nullspaceAffA() const { return column(6); }
  std::vector<double> nullspaceAffB() const { return column(7); }
  std::vector<double> nullspaceScale() const { return column(8); }

  void compute(dsm_context *ctx, const dsm_nullspace_params *params = nullptr) {
    std::vector<WindowNullspace *> one(1, this);
    computeMany(ctx, one, params);
  }
  // ... for the windows of many sequences in ONE call
  static void computeMany(dsm_context *ctx, const std::vector<WindowNullspace *> &ws, const dsm_nullspace_params *params = nullptr) {
    std::vector<dsm_nullspace_job> jobs(ws.size());
    for (size_t i = 0; i < ws.size(); i++) jobs[i] = ws[i]->fill();
    immature_check(dsm_window_nullspace_batch(ctx, (int)jobs.size(), jobs.data(), params), "WindowNullspace::compute");
  }
  // ... and through the host form (no device)
  void computeHost(const dsm_nullspace_params *params = nullptr) {
    dsm_nullspace_job job = fill();
    immature_check(dsm_window_nullspace_host(1, &job, params), "WindowNullspace::computeHost");
  }
  // the basis and its pseudo-inverse into a solve request (SOLVER_ORTHOGONALIZE_X_LATER: rule F7)
  void applyTo(SolveRequest &req) const { req.nullBasis = nullBasis, req.nullPinv = nullPinv; }

private:
  dsm_nullspace_job fill() {
    const size_t n = frames(), N = 4 + 8 * n;
    if (worldToCamEval.size() != 7 * n || stateZero.size() != 8 * n || (!frameNullIn.empty() && frameNullIn.size() != 42 * n))
      throw std::invalid_argument("WindowNullspace: an array of the wrong length");
    nullBasis.assign(7 * N, 0.0), nullPinv.assign(7 * N, 0.0), frameNull.assign(42 * n, 0.0), nullspacesX0Pre.assign(9 * N, 0.0);
    dsm_nullspace_job j;
    memset(&j, 0, sizeof j);
    j.n_frames = (int)n;
    j.world_to_cam_eval = worldToCamEval.data(), j.state_zero = stateZero.data(), j.exposure = exposure.data();
    j.frame_null_in = frameNullIn.empty() ? nullptr : frameNullIn.data();
    j.null_basis = nullBasis.data(), j.null_pinv = nullPinv.data(), j.sing = singularValues, j.rank = &rank, j.flags = &flags;
    j.frame_null_out = frameNull.data(), j.null_x0_pre = nullspacesX0Pre.data();
    return j;
  }
};

} // namespace dsm_host
