// WindowSolve.hpp -- C++ host adaptor with the shape of EnergyFunctional::solveSystemF: everything FrontEnd::optimize
// (dso_helpers/FrontEndOptimize.cpp:332-486) does for one trial step between backupState and doStepFromBackup -- linearizeAll,
// accumulateAF_MT / accumulateSCF_MT, the stitch, the prior systems, damping, the Schur-reduced solve (non-SVD), orthogonalize on a
// caller-supplied basis and resubstituteF_MT -- as ONE call, for one window or for the windows of many sequences, on top of the C ABI
// (include/dsm_hotpath.h).  Header-only, plain C++11.  Semantics: DESIGN.md section 18 (T1d, F1-F8, R1-R3).
#pragma once
#include "WindowHessian.hpp"

namespace dsm_host {

// One window: the accumulation's request and what solveSystemF reads on top.  N = 4 + 8 n_frames.
struct SolveRequest {
  HessianRequest hes;
  std::vector<double> H_L, b_L;      // accumulateLF_MT after stitchDouble: N * N and N
  std::vector<double> HM, bM;        // the marginalisation prior (empty: zeros)
  std::vector<double> deltaX;        // getStitchedDeltaF (empty: zeros)
  double lambda = 0;                 // after SOLVER_FIX_LAMBDA / SOLVER_USE_GN
  std::vector<double> nullBasis, nullPinv; // N x k and k x N, k <= 8 (empty: no projection)
  bool wantStitched = false;         // also return hes.H_A, b_A, H_sc, b_sc and lastHS, lastbS

  // results
  std::vector<double> lastX;         // N; the steps are -lastX
  std::vector<float> pointStep;      // per point: PointHessian::step (0 for a point without an active residual)
  std::vector<double> lastHS, lastbS; // with wantStitched
  bool xFinite = true, stepsFinite = true; // upstream asserts on these

  // the calibration step and the step of frame h (8 values), as doStepFromBackup reads them
  void stepC(double out[4]) const {
    for (int i = 0; i < 4; i++) out[i] = -lastX[i];
  }
  void stepFrame(size_t h, double out[8]) const {
    for (int i = 0; i < 8; i++) out[i] = -lastX[4 + 8 * h + i];
  }
};

namespace solve_detail {
struct Flat {
  linearize_detail::Flat lin;
  int flags = 0;
};
inline dsm_solve_job flatten(Flat &f, SolveRequest &r) {
  dsm_solve_job j;
  memset(&j, 0, sizeof j);
  j.hes = hessian_detail::flatten(f.lin, r.hes);
  const size_t nf = r.hes.lin.frame_ids.size(), n = r.hes.lin.points->size(), N = 4 + 8 * nf;
  auto sized = [](const std::vector<double> &v, size_t want, bool required) {
    if ((required || !v.empty()) && v.size() != want) throw std::invalid_argument("solveWindow: an array of the wrong length");
    return v.empty() ? nullptr : v.data();
  };
  j.H_L = sized(r.H_L, N * N, true), j.b_L = sized(r.b_L, N, true);
  j.H_M = sized(r.HM, N * N, false), j.b_M = sized(r.bM, N, false), j.delta_x = sized(r.deltaX, N, false);
  j.lambda = r.lambda;
  if (r.nullBasis.size() % N || r.nullBasis.size() != r.nullPinv.size()) throw std::invalid_argument("solveWindow: nullBasis / nullPinv");
  j.n_null = (int)(r.nullBasis.size() / N);
  j.null_basis = j.n_null ? r.nullBasis.data() : nullptr, j.null_pinv = j.n_null ? r.nullPinv.data() : nullptr;
  if (!r.wantStitched) {
    j.hes.H_A = j.hes.b_A = j.hes.H_sc = j.hes.b_sc = nullptr;
    r.hes.H_A.clear(), r.hes.b_A.clear(), r.hes.H_sc.clear(), r.hes.b_sc.clear();
    r.lastHS.clear(), r.lastbS.clear();
  } else {
    r.lastHS.assign(N * N, 0.0), r.lastbS.assign(N, 0.0);
    j.last_HS = r.lastHS.data(), j.last_bS = r.lastbS.data();
  }
  r.lastX.assign(N, 0.0), r.pointStep.assign(n + 1, 0.f);
  j.x = r.lastX.data(), j.step = r.pointStep.data(), j.flags = &f.flags;
  return j;
}
inline void unpack(const Flat &f, SolveRequest &r) {
  hessian_detail::unpack(f.lin, r.hes);
  r.pointStep.pop_back();
  r.xFinite = !(f.flags & DSM_SOLVE_X_NOT_FINITE), r.stepsFinite = !(f.flags & DSM_SOLVE_STEP_NOT_FINITE);
}
} // namespace solve_detail

// one trial step for the windows of many sequences in ONE call; every window must have the same image size.  Fills the results of
// every request.  params: null = the upstream defaults.
inline void solveWindows(dsm_context *ctx, std::vector<SolveRequest> &reqs, const dsm_linearize_params *params = nullptr) {
  if (reqs.empty()) return;
  dsm_linearize_params defaults;
  dsm_linearize_params_default(&defaults);
  std::vector<solve_detail::Flat> flat(reqs.size());
  std::vector<dsm_solve_job> jobs(reqs.size());
  for (size_t i = 0; i < reqs.size(); i++) jobs[i] = solve_detail::flatten(flat[i], reqs[i]);
  immature_check(dsm_window_solve_batch(ctx, (int)jobs.size(), jobs.data(), params ? params : &defaults), "solveWindows");
  for (size_t i = 0; i < reqs.size(); i++) solve_detail::unpack(flat[i], reqs[i]);
}

// ... and for one window
inline void solveWindow(dsm_context *ctx, SolveRequest &req, const dsm_linearize_params *params = nullptr) {
  dsm_linearize_params defaults;
  dsm_linearize_params_default(&defaults);
  solve_detail::Flat flat;
  dsm_solve_job job = solve_detail::flatten(flat, req);
  immature_check(dsm_window_solve_batch(ctx, 1, &job, params ? params : &defaults), "solveWindow");
  solve_detail::unpack(flat, req);
}

} // namespace dsm_host
