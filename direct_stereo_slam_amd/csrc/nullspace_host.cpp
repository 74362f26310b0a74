// nullspace_host.cpp -- the host form of the window's nullspaces and their pseudo-inverse (dsm_window_nullspace_host, DESIGN.md section
// 23) and the job rules both forms share (V).  FrontEnd::getNullspaces (dso_helpers/FrontEndOptimize.cpp:525-574, called from
// solveSystem :488-494) as plain loops over G1-G7; the expressions are nullspace_math.hpp, shared with the device kernel
// (nullspace_kernels.hip).  Plain C++; no device code.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "dsm_internal.hpp"
#include "nullspace_launch.hpp"

namespace dsm {

const char *nullspace_params_error(const dsm_nullspace_params *p) {
  if (!p) return "no parameters";
  if (p->struct_size != (int)sizeof(dsm_nullspace_params)) return "struct_size is not sizeof(dsm_nullspace_params)";
  const double v[5] = {p->scale_xi_trans, p->scale_xi_rot, p->scale_a, p->scale_b, p->solver_mode_delta};
  for (double x : v)
    if (!std::isfinite(x) || !(x > 0.0)) return "a parameter that is not finite or not positive";
  return nullptr;
}

// V of DESIGN.md section 23
const char *nullspace_job_error(const dsm_nullspace_job &J) {
  if (J.n_frames < 1 || J.n_frames > DSM_WINDOW_MAX_FRAMES) return "n_frames outside [1, 16]";
  if (!J.world_to_cam_eval || !J.state_zero || !J.exposure) return "NULL world_to_cam_eval, state_zero or exposure";
  if (!J.null_basis || !J.null_pinv || !J.sing || !J.rank || !J.flags) return "NULL required output";
  const size_t n = J.n_frames;
  for (size_t i = 0; i < 7 * n; i++)
    if (!std::isfinite(J.world_to_cam_eval[i])) return "a non-finite world_to_cam_eval";
  for (size_t f = 0; f < n; f++) {
    if (!std::isfinite(J.state_zero[8 * f + 6])) return "a non-finite state_zero";
    if (!std::isfinite(J.exposure[f]) || !(J.exposure[f] > 0.0f)) return "an exposure that is not finite or not positive";
    const double *q = J.world_to_cam_eval + 7 * f;
    const double nn = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
    if (!(fabs(nn - 1.0) <= 1e-9)) return "a world_to_cam_eval quaternion that is not of unit length (squared norm within 1e-9 of 1)";
  }
  for (size_t i = 0; J.frame_null_in && i < 42 * n; i++)
    if (!std::isfinite(J.frame_null_in[i])) return "a non-finite frame_null_in";
  return nullptr;
}

int nullspace_check(const char *call, int n_jobs, const dsm_nullspace_job *jobs, const dsm_nullspace_params *params, dsm_nullspace_params &P) {
  auto bad = [call](const char *msg) { return invalid((std::string(call) + ": " + msg).c_str()); };
  if (n_jobs < 1 || !jobs) return bad("bad argument");
  if (params)
    P = *params;
  else
    dsm_nullspace_params_default(&P);
  if (const char *e = nullspace_params_error(&P)) return bad(e);
  for (int j = 0; j < n_jobs; j++)
    if (const char *e = nullspace_job_error(jobs[j])) return bad(e);
  return DSM_OK;
}

nsp::Scales nullspace_scales(const dsm_nullspace_params &P) {
  return nsp::Scales{1.0 / P.scale_xi_trans, 1.0 / P.scale_xi_rot, 1.0 / P.scale_a, 1.0 / P.scale_b, P.solver_mode_delta};
}

namespace {

void nullspace_one(const dsm_nullspace_job &J, const dsm_nullspace_params &P, const nsp::Scales &S, const nsp::UnitPoses &U) {
  using namespace nsp;
  const int n = J.n_frames, N = 4 + 8 * n;
  std::vector<double> fn(42 * (size_t)n);
  if (J.frame_null_in) {
    memcpy(fn.data(), J.frame_null_in, 8 * fn.size());
  } else {
    for (int f = 0; f < n; f++) { // G1, G2
      double lg[kLogs][6];
      for (int c = 0; c < kLogs; c++) frame_log(J.world_to_cam_eval + 7 * f, U, c, lg[c]);
      for (int i = 0; i < kCols; i++)
        for (int r = 0; r < 6; r++) fn[42 * f + r * 7 + i] = null_entry(lg[i < 6 ? i : 12][r], lg[i < 6 ? 6 + i : 13][r]);
    }
  }
  std::vector<double> pre(9 * (size_t)N, 0.0), W(kCols * (size_t)N, 0.0);
  for (int f = 0; f < n; f++) { // G3, G4
    double *rows = &pre[9 * (size_t)(4 + 8 * f)];
    for (int r = 0; r < 6; r++)
      for (int i = 0; i < kCols; i++) rows[9 * r + (i < 6 ? i : 8)] = scaled_entry(fn[42 * f + r * 7 + i], r, S);
    double A[2], B[2];
    affine_rows(affine_b(J.state_zero[8 * f + 6], P.scale_a, J.exposure[f]), S, A, B);
    rows[9 * 6 + 6] = A[0], rows[9 * 7 + 6] = A[1], rows[9 * 6 + 7] = B[0], rows[9 * 7 + 7] = B[1];
  }
  int flags = 0;
  for (int i = 0; i < N; i++)
    for (int k = 0; k < kCols; k++) W[(size_t)i * kCols + k] = pre[9 * (size_t)i + (k < 6 ? k : 8)];
  for (int k = 0; k < kCols; k++) { // G5
    const double s = col_dot(W.data(), N, k, k);
    if (s > 0.0) {
      const double d = sqrt(s);
      for (int i = 0; i < N; i++) W[(size_t)i * kCols + k] = W[(size_t)i * kCols + k] / d;
    } else {
      flags |= DSM_NULLSPACE_UNNORMALISED;
    }
  }
  std::vector<double> basis = W;
  double V[kCols * kCols]; // G6
  for (int i = 0; i < kCols * kCols; i++) V[i] = i % (kCols + 1) == 0 ? 1.0 : 0.0;
  double amax = 0.0;
  for (int k = 0; k < kCols; k++) {
    const double s = col_dot(W.data(), N, k, k);
    if (s > amax) amax = s;
  }
  bool capped = true;
  for (int sweep = 0; sweep < kSweepCap; sweep++) {
    bool rotated = false;
    for (int r = 0; r < kRounds; r++)
      for (int k = 0; k < 3; k++) {
        int p, q;
        round_pair(r, k, p, q);
        const double a = col_dot(W.data(), N, p, p), b = col_dot(W.data(), N, q, q), c = col_dot(W.data(), N, p, q);
        double cs, sn;
        if (!rotation(a, b, c, amax, S.delta, cs, sn)) continue;
        rotated = true;
        for (int i = 0; i < N; i++) rotate(W[(size_t)i * kCols + p], W[(size_t)i * kCols + q], cs, sn);
        for (int i = 0; i < kCols; i++) rotate(V[i * kCols + p], V[i * kCols + q], cs, sn);
      }
    if (!rotated) {
      capped = false;
      break;
    }
  }
  if (capped) flags |= DSM_NULLSPACE_SWEEP_CAP;
  double sing[kCols], inv[kCols];
  for (int k = 0; k < kCols; k++) sing[k] = sqrt(col_dot(W.data(), N, k, k));
  const int rank = kept_inverses(sing, S.delta, inv);
  std::vector<double> pinv(kCols * (size_t)N);
  for (int k = 0; k < kCols; k++)
    for (int i = 0; i < N; i++) pinv[(size_t)k * N + i] = pinv_entry(V + k * kCols, &W[(size_t)i * kCols], inv);
  bool finite = true; // G7
  for (double x : basis) finite = finite && std::isfinite(x);
  for (double x : pinv) finite = finite && std::isfinite(x);
  for (double x : sing) finite = finite && std::isfinite(x);
  if (!finite) flags |= DSM_NULLSPACE_NONFINITE;

  memcpy(J.null_basis, basis.data(), 8 * basis.size()), memcpy(J.null_pinv, pinv.data(), 8 * pinv.size()), memcpy(J.sing, sing, sizeof sing);
  *J.rank = rank, *J.flags = flags;
  if (J.frame_null_out) memcpy(J.frame_null_out, fn.data(), 8 * fn.size());
  if (J.null_x0_pre) memcpy(J.null_x0_pre, pre.data(), 8 * pre.size());
}

} // namespace
} // namespace dsm

extern "C" int dsm_nullspace_params_default(dsm_nullspace_params *p) {
  if (!p) return DSM_ERR_INVALID;
  p->struct_size = (int)sizeof(dsm_nullspace_params);
  p->scale_xi_trans = 0.5, p->scale_xi_rot = 1.0, p->scale_a = 10.0, p->scale_b = 1000.0, p->solver_mode_delta = 1e-5;
  return DSM_OK;
}

extern "C" int dsm_window_nullspace_host(int n_jobs, const dsm_nullspace_job *jobs, const dsm_nullspace_params *params) {
  using namespace dsm;
  dsm_nullspace_params P;
  if (int rc = nullspace_check("dsm_window_nullspace_host", n_jobs, jobs, params, P)) return rc;
  const nsp::Scales S = nullspace_scales(P);
  nsp::UnitPoses U;
  nsp::unit_poses(U);
  for (int j = 0; j < n_jobs; j++) nullspace_one(jobs[j], P, S, U);
  return DSM_OK;
}
