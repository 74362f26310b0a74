// solve_host.cpp -- the host form of the window optimisation's solve (dsm_window_solve_host) and the job rules
// both forms share (V).  The host form is dsm_window_hessian_host, then plain loops over F1-R3; the expressions are solve_math.hpp,
// shared with the device kernels (solve_kernels.hip), which must equal it bit for bit.  Plain C++; no device code.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "dsm_internal.hpp"
#include "solve_math.hpp"

namespace dsm {

// V of DESIGN.md section 18, after linearize_job_error and hessian_job_error(J.hes, false) have passed
const char *solve_job_error(const dsm_solve_job &J) {
  const size_t N = 4 + 8 * (size_t)J.hes.lin.n_frames;
  if (!J.H_L || !J.b_L) return "NULL H_L or b_L";
  if (!J.x || !J.step || !J.flags) return "NULL x, step or flags";
  if (!std::isfinite(J.lambda) || J.lambda <= -1.0) return "lambda is not finite or <= -1";
  if (J.n_null < 0 || J.n_null > DSM_SOLVE_MAX_NULL) return "n_null outside 0..8";
  if (J.n_null > 0 && (!J.null_basis || !J.null_pinv)) return "n_null > 0 with a NULL null_basis or null_pinv";
  auto finite = [](const double *a, size_t n) {
    for (size_t i = 0; a && i < n; i++)
      if (!std::isfinite(a[i])) return false;
    return true;
  };
  if (!finite(J.H_L, N * N) || !finite(J.b_L, N)) return "a non-finite H_L or b_L";
  if (!finite(J.H_M, N * N) || !finite(J.b_M, N) || !finite(J.delta_x, N)) return "a non-finite H_M, b_M or delta_x";
  if (J.n_null > 0 && (!finite(J.null_basis, N * J.n_null) || !finite(J.null_pinv, N * J.n_null))) return "a non-finite null_basis or null_pinv";
  return nullptr;
}

} // namespace dsm

extern "C" int dsm_window_solve_host(int w, int h, const dsm_solve_job *job, const float *const *frame_I, const dsm_linearize_params *params) {
  using namespace dsm;
  auto fail = [](const char *msg) {
    set_error(std::string("dsm_window_solve_host: ") + msg);
    return DSM_ERR_INVALID;
  };
  if (w < 8 || h < 8 || !job || !frame_I) return fail("bad argument");
  if (const char *e = linearize_params_error(params)) return fail(e);
  if (const char *e = linearize_job_error(job->hes.lin)) return fail(e);
  if (const char *e = hessian_job_error(job->hes, false)) return fail(e);
  if (const char *e = solve_job_error(*job)) return fail(e);
  const dsm_solve_job &J = *job;
  const int nf = J.hes.lin.n_frames, np = J.hes.lin.n_pts, nr = J.hes.lin.n_res, N = 4 + 8 * nf;
  // section 17's host form, with room of our own for what the job does not ask for
  dsm_hessian_job H = J.hes;
  std::vector<double> HA, bA, HS, bS;
  std::vector<float> hdi, bd_sum, hcd_acc, jp;
  std::vector<unsigned char> active;
  if (!H.H_A) HA.resize((size_t)N * N), H.H_A = HA.data();
  if (!H.b_A) bA.resize(N), H.b_A = bA.data();
  if (!H.H_sc) HS.resize((size_t)N * N), H.H_sc = HS.data();
  if (!H.b_sc) bS.resize(N), H.b_sc = bS.data();
  if (!H.hdi) hdi.resize((size_t)np + 1), H.hdi = hdi.data();
  if (!H.bd_sum) bd_sum.resize((size_t)np + 1), H.bd_sum = bd_sum.data();
  if (!H.hcd_acc) hcd_acc.resize(4 * (size_t)np + 1), H.hcd_acc = hcd_acc.data();
  if (!H.JpJdF) jp.resize(8 * (size_t)nr + 1), H.JpJdF = jp.data();
  if (!H.active) active.resize((size_t)nr + 1), H.active = active.data();
  if (int rc = dsm_window_hessian_host(w, h, &H, frame_I, params)) return rc;

  std::vector<double> A((size_t)N * N), P((size_t)N * N), bF(N), v(N), av(N), y(N), temp(N), x(N);
  std::vector<int> ix(N);
  const double lam1 = 1.0 + J.lambda, s = 1.0 / lam1;
  for (int i = 0; i < N; i++) { // F1, F2, F3
    const double top = sol::prior_top(J.H_M ? J.H_M + (size_t)i * N : nullptr, J.b_M, J.delta_x, i, N);
    bF[i] = sol::bf_entry(J.b_L[i], top, H.b_A[i], H.b_sc[i]);
    if (J.last_bS) J.last_bS[i] = bF[i];
    for (int j = 0; j < N; j++) {
      const size_t e = (size_t)i * N + j;
      const double hf = sol::hf_entry(J.H_L[e], J.H_M ? J.H_M[e] : 0.0, H.H_A[e]);
      if (J.last_HS) J.last_HS[e] = hf - H.H_sc[e];
      A[e] = sol::damped(hf, H.H_sc[e], i == j, lam1, s); // F4
    }
  }
  for (int i = 0; i < N; i++) v[i] = sol::scale_of(A[(size_t)i * N + i]); // F5
  for (int i = 0; i < N; i++)
    for (int j = 0; j < N; j++) A[(size_t)i * N + j] = sol::scaled(v[i], A[(size_t)i * N + j], v[j]);
  for (int i = 0; i < N; i++) av[i] = fabs(A[(size_t)i * N + i]); // F6
  sol::pivot_order(av.data(), ix.data(), N);
  for (int i = 0; i < N; i++) {
    for (int j = 0; j <= i; j++) {
      const int hi = ix[i] > ix[j] ? ix[i] : ix[j], lo = ix[i] > ix[j] ? ix[j] : ix[i];
      P[(size_t)i * N + j] = A[(size_t)hi * N + lo];
    }
    y[i] = v[ix[i]] * bF[ix[i]];
  }
  sol::ldlt_solve_permuted(P.data(), N, y.data(), temp.data());
  for (int i = 0; i < N; i++) x[ix[i]] = v[ix[i]] * y[i];
  if (J.n_null > 0) { // F7
    double t[DSM_SOLVE_MAX_NULL];
    for (int k = 0; k < J.n_null; k++) {
      double a = 0.0;
      for (int i = 0; i < N; i++) a += J.null_pinv[(size_t)k * N + i] * x[i];
      t[k] = a;
    }
    for (int i = 0; i < N; i++) {
      double a = 0.0;
      for (int k = 0; k < J.n_null; k++) a += J.null_basis[(size_t)i * J.n_null + k] * t[k];
      x[i] = x[i] - a;
    }
  }
  int flags = 0;
  for (int i = 0; i < N; i++) {
    J.x[i] = x[i];
    if (!std::isfinite(x[i])) flags |= DSM_SOLVE_X_NOT_FINITE;
  }
  std::vector<float> xad((size_t)nf * nf * 8, 0.0f); // R1
  for (int hh = 0; hh < nf; hh++)
    for (int t = 0; t < nf; t++)
      for (int c = 0; t != hh && c < 8; c++) {
        const size_t pr = (size_t)hh * nf + t;
        xad[pr * 8 + c] = sol::x_ad(x.data(), hh, t, J.hes.ad_host + pr * 64, J.hes.ad_target + pr * 64, c);
      }
  const dsm_linearize_job &L = J.hes.lin;
  std::vector<float> b((size_t)np);
  std::vector<unsigned char> has((size_t)np, 0);
  for (int p = 0; p < np; p++) { // R2: the residuals in ascending index
    float hcd[4];
    for (int c = 0; c < 4; c++) hcd[c] = H.hcd_acc[4 * p + c] + (H.hcd_lin ? H.hcd_lin[4 * p + c] : 0.0f);
    b[p] = sol::step_begin(H.bd_sum[p], x.data(), hcd);
  }
  for (int r = 0; r < nr; r++) {
    if (!H.active[r]) continue;
    const int p = L.point[r];
    has[p] = 1;
    b[p] = sol::step_residual(b[p], xad.data() + ((size_t)L.host[p] * nf + L.target[r]) * 8, H.JpJdF + (size_t)8 * r);
  }
  for (int p = 0; p < np; p++) {
    const float st = has[p] ? sol::step_end(b[p], H.hdi[p]) : 0.0f;
    J.step[p] = st;
    if (!std::isfinite(st)) flags |= DSM_SOLVE_STEP_NOT_FINITE; // R3
  }
  *J.flags = flags;
  return DSM_OK;
}
