// solve_math.hpp -- the solve and the back-substitution of the window optimisation as DESIGN.md section 18 states them: the entries of
// the stitch's small products (T1d), the prior and accumulated systems put together (F1, F2), damping (F4), scaling (F5), the pivot
// order and the element operations of the LDLT (F6), the projection (F7) and a point's step (R1, R2).  The device kernels
// (solve_kernels.hip) and the host form (solve_host.cpp) share them, so that both evaluate one expression tree; each keeps its own
// way of walking rows, lanes and points in the stated order.  IEEE double and float, left to right as written, no contraction
// (-ffp-contract=off), no fma.
#pragma once

#include <cmath>

#include "hessian_math.hpp"

namespace dsm {
namespace sol {

constexpr int kMaxN = 4 + 8 * 16; // N of a window of DSM_WINDOW_MAX_FRAMES frames
constexpr int kMaxNull = 8;

// T1d: one entry of a small product, the double sum over the ascending inner index from 0.0; a and b walk with strides sa and sb
DSM_HD double dot8(const double *a, int sa, const double *b, int sb) {
  double s = 0.0;
  for (int k = 0; k < 8; k++) s += a[k * sa] * b[k * sb];
  return s;
}

// F1: bM_top[i] from row i of H_M (hm_row, b_m, dx: null reads as zeros)
DSM_HD double prior_top(const double *hm_row, const double *b_m, const double *dx, int i, int N) {
  double s = 0.0;
  for (int j = 0; j < N; j++) s += (hm_row ? hm_row[j] : 0.0) * (dx ? dx[j] : 0.0);
  return (b_m ? b_m[i] : 0.0) + s;
}
// F2
DSM_HD double hf_entry(double hl, double hm, double ha) { return (hl + hm) + ha; }
DSM_HD double bf_entry(double bl, double bm_top, double ba, double bsc) { return ((bl + bm_top) + ba) - bsc; }
// F4: lam1 = 1.0 + lambda, s = 1.0 / lam1
DSM_HD double damped(double hf, double hsc, bool diagonal, double lam1, double s) {
  if (diagonal) hf = hf * lam1;
  return hf - hsc * s;
}
// F5
DSM_HD double scale_of(double hf_diagonal) { return 1.0 / sqrt(hf_diagonal + 10.0); }
DSM_HD double scaled(double vi, double hf, double vj) { return (vi * hf) * vj; }

// F6: the pivot order of the unblocked left-looking LDLT, a function of the input diagonal alone: the selection loop as written,
// first maximum of the remaining |diagonal| in its current arrangement swapped to position k (a comparison with a NaN is false).
// av: |diagonal|, overwritten; ix[k]: the unknown that stands at position k afterwards.
DSM_HD void pivot_order(double *av, int *ix, int n) {
  for (int i = 0; i < n; i++) ix[i] = i;
  for (int k = 0; k < n; k++) {
    int big = k;
    double bigv = av[k];
    for (int i = k + 1; i < n; i++)
      if (av[i] > bigv) bigv = av[i], big = i;
    const double tv = av[k];
    const int ti = ix[k];
    av[k] = av[big], ix[k] = ix[big];
    av[big] = tv, ix[big] = ti;
  }
}
// the D^-1 of the solve
DSM_HD double d_inverse(double y, double d) {
  const double tol = 1.0 / 1.7976931348623157e308;
  return fabs(d) > tol ? y / d : 0.0;
}

// F6 as plain loops (host): A is the permuted system P HS P^T (row-major, ld N, lower triangle read and overwritten), y = P r in, the
// solution of the permuted system out.  The device runs the same operations one row per lane.
inline void ldlt_solve_permuted(double *A, int N, double *y, double *temp) {
  bool all_zero = false;
  for (int k = 0; k < N; k++) {
    if (k > 0) {
      for (int j = 0; j < k; j++) temp[j] = A[j * N + j] * A[k * N + j];
      for (int i = k; i < N; i++) {
        double s = 0.0;
        for (int j = 0; j < k; j++) s += A[i * N + j] * temp[j];
        A[i * N + k] -= s;
      }
    }
    const double akk = A[k * N + k];
    const bool valid = fabs(akk) > 0.0;
    if (k == 0 && !valid) {
      all_zero = true;
      break;
    }
    if (valid)
      for (int i = k + 1; i < N; i++) A[i * N + k] /= akk;
  }
  if (all_zero) {
    for (int i = 0; i < N; i++) y[i] = 0.0;
    return;
  }
  for (int i = 0; i < N; i++)
    for (int j = 0; j < i; j++) y[i] -= A[i * N + j] * y[j];
  for (int i = 0; i < N; i++) y[i] = d_inverse(y[i], A[i * N + i]);
  for (int i = N - 1; i >= 0; i--)
    for (int j = i + 1; j < N; j++) y[i] -= A[j * N + i] * y[j];
}

// R1: xAd[h][t][c] from the float steps of the two frames and the pair's adHost / adTarget blocks (8 x 8 doubles, row-major)
DSM_HD float x_ad(const double *x, int h, int t, const double *ad_host, const double *ad_target, int c) {
  float a = 0.0f, b = 0.0f;
  for (int k = 0; k < 8; k++) a += (float)x[4 + 8 * h + k] * (float)ad_host[8 * k + c];
  for (int k = 0; k < 8; k++) b += (float)x[4 + 8 * t + k] * (float)ad_target[8 * k + c];
  return a + b;
}
// R2: the first part of a point's b, from bd_sum and Hcd; then one active residual's share; then the step
DSM_HD float step_begin(float bd_sum, const double *x, const float *hcd) {
  float s = 0.0f;
  for (int c = 0; c < 4; c++) s += (float)x[c] * hcd[c];
  return bd_sum - s;
}
DSM_HD float step_residual(float b, const float *xad, const float *jp) {
  float s = 0.0f;
  for (int c = 0; c < 8; c++) s += xad[c] * jp[c];
  return b - s;
}
DSM_HD float step_end(float b, float hdi) { return -(b * hdi); }

} // namespace sol
} // namespace dsm
