// marginalize_math.hpp -- marginalising points and frames as DESIGN.md section 21 states it: a point's verdict (C), a residual's
// res_toZeroF (X1), the fold into the prior (M2) and the element operations of one frame's scaled Schur complement (G3-G7).  The
// device kernels (marginalize_kernels.hip) and the host form (marginalize_host.cpp) share them, so that both evaluate one expression
// tree; each keeps its own way of walking residuals, entries and frames in the stated order.  IEEE float and double, left to right as
// written, no contraction (-ffp-contract=off), no fma.  Operands are picked by address from memory or LDS.
#pragma once

#include <cmath>

#include "solve_math.hpp"

namespace dsm {
namespace mrg {

enum { KEEP = 0, MARGINALIZE = 1, DROP = 2 }; // the verdicts, as dsm_activate_points_batch has them

// C: integers and compares only.  k residuals of the point, `vis` of them IN and against a flagged frame
DSM_HD int verdict(float idepth_scaled, int k, int vis, int n_good, int last0, int last1, bool host_flagged, float idepth_hessian,
                   int min_good_active, int min_good_res, float min_idepth_h) {
  if (idepth_scaled < 0.0f || k == 0) return DROP; // C1
  const bool oob = (k >= min_good_active && n_good > min_good_res + 10 && k - vis < min_good_active) || last0 == lin::RES_OOB ||
                   (k >= 2 && last0 == lin::RES_OUTLIER && last1 == lin::RES_OUTLIER); // C2
  if (!(oob || host_flagged)) return KEEP;
  if (!(k >= min_good_active && n_good >= min_good_res)) return DROP; // C3
  return idepth_hessian > min_idepth_h ? MARGINALIZE : DROP;         // C4
}

// X1: rtz[0..8) of an active residual from its row (L8), the pair's adHTdeltaF dp[8], cDeltaF cd[4] and the point's deltaF.
// rtz may be the row's own resF.
DSM_HD void res_to_zero(const float *row, const float *dp, const float *cd, float delta, float *rtz) {
  float j[2];
  for (int a = 0; a < 2; a++) {
    float sx = 0.0f, sc = 0.0f;
    for (int k = 0; k < 6; k++) sx += row[lin::J_PDXI + 6 * a + k] * dp[k];
    for (int c = 0; c < 4; c++) sc += row[lin::J_PDC + 4 * a + c] * cd[c];
    j[a] = (sx + sc) + row[lin::J_PDD + a] * delta;
  }
  const float ta = dp[6], tb = dp[7];
  for (int i = 0; i < 8; i++)
    rtz[i] = (((row[lin::J_RESF + i] - row[lin::J_IDX + i] * j[0]) - row[lin::J_IDX + 8 + i] * j[1]) - row[lin::J_ABF + i] * ta) -
             row[lin::J_ABF + 8 + i] * tb;
}

// M2
DSM_HD double fold(double m, double w, double a, double sc) { return m + w * (a - sc); }

// G1: where row / column i of the permuted system stands in the system before: frame f (8 entries from 4 + 8 f) moves to the end
DSM_HD int source_index(int i, int f, int N) {
  const int nd = N - 8, at = 4 + 8 * f;
  return i >= nd ? at + (i - nd) : i < at ? i : i + 8;
}
// G3
DSM_HD double scale_of(double h_diagonal) { return sqrt(fabs(h_diagonal) + 10.0); }
DSM_HD double scale_inverse(double s) { return 1.0 / s; }
// G4, G7: (l * h) * r
DSM_HD double scaled(double l, double h, double r) { return (l * h) * r; }

// G5: P (8 x 8, row-major) = the inverse of a (8 x 8, row-major, overwritten with its LU factors) by LU with row partial pivoting:
// the pivot is the first maximum of |entry| in the column among the rows not yet eliminated (a comparison with a NaN is false), the
// multiplier a[i][k] / a[k][k], the updates a[i][j] - m a[k][j]; per unit column in ascending order a forward and a backward
// substitution with sums over ascending index from 0.0 and one division per unknown.  piv: 8 ints, y: 8 doubles of room.
// (Upstream then symmetrises the inverse with 0.5f * (hpi + hpi), twice: a matrix added to ITSELF and halved, which is exact and
// changes nothing -- the quirk is not performed.)
DSM_HD void lu_inverse8(double *a, double *P, int *piv, double *y) {
  for (int i = 0; i < 8; i++) piv[i] = i;
  for (int k = 0; k < 8; k++) {
    int big = k;
    double bigv = fabs(a[8 * k + k]);
    for (int i = k + 1; i < 8; i++)
      if (fabs(a[8 * i + k]) > bigv) bigv = fabs(a[8 * i + k]), big = i;
    if (big != k) {
      for (int j = 0; j < 8; j++) {
        const double t = a[8 * k + j];
        a[8 * k + j] = a[8 * big + j], a[8 * big + j] = t;
      }
      const int t = piv[k];
      piv[k] = piv[big], piv[big] = t;
    }
    for (int i = k + 1; i < 8; i++) {
      const double m = a[8 * i + k] / a[8 * k + k];
      a[8 * i + k] = m;
      for (int j = k + 1; j < 8; j++) a[8 * i + j] = a[8 * i + j] - m * a[8 * k + j];
    }
  }
  for (int c = 0; c < 8; c++) {
    for (int i = 0; i < 8; i++) { // L y = the permuted unit column
      double s = 0.0;
      for (int j = 0; j < i; j++) s += a[8 * i + j] * y[j];
      y[i] = (piv[i] == c ? 1.0 : 0.0) - s;
    }
    for (int i = 7; i >= 0; i--) { // U x = y
      double s = 0.0;
      for (int j = i + 1; j < 8; j++) s += a[8 * i + j] * P[8 * j + c];
      P[8 * i + c] = (y[i] - s) / a[8 * i + i];
    }
  }
}

// G6: bli[i][k] from column i of the bottom rows of Hs (stride ld) and column k of P; then one entry of the Schur complement from
// row i of bli and a column of the bottom rows (or the bottom of bs, stride 1)
DSM_HD double bli_entry(const double *bottom_col_i, int ld, const double *P_col_k) {
  double s = 0.0;
  for (int j = 0; j < 8; j++) s += bottom_col_i[(long long)j * ld] * P_col_k[8 * j];
  return s;
}
DSM_HD double schur_entry(double h, const double *bli_row, const double *bottom_col, int ld) {
  double s = 0.0;
  for (int k = 0; k < 8; k++) s += bli_row[k] * bottom_col[(long long)k * ld];
  return h - s;
}
// G7
DSM_HD double symmetrised(double hu_ij, double hu_ji) { return 0.5 * (hu_ij + hu_ji); }

} // namespace mrg
} // namespace dsm
