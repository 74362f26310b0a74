// hessian_math.hpp -- the accumulation of the window optimisation as DESIGN.md section 17 states it: what a residual contributes
// (A1-A3), what a point sums and derives (S1, S2) and the Schur terms (S3).  The device kernels (hessian_kernels.hip) and the host
// form (points_host.cpp) share them, so that both evaluate one expression tree; each keeps its own way of walking the residuals in
// the stated order.  Products are float32, left to right as written, no contraction (-ffp-contract=off), no fmaf.
// Operands are picked by address from a record in memory or LDS, never from a register array indexed at run time.
#pragma once

#include "linearize_math.hpp"

namespace dsm {
namespace hes {

// The record of an active residual, written once from its row (A1, A2) and read by every later stage.
//   X, Y      the 10-vectors x = (Jpdc[0], Jpdxi[0]), y = (Jpdc[1], Jpdxi[1])
//   I2        JIdx2_00, _01, _11
//   K         the coefficients of the columns a, b, r of the top right: (JabJIdx_00, _01), (JabJIdx_10, _11), (JI_r[0], JI_r[1])
//   BR        the bottom right 3 x 3, full: [[Jab2_00, Jab2_01, Jab_r[0]], [Jab2_01, Jab2_11, Jab_r[1]], [Jab_r[0], Jab_r[1], rr]]
//   JP        JpJdF[8];  PDD Jpdd[2];  V v0, v1;  ACTIVE an int: A0
enum { R_X = 0, R_Y = 10, R_I2 = 20, R_K = 23, R_BR = 29, R_TOP_END = 38, R_JP = 38, R_PDD = 46, R_V = 48, R_ACTIVE = 50, R_FLOATS = 52 };
// What a point keeps: the S1 sums, then S2's results in the order the Schur stage reads them
enum { P_HDD = 0, P_BD = 1, P_HCD = 2, P_HDI = 6, P_BDSUM = 7, P_IDH = 8, P_HCDSUM = 9, P_NACT = 13, P_FLOATS = 16 };
constexpr int kTop = 13, kTopEntries = 91; // the 13 x 13 term and its upper half

// A1, A2 and the copies: rec[0 .. R_ACTIVE) from a row of L8
DSM_HD void residual_record(const float *row, float *rec) {
  float ji0 = 0.0f, ji1 = 0.0f, ja0 = 0.0f, ja1 = 0.0f, rr = 0.0f;
  for (int i = 0; i < 8; i++) {
    const float r = row[lin::J_RESF + i];
    ji0 += r * row[lin::J_IDX + i], ji1 += r * row[lin::J_IDX + 8 + i];
    ja0 += r * row[lin::J_ABF + i], ja1 += r * row[lin::J_ABF + 8 + i];
    rr += r * r;
  }
  for (int k = 0; k < 4; k++) rec[R_X + k] = row[lin::J_PDC + k], rec[R_Y + k] = row[lin::J_PDC + 4 + k];
  for (int k = 0; k < 6; k++) rec[R_X + 4 + k] = row[lin::J_PDXI + k], rec[R_Y + 4 + k] = row[lin::J_PDXI + 6 + k];
  const float i00 = row[lin::J_IDX2], i01 = row[lin::J_IDX2 + 1], i10 = row[lin::J_IDX2 + 2], i11 = row[lin::J_IDX2 + 3];
  rec[R_I2] = i00, rec[R_I2 + 1] = i01, rec[R_I2 + 2] = i11;
  const float k00 = row[lin::J_ABJIDX], k01 = row[lin::J_ABJIDX + 1], k10 = row[lin::J_ABJIDX + 2], k11 = row[lin::J_ABJIDX + 3];
  rec[R_K] = k00, rec[R_K + 1] = k01, rec[R_K + 2] = k10, rec[R_K + 3] = k11, rec[R_K + 4] = ji0, rec[R_K + 5] = ji1;
  const float b00 = row[lin::J_AB2], b01 = row[lin::J_AB2 + 1], b11 = row[lin::J_AB2 + 3];
  rec[R_BR] = b00, rec[R_BR + 1] = b01, rec[R_BR + 2] = ja0;
  rec[R_BR + 3] = b01, rec[R_BR + 4] = b11, rec[R_BR + 5] = ja1;
  rec[R_BR + 6] = ja0, rec[R_BR + 7] = ja1, rec[R_BR + 8] = rr;
  const float d0 = row[lin::J_PDD], d1 = row[lin::J_PDD + 1];
  const float v0 = i00 * d0 + i01 * d1, v1 = i10 * d0 + i11 * d1;
  for (int i = 0; i < 6; i++) rec[R_JP + i] = row[lin::J_PDXI + i] * v0 + row[lin::J_PDXI + 6 + i] * v1;
  rec[R_JP + 6] = k00 * d0 + k01 * d1, rec[R_JP + 7] = k10 * d0 + k11 * d1;
  rec[R_PDD] = d0, rec[R_PDD + 1] = d1, rec[R_V] = v0, rec[R_V + 1] = v1;
}

// A3: entry (a, b), a <= b, of the residual's 13 x 13 term
DSM_HD float top_term(const float *rec, int a, int b) {
  if (b < 10) {
    const float xa = rec[R_X + a], xb = rec[R_X + b], ya = rec[R_Y + a], yb = rec[R_Y + b];
    return (xa * xb) * rec[R_I2] + ((xa * yb) + (ya * xb)) * rec[R_I2 + 1] + (ya * yb) * rec[R_I2 + 2];
  }
  if (a < 10) return rec[R_X + a] * rec[R_K + 2 * (b - 10)] + rec[R_Y + a] * rec[R_K + 2 * (b - 10) + 1];
  return rec[R_BR + 3 * (a - 10) + (b - 10)];
}

// entry k in [0, 91) of the upper half, row by row
DSM_HD void top_entry(int k, int &a, int &b) {
  a = 0;
  while (k >= kTop - a) k -= kTop - a, a++;
  b = a + k;
}

// S1: one active residual into its point's sums
DSM_HD void point_add(const float *rec, float &bd, float &hdd, float &hcd0, float &hcd1, float &hcd2, float &hcd3) {
  const float d0 = rec[R_PDD], d1 = rec[R_PDD + 1], v0 = rec[R_V], v1 = rec[R_V + 1];
  bd += rec[R_K + 4] * d0 + rec[R_K + 5] * d1;
  hdd += v0 * d0 + v1 * d1;
  hcd0 += rec[R_X] * v0 + rec[R_Y] * v1, hcd1 += rec[R_X + 1] * v0 + rec[R_Y + 1] * v1;
  hcd2 += rec[R_X + 2] * v0 + rec[R_Y + 2] * v1, hcd3 += rec[R_X + 3] * v0 + rec[R_Y + 3] * v1;
}

// S2: prec[P_HDI ..] from the sums prec[P_HDD .. P_HDI) of a point with n_active active residuals; hcd_lin: four floats or null
DSM_HD void point_finish(float *prec, int n_active, float prior, float delta, float hdd_lin, float bd_lin, const float *hcd_lin, bool shift) {
  *reinterpret_cast<int *>(prec + P_NACT) = n_active;
  if (!n_active) {
    prec[P_HDI] = prec[P_BDSUM] = prec[P_IDH] = 0.0f;
    for (int c = 0; c < 4; c++) prec[P_HCDSUM + c] = 0.0f;
    return;
  }
  float H = (prec[P_HDD] + hdd_lin) + prior;
  if (H < 1e-10f) H = 1e-10f;
  prec[P_IDH] = H;
  prec[P_HDI] = (float)(1.0 / (double)H);
  float bd = prec[P_BD] + bd_lin;
  if (shift) bd = bd + prior * delta;
  prec[P_BDSUM] = bd;
  for (int c = 0; c < 4; c++) prec[P_HCDSUM + c] = prec[P_HCD + c] + (hcd_lin ? hcd_lin[c] : 0.0f);
}

// S3: the float terms, from a point's prec and the JpJdF of its residuals r1, r2
DSM_HD float term_Hcc(const float *prec, int c, int d) { return (prec[P_HCDSUM + c] * prec[P_HCDSUM + d]) * prec[P_HDI]; }
DSM_HD float term_bc(const float *prec, int c) { return prec[P_HCDSUM + c] * (prec[P_BDSUM] * prec[P_HDI]); }
DSM_HD float term_E(const float *prec, const float *jp1, int a, int c) { return (jp1[a] * prec[P_HCDSUM + c]) * prec[P_HDI]; }
DSM_HD float term_EB(const float *prec, const float *jp1, int a) { return jp1[a] * (prec[P_HDI] * prec[P_BDSUM]); }
DSM_HD float term_D(const float *prec, const float *jp1, const float *jp2, int a, int b) { return (jp1[a] * jp2[b]) * prec[P_HDI]; }

} // namespace hes
} // namespace dsm
