// step_math.hpp -- applying a step of the window optimisation as DESIGN.md section 19 states it: the calibration (D1), a frame's trial
// state and poses (D2), a point (D3), the step sums and can_break (D4), a pair's precalc row (Q1-Q4), and the entries of the stitched
// delta, the M energy and the priors (E1-E3).  The device kernels (step_kernels.hip) and the host form (step_host.cpp) share them, so
// that both evaluate one expression tree; each keeps its own way of walking frames, pairs, rows and points in the stated order.
// The quaternion, SE3 and light-transfer pieces restate lm_math.hpp's (the oracle's orc_se3_exp, orc_se3_mul, orc_quat_to_rot,
// orc_aff_from_to) for one lane and for the host.  IEEE double and float, left to right as written, no contraction
// (-ffp-contract=off), no fma.
#pragma once

#include <cmath>

#include "point_math.hpp"

namespace dsm {
namespace stp {

struct Scales { // dsm_step_params and the three scales of dsm_linearize_params this call reads
  double xi_trans, xi_rot, a, b, th;
  float f, c, idepth;
};

DSM_HD void quat_normalize(double q[4]) {
  const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  q[0] /= n, q[1] /= n, q[2] /= n, q[3] /= n;
}
DSM_HD void quat_to_rot(const double q[4], double R[9]) {
  const double x = q[0], y = q[1], z = q[2], w = q[3];
  const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w;
  const double txx = tx * x, txy = ty * x, txz = tz * x;
  const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
  R[0] = 1.0 - (tyy + tzz), R[1] = txy - twz, R[2] = txz + twy;
  R[3] = txy + twz, R[4] = 1.0 - (txx + tzz), R[5] = tyz - twx;
  R[6] = txz - twy, R[7] = tyz + twx, R[8] = 1.0 - (txx + tyy);
}
DSM_HD void quat_mul(const double a[4], const double b[4], double o[4]) {
  const double ax = a[0], ay = a[1], az = a[2], aw = a[3];
  const double bx = b[0], by = b[1], bz = b[2], bw = b[3];
  o[3] = aw * bw - ax * bx - ay * by - az * bz;
  o[0] = aw * bx + ax * bw + ay * bz - az * by;
  o[1] = aw * by + ay * bw + az * bx - ax * bz;
  o[2] = aw * bz + az * bw + ax * by - ay * bx;
}
DSM_HD void quat_rotate(const double q[4], const double v[3], double o[3]) {
  double uv0 = q[1] * v[2] - q[2] * v[1], uv1 = q[2] * v[0] - q[0] * v[2], uv2 = q[0] * v[1] - q[1] * v[0];
  uv0 += uv0, uv1 += uv1, uv2 += uv2;
  const double c0 = q[1] * uv2 - q[2] * uv1, c1 = q[2] * uv0 - q[0] * uv2, c2 = q[0] * uv1 - q[1] * uv0;
  o[0] = v[0] + q[3] * uv0 + c0;
  o[1] = v[1] + q[3] * uv1 + c1;
  o[2] = v[2] + q[3] * uv2 + c2;
}
// Sophus SE3 product a * b
DSM_HD void se3_mul(const double a[7], const double b[7], double out[7]) {
  double r[3], q[4];
  quat_rotate(a, b + 4, r);
  quat_mul(a, b, q);
  quat_normalize(q);
  out[0] = q[0], out[1] = q[1], out[2] = q[2], out[3] = q[3];
  out[4] = a[4] + r[0], out[5] = a[5] + r[1], out[6] = a[6] + r[2];
}
// Sophus SE3 inverse: the conjugate quaternion, then t' = -(q' t)
DSM_HD void se3_inverse(const double a[7], double out[7]) {
  const double qc[4] = {-a[0], -a[1], -a[2], a[3]};
  double r[3];
  quat_rotate(qc, a + 4, r);
  out[0] = qc[0], out[1] = qc[1], out[2] = qc[2], out[3] = qc[3];
  out[4] = -r[0], out[5] = -r[1], out[6] = -r[2];
}
// Sophus SE3::exp, tangent = [upsilon ; omega], in one lane
DSM_HD void se3_exp(const double xi[6], double pose[7]) {
  const double *ups = xi, *om = xi + 3;
  const double theta_sq = om[0] * om[0] + om[1] * om[1] + om[2] * om[2];
  const double theta = sqrt(theta_sq);
  const double half = 0.5 * theta;
  const bool small = theta < 1e-10;
  double imag, real, s_th = 0.0, c_th = 1.0;
  if (small) {
    const double t2 = theta * theta, t4 = t2 * t2;
    imag = 0.5 - (1.0 / 48.0) * t2 + (1.0 / 3840.0) * t4;
    real = 1.0 - 0.5 * t2 + (1.0 / 384.0) * t4;
  } else {
    double s_half;
#if defined(__HIP_DEVICE_COMPILE__)
    sincos(half, &s_half, &real);
    sincos(theta, &s_th, &c_th);
#else
    s_half = sin(half), real = cos(half), s_th = sin(theta), c_th = cos(theta);
#endif
    imag = s_half / theta;
  }
  double q[4] = {imag * om[0], imag * om[1], imag * om[2], real};
  quat_normalize(q);
  double V[9];
  if (small) {
    quat_to_rot(q, V);
  } else {
    const double O[9] = {0, -om[2], om[1], om[2], 0, -om[0], -om[1], om[0], 0};
    double O2[9];
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) O2[i * 3 + j] = O[i * 3 + 0] * O[0 * 3 + j] + O[i * 3 + 1] * O[1 * 3 + j] + O[i * 3 + 2] * O[2 * 3 + j];
    const double ca = (1.0 - c_th) / theta_sq;
    const double cb = (theta - s_th) / (theta_sq * theta);
    for (int i = 0; i < 9; i++) V[i] = ((i % 4 == 0) ? 1.0 : 0.0) + ca * O[i] + cb * O2[i];
  }
  pose[0] = q[0], pose[1] = q[1], pose[2] = q[2], pose[3] = q[3];
  for (int i = 0; i < 3; i++) pose[4 + i] = V[i * 3 + 0] * ups[0] + V[i * 3 + 1] * ups[1] + V[i * 3 + 2] * ups[2];
}
DSM_HD void mat3f_mul(const float *a, const float *b, float *o) {
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) o[i * 3 + j] = (a[i * 3 + 0] * b[0 * 3 + j] + a[i * 3 + 1] * b[1 * 3 + j]) + a[i * 3 + 2] * b[2 * 3 + j];
}

// D1: entry c of the calibration: the value, the scaled value as float (cam[c]) and c_delta[c]
DSM_HD void calib_entry(int c, double backup, float fac_c, double step, double zero, const Scales &S, double &value, float &cam, float &c_delta) {
  value = backup + (double)fac_c * step;
  cam = (float)((double)(c < 2 ? S.f : S.c) * value);
  c_delta = (float)(value - zero);
}
DSM_HD float cam_inverse(float f) { return 1.0f / f; }

// D2: the factor of state entry k among stepfac = (C, T, R, A, D), and its scale
DSM_HD float frame_factor(const float *stepfac, int k) { return k < 3 ? stepfac[1] : k < 6 ? stepfac[2] : stepfac[3]; }
DSM_HD double frame_scale(const Scales &S, int k) { return k < 3 ? S.xi_trans : k < 6 ? S.xi_rot : k == 6 ? S.a : S.b; }
// D2: a frame's trial state, delta_f, aff and the two poses
DSM_HD void frame_state(const double *backup, const double *step, const double *zero, const double *eval, const float *stepfac, const Scales &S,
                        double state[8], double delta_f[8], double aff[2], double W[7], double C[7]) {
  double scaled[8];
  for (int k = 0; k < 8; k++) {
    state[k] = backup[k] + (double)frame_factor(stepfac, k) * step[k];
    scaled[k] = state[k] * frame_scale(S, k);
    delta_f[k] = state[k] - zero[k];
  }
  double ex[7];
  se3_exp(scaled, ex);
  se3_mul(ex, eval, W);
  se3_inverse(W, C);
  aff[0] = scaled[6], aff[1] = scaled[7];
}

// D3
DSM_HD float point_idepth(float backup, float fac_d, float step) { return backup + fac_d * step; }
DSM_HD float point_idepth_scaled(float scale, float idepth) { return scale * idepth; }

// D4: one frame's term of a float accumulator: a double product (or squared norm), added in double, rounded to float
DSM_HD float sum_frame(float acc, double term) { return (float)((double)acc + term); }
DSM_HD double squared_norm3(const double *x) { return (x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]; }
// D4: the frames' four sums (A, B, R, T) after their division by the frame count
DSM_HD void frame_sums(const double *frame_step, int n, float out[4]) {
  float a = 0.0f, b = 0.0f, t = 0.0f, r = 0.0f;
  for (int f = 0; f < n; f++) {
    const double *s = frame_step + 8 * f;
    a = sum_frame(a, s[6] * s[6]);
    b = sum_frame(b, s[7] * s[7]);
    t = sum_frame(t, squared_norm3(s));
    r = sum_frame(r, squared_norm3(s + 3));
  }
  const float nf = (float)n;
  out[0] = a / nf, out[1] = b / nf, out[2] = r / nf, out[3] = t / nf;
}
// D4: a point's term of sumID
DSM_HD float point_sq(float step) { return step * step; }
// D4: the points' two chains over ascending index, divided by the count (0 / 0 for no point, as the reference)
DSM_HD void point_sums(const float *idepth_backup, const float *idepth_step, int n_pts, float out[2]) {
  float id = 0.0f, nid = 0.0f, num = 0.0f;
  for (int p = 0; p < n_pts; p++) {
    id += point_sq(idepth_step[p]);
    nid += fabsf(idepth_backup[p]);
    num += 1.0f;
  }
  out[0] = id / num, out[1] = nid / num;
}
// D4: sums = (A, B, R, T, ID, NID)
DSM_HD int can_break(const float *sums, double th) {
  return (double)sqrtf(sums[0]) < 0.0005 * th && (double)sqrtf(sums[1]) < 0.00005 * th && (double)sqrtf(sums[2]) < 0.00005 * th &&
         (double)(sqrtf(sums[3]) * sums[5]) < 0.00005 * th;
}

// Q1-Q4: the row of pair (h, t), h != t.  eval_inv_h = eval_h^-1; cam = (fx, fy, cx, cy, fxi, fyi)
struct PairRow {
  float R0[9], t0[3], M[9], Kt[3], aff[2], b0;
};
DSM_HD void pair_row(const double *eval_t, const double *eval_inv_h, const double *W_t, const double *C_h, const float *cam, float exp_h, float exp_t,
                     const double *aff_h, const double *aff_t, double zero_b_h, double scale_b, PairRow &o) {
  double L0[7], L[7], Rd[9];
  float R[9], t[3];
  se3_mul(eval_t, eval_inv_h, L0);
  quat_to_rot(L0, Rd);
  for (int i = 0; i < 9; i++) o.R0[i] = (float)Rd[i];
  for (int i = 0; i < 3; i++) o.t0[i] = (float)L0[4 + i];
  se3_mul(W_t, C_h, L);
  quat_to_rot(L, Rd);
  for (int i = 0; i < 9; i++) R[i] = (float)Rd[i];
  for (int i = 0; i < 3; i++) t[i] = (float)L[4 + i];
  const float K[9] = {cam[0], 0.0f, cam[2], 0.0f, cam[1], cam[3], 0.0f, 0.0f, 1.0f};
  const float Ki[9] = {cam[4], 0.0f, -cam[2] * cam[4], 0.0f, cam[5], -cam[3] * cam[5], 0.0f, 0.0f, 1.0f};
  float KR[9];
  mat3f_mul(K, R, KR);
  mat3f_mul(KR, Ki, o.M);
  for (int i = 0; i < 3; i++) o.Kt[i] = (K[i * 3 + 0] * t[0] + K[i * 3 + 1] * t[1]) + K[i * 3 + 2] * t[2];
  if (exp_h == 0 || exp_t == 0) exp_t = exp_h = 1;
  const double a = exp(aff_t[0] - aff_h[0]) * exp_t / exp_h;
  o.aff[0] = (float)a;
  o.aff[1] = (float)(aff_t[1] - a * aff_h[1]);
  o.b0 = (float)(zero_b_h * scale_b);
}

// E2: row i's term of the M energy (hm_row, b_m: null reads as zeros)
DSM_HD double energy_m_term(const double *hm_row, const double *b_m, const double *dx, int i, int N) {
  double s = 0.0;
  for (int j = 0; j < N; j++) s += (hm_row ? hm_row[j] : 0.0) * dx[j];
  return dx[i] * (2.0 * (b_m ? b_m[i] : 0.0) + s);
}
// E3
DSM_HD double prior_h(double hl_ii, double prior_i) { return hl_ii + prior_i; }
DSM_HD double prior_b(double bl_i, double prior_i, double dp_i) { return bl_i + prior_i * dp_i; }

} // namespace stp
} // namespace dsm
