// finish_math.hpp -- the end of FrontEnd::optimize behind its loop as DESIGN.md section 22 states it: the newest frame's new evaluation
// point (Z1), a pair's adHost / adTarget (Z2), a frame's poses and a calibration entry at the committed state (Z3, on step_math.hpp's
// pieces), a point's bookkeeping over its residuals (Z5, Z6) and the result (Z8).  The device kernels (finish_kernels.hip) and the host
// form (finish_host.cpp) share them, so that both evaluate one expression tree; each keeps its own way of walking frames, pairs, points
// and residuals in the stated order.  IEEE double and float, left to right as written, no contraction, no fma.
#pragma once

#include "delta_math.hpp"
#include "step_math.hpp"

namespace dsm {
namespace fin {

// Z1: the newest frame's state and state_zero after setEvalPT: no pose part, the affine part of the committed state
DSM_HD void newest_state(const double *committed, double out[8]) {
  for (int k = 0; k < 6; k++) out[k] = 0.0;
  out[6] = committed[6], out[7] = committed[7];
}

// D1 of section 19 on the committed value of calibration entry c: cam[c] and c_delta[c]
DSM_HD void calib_cam(int c, double value, double zero, const stp::Scales &S, float &cam, float &c_delta) {
  cam = (float)((double)(c < 2 ? S.f : S.c) * value);
  c_delta = (float)(value - zero);
}

// D2 of section 19 on a given state: delta_f, aff (of the state), aff0 (of state_zero: Z2 reads it) and the two poses
DSM_HD void frame_pose(const double *state, const double *zero, const double *eval, const stp::Scales &S, double delta_f[8], double aff[2], double aff0[2],
                       double W[7], double C[7]) {
  double scaled[8];
  for (int k = 0; k < 8; k++) {
    scaled[k] = state[k] * stp::frame_scale(S, k);
    delta_f[k] = state[k] - zero[k];
  }
  double ex[7];
  stp::se3_exp(scaled, ex);
  stp::se3_mul(ex, eval, W);
  stp::se3_inverse(W, C);
  aff[0] = scaled[6], aff[1] = scaled[7];
  aff0[0] = zero[6] * S.a, aff0[1] = zero[7] * S.b;
}

// Z2: aff_from_to(exposure_h, exposure_t, aff0_h, aff0_t).a (Q4's expression) through float
DSM_HD double aff_a0(const double *aff0_h, const double *aff0_t, float exp_h, float exp_t) {
  if (exp_h == 0 || exp_t == 0) exp_t = exp_h = 1;
  const double a = exp(aff0_t[0] - aff0_h[0]) * exp_t / exp_h;
  return (double)(float)a;
}

// Z2: Adj(L0) = [[R, t^ R], [0, R]] (6 x 6, row-major), L0 = eval_t eval_h^-1 by Q1's operations
DSM_HD void adjoint(const double *eval_t, const double *eval_inv_h, double Adj[36]) {
  double L0[7], R[9];
  stp::se3_mul(eval_t, eval_inv_h, L0);
  stp::quat_to_rot(L0, R);
  const double tx = L0[4], ty = L0[5], tz = L0[6];
  const double T[9] = {0.0, -tz, ty, tz, 0.0, -tx, -ty, tx, 0.0};
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      const double tr = (T[i * 3 + 0] * R[0 * 3 + j] + T[i * 3 + 1] * R[1 * 3 + j]) + T[i * 3 + 2] * R[2 * 3 + j];
      Adj[i * 6 + j] = R[i * 3 + j], Adj[i * 6 + 3 + j] = tr, Adj[(3 + i) * 6 + j] = 0.0, Adj[(3 + i) * 6 + 3 + j] = R[i * 3 + j];
    }
}

// Z2: the pair's adHost and adTarget (8 x 8, row-major) from Adj and a
DSM_HD void adjoint_pair(const double Adj[36], double a, const stp::Scales &S, double *AH, double *AT) {
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const double scale = stp::frame_scale(S, k);
#pragma unroll
    for (int c = 0; c < 8; c++) {
      double h = k == c ? 1.0 : 0.0, t = h;
      if (k < 6 && c < 6) h = -Adj[c * 6 + k];
      if (k == 6 && c == 6) h = a, t = -a;
      if (k == 7 && c == 7) h = a, t = -1.0;
      AH[8 * k + c] = h * scale, AT[8 * k + c] = t * scale;
    }
  }
}

// Z5, Z6: a point's bookkeeping.  Res answers, for a residual index, keep(r), is_new(r), rel_bs(r) and new_state(r) of the final
// linearisation; list[0 .. count) are the point's residuals in ascending index
struct PointBook {
  int n_good;
  float max_rel_baseline;
  int last_res[2];
  unsigned char last_state[2];
  int n_kept;
  unsigned char dropped;
};
template <class Res>
DSM_HD void point_book(const int *list, int count, const Res &R, int n_good_in, float max_rel_baseline_in, const int *last_res_in, const int *last_state_in,
                       PointBook &o) {
  o.n_good = n_good_in, o.max_rel_baseline = max_rel_baseline_in, o.n_kept = 0;
  for (int i = 0; i < count; i++) {
    const int r = list[i];
    if (!R.keep(r)) continue;
    o.n_kept++;
    if (!R.is_new(r)) continue;
    o.n_good++;
    const float rel = R.rel_bs(r);
    if (rel > o.max_rel_baseline) o.max_rel_baseline = rel;
  }
  const int l0 = last_res_in[0], l1 = last_res_in[1];
  o.last_res[0] = l0, o.last_res[1] = l1;
  o.last_state[0] = (unsigned char)last_state_in[0], o.last_state[1] = (unsigned char)last_state_in[1];
  if (l0 >= 0) o.last_state[0] = (unsigned char)R.new_state(l0); // :147-153
  if (l1 >= 0 && l1 != l0) o.last_state[1] = (unsigned char)R.new_state(l1);
  if (l0 >= 0 && !R.keep(l0)) o.last_res[0] = -1; // :156-164
  if (l1 >= 0 && l1 != l0 && !R.keep(l1)) o.last_res[1] = -1;
  o.dropped = o.n_kept == 0; // Z6
}

// Z8
DSM_HD int lost(double energy) { return !(fabs(energy) <= 1.7976931348623157e308); }
DSM_HD float rmse(double energy, int n_res_out) { return sqrtf((float)(energy / (double)(8 * n_res_out))); }

} // namespace fin
} // namespace dsm
