// rescale_math.hpp -- adopting the stereo scale into the window as DESIGN.md section 25 states it: the decision with its trapped /
// fail-count state (S1), a point (S2) and the newest frame (S3).  S4 is section 22's Z3 on the primed values and lives in
// finish_math.hpp, step_math.hpp and delta_math.hpp, on which this header sits.  The device kernel (rescale_kernels.hip) and the host
// form (rescale_host.cpp) share them, so that both evaluate one expression tree.  IEEE double and float, left to right as written, no
// contraction, no fma.
#pragma once

#include "finish_math.hpp"

namespace dsm {
namespace rsc {

// S0, S1 (FrontEnd.cpp:806, :1010-1023): the decision and the state behind it
struct Decision {
  int decision; // 0 disabled, 1 rejected, 2 accepted
  float scale_error;
  int trapped, fails;
};
inline Decision decide(int enabled, float scale_error, float new_scale, float thres, int trapped, int fails) {
  Decision d{0, -1.0f, trapped, fails};
  if (!enabled) return d; // S0
  bool succeed = scale_error < thres;                        // :1010, false for a NaN
  const bool jump = fabs((double)new_scale - 1.0) > 0.5;     // :1013
  if (trapped && jump) succeed = false;                      // :1014-1016
  d.fails = succeed ? 0 : fails + 1;                         // :1019
  d.scale_error = scale_error;
  if (d.fails > 5) d.trapped = 0, d.scale_error = -1.0f;     // :1020-1023
  if (succeed) d.trapped = 1;                                // :1057-1060
  d.decision = succeed ? 2 : 1;
  return d;
}

// S2: setIdepth(idepth / new_scale), setIdepthZero(idepth)
DSM_HD float point_idepth(float idepth, float new_scale) { return idepth / new_scale; }

// S3: the newest frame.  ctr = camToTrackingRef, ref = trackingRef->camToWorld; ctr_out its translation scaled, c2w = ref * ctr_out,
// eval its inverse; state = state_zero = (0 x 6, aff_g2l / SCALE_A, aff_g2l / SCALE_B) through upstream's float quotients
DSM_HD void newest_frame(const double *ctr, const double *ref, const double *aff_g2l, float new_scale, const stp::Scales &S, double ctr_out[7],
                         double c2w[7], double eval[7], double state[8]) {
  const double s = (double)new_scale;
  for (int k = 0; k < 4; k++) ctr_out[k] = ctr[k];
  for (int k = 4; k < 7; k++) ctr_out[k] = ctr[k] * s;
  stp::se3_mul(ref, ctr_out, c2w);
  stp::se3_inverse(c2w, eval);
  const double ia = (double)(1.0f / (float)S.a), ib = (double)(1.0f / (float)S.b);
  for (int k = 0; k < 6; k++) state[k] = 0.0;
  state[6] = ia * aff_g2l[0], state[7] = ib * aff_g2l[1];
}

} // namespace rsc
} // namespace dsm
