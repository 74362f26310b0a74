// immature_math.hpp -- FrontEnd::optimizeImmaturePoint as DESIGN.md section 13 states it: one pattern pixel of
// ImmaturePoint::linearizeResidual (U2-U8) and the Levenberg-Marquardt rules around the passes over the residuals (M1, M3-M5, the
// final status).  The device kernel (immature_kernels.hip) and the host form (points_host.cpp) share both, so that they evaluate the
// same expression tree; each keeps its own way of summing a pass and of committing the residual states.  float32 throughout, no
// contraction (-ffp-contract=off), no fmaf; the step's quotient and product (M3) and the stop test (M5) in double.
#pragma once

#include "point_math.hpp"

namespace dsm {
namespace imm {

enum { RES_IN = 0, RES_OOB = 1, RES_OUTLIER = 2 }; // DSM_RES_*

struct Cam {
  float fx, fy, cx, cy, fxi, fyi;
  int w, h;
};

// Pattern pixel (dx, dy) of the point (u, v) at inverse depth idepth against the frame plane I, with the pair's PRE_RTll R (row-major),
// PRE_tTll t and PRE_aff_mode aff.  False: the pixel fails (U4: projection or bounds; U6: non-finite intensity) and nothing is
// written.  True: tE, tH, tb are the pixel's terms of the energy, Hdd and bd (U7, U8); the caller adds them in pattern order.
DSM_HD bool tap(const Cam &C, const float *I, const float *R, const float *t, const float *aff, float u, float v, int dx, int dy,
                float idepth, float color, float wt, float huber, float &tE, float &tH, float &tb) {
  const float k0 = ((u + (float)dx) - C.cx) * C.fxi, k1 = ((v + (float)dy) - C.cy) * C.fyi;
  const pt::Vec3 p = pt::add_translation(pt::rotate_uv1(R, k0, k1), t, idepth);
  const float drescale = 1.0f / p.z;
  if (!(drescale > 0.0f)) return false;
  const float up = p.x * drescale, vp = p.y * drescale;
  const float Ku = up * C.fx + C.cx, Kv = vp * C.fy + C.cy;
  if (!(Ku > 1.1f && Kv > 1.1f && Ku < (float)(C.w - 3) && Kv < (float)(C.h - 3))) return false;
  // ix in [1, w - 4], iy in [1, h - 4]: the twelve texels lie in the plane
  float hI, hx, hy;
  pt::interp_Ig(pt::load12(I, C.w, Ku, Kv), Ku, Kv, hI, hx, hy);
  if (!__builtin_isfinite(hI)) return false;
  const float r = hI - (aff[0] * color + aff[1]);
  const float ar = __builtin_fabsf(r);
  float hw = ar < huber ? 1.0f : huber / ar;
  tE = ((((wt * wt) * hw) * r) * r) * (2 - hw);
  const float d = ((hx * C.fx) * drescale) * (t[0] - t[2] * up) + ((hy * C.fy) * drescale) * (t[1] - t[2] * vp);
  hw *= wt * wt;
  tH = (hw * d) * d;
  tb = (hw * r) * d;
  return true;
}

// the optimisation of one point between its passes (FrontEndOptPoint.cpp:48-138)
struct LM {
  float idepth, energy, Hdd, bd; // currentIdepth, lastEnergy, lastHdd, lastbd
  float lambda, step, trial;     // of the pass to come: the step and the inverse depth it is taken at
  int status, iterations;        // status: -1 until decided, then 0 not yet, 1 activate, 2 delete
  bool done;                     // no further pass
};

DSM_HD float lm_start(float idepth_min, float idepth_max) { return (idepth_max + idepth_min) * 0.5f; } // M1

// after the first pass (M2), taken at lm_start with slack 1000: its sums (:63-68)
DSM_HD LM lm_begin(float idepth, float E, float Hdd, float bd, float min_h) {
  LM s{idepth, E, Hdd, bd, 0.1f, 0.f, 0.f, -1, 0, false};
  if (!__builtin_isfinite(E) || Hdd < min_h) s.status = 0, s.done = true;
  return s;
}

// M3: the inverse depth of the next pass; quotient and product in double, rounded once
DSM_HD float lm_propose(LM &s) {
  float H = s.Hdd;
  H *= 1 + s.lambda;
  s.step = (float)((1.0 / (double)H) * (double)s.bd);
  s.trial = s.idepth - s.step;
  return s.trial;
}

// the end of an iteration, given the sums of the pass at lm_propose's inverse depth.  True: the pass is accepted and the caller
// commits the residuals' new states and energies.
DSM_HD bool lm_trial(LM &s, float newEnergy, float newHdd, float newbd, float min_h) {
  s.iterations++;
  if (!__builtin_isfinite(s.energy) || newHdd < min_h) { // M4: lastEnergy, not newEnergy (:90)
    s.status = 0, s.done = true;
    return false;
  }
  const bool accepted = newEnergy < s.energy;
  if (accepted) {
    s.idepth = s.trial, s.Hdd = newHdd, s.bd = newbd, s.energy = newEnergy;
    s.lambda *= 0.5f;
  } else {
    s.lambda *= 5.f;
  }
  if ((double)__builtin_fabsf(s.step) < 0.0001 * (double)s.idepth) s.done = true; // M5: in double, against the already updated depth
  return accepted;
}

// :121-138; good: the residuals that ended IN
DSM_HD void lm_finish(LM &s, int good, int min_obs) {
  if (s.status < 0) s.status = (!__builtin_isfinite(s.idepth) || good < min_obs) ? 2 : 1;
}

} // namespace imm
} // namespace dsm
