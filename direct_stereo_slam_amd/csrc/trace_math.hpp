// trace_math.hpp -- ImmaturePoint::traceOn as DESIGN.md section 14 states it (T1-T16): the arithmetic the device kernel
// (trace_kernels.hip) and the host form (points_host.cpp) share, so that both evaluate the same expression tree.  float32 throughout,
// no contraction (-ffp-contract=off), no fmaf; division and sqrtf correctly rounded.  The sums over the eight pattern pixels are the
// callers': the host form adds in a loop, the kernel along the lanes of a point, both in pattern order.
#pragma once

#include "../../include/dsm_hotpath.h"
#include "point_math.hpp"

namespace dsm {
namespace trc {

// the fields of an ImmaturePoint that traceOn reads and writes
struct Point {
  int status;
  float idepth_min, idepth_max, quality, uv0, uv1, interval;
};

// what T2-T7 leave for the search, the refinement and the new interval
struct Line {
  pt::Vec3 pr;    // K R K^-1 (u, v, 1)
  float dx, dy;   // the unit step along the epipolar line
  float err;      // errorInPixel
  float ptx, pty; // the first position of the search
  int numSteps;
};

struct GN {
  float bestU, bestV, uBak, vBak, stepBack, bestEnergy;
};

DSM_HD bool inside(float u, float v, int w, int h) { return u > 4 && v > 4 && u < (float)(w - 5) && v < (float)(h - 5); } // T2
DSM_HD void oob_exit(Point &P) { P.uv0 = -1, P.uv1 = -1, P.interval = 0, P.status = DSM_IPS_OOB; }

// T1-T7 for the point (u, v) of a host with K R K^-1 = R (row-major), K t = t and gradH = G.  True: the search runs on L.  False: the
// rule that returned has written P (T1: nothing).
DSM_HD bool geometry(int w, int h, const float *R, const float *t, float u, float v, const float *G, const dsm_trace_params &S, Point &P,
                     Line &L) {
  if (P.status == DSM_IPS_OOB) return false; // T1
  const float maxPix = (float)(w + h) * S.max_pix_search; // T2
  L.pr = pt::rotate_uv1(R, u, v);
  const pt::Vec3 m = pt::add_translation(L.pr, t, P.idepth_min);
  const float m2 = m.z, uMin = m.x / m2, vMin = m.y / m2;
  if (!inside(uMin, vMin, w, h)) {
    oob_exit(P);
    return false;
  }
  const bool bounded = __builtin_isfinite(P.idepth_max);
  float dist, uMax, vMax;
  if (bounded) { // T3
    const pt::Vec3 x = pt::add_translation(L.pr, t, P.idepth_max);
    uMax = x.x / x.z, vMax = x.y / x.z;
    if (!inside(uMax, vMax, w, h)) {
      oob_exit(P);
      return false;
    }
    dist = __builtin_sqrtf((uMin - uMax) * (uMin - uMax) + (vMin - vMax) * (vMin - vMax));
    if (dist < S.slack_interval) {
      P.uv0 = (uMax + uMin) * 0.5f, P.uv1 = (vMax + vMin) * 0.5f, P.interval = dist, P.status = DSM_IPS_SKIPPED;
      return false;
    }
  } else { // T4
    dist = maxPix;
    const pt::Vec3 x = pt::add_translation(L.pr, t, 0.01f);
    uMax = x.x / x.z, vMax = x.y / x.z;
    const float dx = uMax - uMin, dy = vMax - vMin;
    const float d = 1.0f / __builtin_sqrtf(dx * dx + dy * dy);
    uMax = uMin + (dist * dx) * d;
    vMax = vMin + (dist * dy) * d;
    if (!inside(uMax, vMax, w, h)) {
      oob_exit(P);
      return false;
    }
  }
  if (!(P.idepth_min < 0 || (m2 > 0.75f && m2 < 1.5f))) { // T5
    oob_exit(P);
    return false;
  }
  float dx = S.stepsize * (uMax - uMin), dy = S.stepsize * (vMax - vMin); // T6
  const float a = (dx * G[0] + dy * G[2]) * dx + (dx * G[1] + dy * G[3]) * dy;
  const float nx = -dx;
  const float b = (dy * G[0] + nx * G[2]) * dy + (dy * G[1] + nx * G[3]) * nx;
  float err = 0.2f + (0.2f * (a + b)) / a;
  if (err * S.min_improvement > dist && bounded) {
    P.uv0 = (uMax + uMin) * 0.5f, P.uv1 = (vMax + vMin) * 0.5f, P.interval = dist, P.status = DSM_IPS_BADCONDITION;
    return false;
  }
  if (err > 10) err = 10;
  dx /= dist, dy /= dist; // T7
  if (dist > maxPix) dist = maxPix;
  const float fsteps = 1.9999f + dist / S.stepsize;
  const int numSteps = fsteps >= 100.0f ? DSM_TRACE_MAX_STEPS : (int)fsteps; // (int) then the cap at 99, without converting what no int holds
  const float k1000 = uMin * 1000;
  const float randShift = k1000 - __builtin_floorf(k1000);
  L.ptx = uMin - randShift * dx, L.pty = vMin - randShift * dy;
  if (!__builtin_isfinite(dx) || !__builtin_isfinite(dy)) {
    oob_exit(P);
    return false;
  }
  L.dx = dx, L.dy = dy, L.err = err, L.numSteps = numSteps;
  return true;
}

// the rotated pattern pixel of T7
DSM_HD void rotated_pattern(const float *R, int k, float &rx, float &ry) {
  int px, py;
  pt::pattern(k, px, py);
  rx = R[0] * (float)px + R[1] * (float)py;
  ry = R[3] * (float)px + R[4] * (float)py;
}

// T8: samples outside this box count as non-finite; inside it the twelve texels of a sample lie in the plane
DSM_HD bool guard(float x, float y, int w, int h) { return x >= 1 && y >= 1 && x < (float)(w - 2) && y < (float)(h - 2); }

// T9: one pixel's term of a step's energy; `ok`: the sample passed the guard, hI is its intensity
DSM_HD float search_term(bool ok, float hI, const float *aff, float color, float huber) {
  if (!ok || !__builtin_isfinite(hI)) return 1e5f;
  const float r = hI - (aff[0] * color + aff[1]);
  const float ar = __builtin_fabsf(r);
  const float hw = ar < huber ? 1.0f : huber / ar;
  return ((hw * r) * r) * (2 - hw);
}

// T11: one pixel's terms of an iteration.  False: the sample is non-finite, tE = 1e5f and nothing goes into H and b.
DSM_HD bool gn_terms(bool ok, float hI, float gx, float gy, const float *aff, float color, float wt, float huber, float dx, float dy,
                     float &tH, float &tb, float &tE) {
  tH = 0.f, tb = 0.f;
  if (!ok || !__builtin_isfinite(hI)) {
    tE = 1e5f;
    return false;
  }
  const float r = hI - (aff[0] * color + aff[1]);
  const float ar = __builtin_fabsf(r);
  const float hw = ar < huber ? 1.0f : huber / ar;
  const float dRes = dx * gx + dy * gy;
  tH = (hw * dRes) * dRes;
  tb = (hw * r) * dRes;
  tE = ((((wt * wt) * hw) * r) * r) * (2 - hw);
  return true;
}

// T10: steps i < bestIdx - radius || i > bestIdx + radius count; a radius above the 99 steps excludes them all, whatever its size
DSM_HD int test_radius(const dsm_trace_params &S) { return S.min_test_radius > 100 ? 100 : S.min_test_radius; }
DSM_HD bool outside_radius(int i, int bestIdx, int radius) { return i < bestIdx - radius || i > bestIdx + radius; }
DSM_HD void quality_update(Point &P, float secondBest, float bestEnergy, int numSteps) {
  const float q = secondBest / bestEnergy;
  if (q < P.quality || numSteps > 10) P.quality = q;
}

// T11: the end of an iteration, given its sums.  True: the loop ends.
DSM_HD bool gn_update(GN &g, float H, float b, float E, float dx, float dy, float gn_threshold) {
  if (E > g.bestEnergy) {
    g.stepBack *= 0.5f;
    g.bestU = g.uBak + g.stepBack * dx;
    g.bestV = g.vBak + g.stepBack * dy;
  } else {
    float step = (-b) / H;
    if (step < -0.5f) step = -0.5f;
    else if (step > 0.5f) step = 0.5f;
    if (!__builtin_isfinite(step)) step = 0;
    g.uBak = g.bestU, g.vBak = g.bestV, g.stepBack = step;
    g.bestU += step * dx;
    g.bestV += step * dy;
    g.bestEnergy = E;
  }
  return __builtin_fabsf(g.stepBack) < gn_threshold;
}

// T12-T15; `entered`: the status the point came with
DSM_HD void finish(Point &P, const Line &L, const GN &g, const float *t, float energy_th, const dsm_trace_params &S, int entered) {
  if (!(g.bestEnergy < energy_th * S.extra_slack_on_th)) { // T12
    P.uv0 = -1, P.uv1 = -1, P.interval = 0;
    P.status = entered == DSM_IPS_OUTLIER ? DSM_IPS_OOB : DSM_IPS_OUTLIER;
    return;
  }
  float lo, hi; // T13
  if (L.dx * L.dx > L.dy * L.dy) {
    lo = (L.pr.z * (g.bestU - L.err * L.dx) - L.pr.x) / (t[0] - t[2] * (g.bestU - L.err * L.dx));
    hi = (L.pr.z * (g.bestU + L.err * L.dx) - L.pr.x) / (t[0] - t[2] * (g.bestU + L.err * L.dx));
  } else {
    lo = (L.pr.z * (g.bestV - L.err * L.dy) - L.pr.y) / (t[1] - t[2] * (g.bestV - L.err * L.dy));
    hi = (L.pr.z * (g.bestV + L.err * L.dy) - L.pr.y) / (t[1] - t[2] * (g.bestV + L.err * L.dy));
  }
  if (lo > hi) {
    const float s = lo;
    lo = hi, hi = s;
  }
  P.idepth_min = lo, P.idepth_max = hi;
  if (!__builtin_isfinite(lo) || !__builtin_isfinite(hi) || hi < 0) { // T14: the idepths keep what was just written
    P.uv0 = -1, P.uv1 = -1, P.interval = 0, P.status = DSM_IPS_OUTLIER;
    return;
  }
  P.interval = 2 * L.err, P.uv0 = g.bestU, P.uv1 = g.bestV, P.status = DSM_IPS_GOOD; // T15
}

} // namespace trc
} // namespace dsm
