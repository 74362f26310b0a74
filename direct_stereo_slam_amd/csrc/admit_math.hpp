// admit_math.hpp -- admitting the new keyframe into the window as DESIGN.md section 26 states it: the distance of a pair (A2), the
// rules of flagFramesForMarginalization (A4: F0, F1, F2; FrontEndMarginalize.cpp:62-146) and where a residual stands once every point
// has its forward residual (A6; FrontEnd.cpp:746-762).  A1 is rescale_math.hpp's newest_frame at scale 1, A2 and A3 are section 22's
// Z3 and Z2 in finish_math.hpp, step_math.hpp and delta_math.hpp, on which this header sits.  The device kernel (admit_kernels.hip)
// and the host form (admit_host.cpp) share them, so that both evaluate one expression tree.  IEEE double and float, left to right as
// written, no contraction, no fma.
#pragma once

#include "rescale_math.hpp"

namespace dsm {
namespace adm {

struct Params { // dsm_admit_params
  int min_frames, max_frames, min_frame_age;
  float min_points_remaining, max_log_aff_fac_in_window;
};

// A2: FrameFramePrecalc::set's distanceLL, the norm of the translation of L = W_t C_h (Q1's product) in double, kept as float
DSM_HD float distance_ll(const double *W_t, const double *C_h) {
  double L[7];
  stp::se3_mul(W_t, C_h, L);
  return (float)sqrt((L[4] * L[4] + L[5] * L[5]) + L[6] * L[6]);
}

// F0 (:63-69): frame i of the old window under setting_minFrameAge > setting_maxFrames
DSM_HD bool f0_branch(const Params &P) { return P.min_frame_age > P.max_frames; }
DSM_HD bool f0_flagged(int i, int n, const Params &P) { return (long long)i + P.max_frames < n; }

// F1 (:75-85): frame i against the newest old frame `last`; aff_* = (scaled[6], scaled[7]) of D2; `flagged` counted so far
DSM_HD bool f1_flagged(int in, int out, float exp_last, float exp_i, const double *aff_last, const double *aff_i, int n, int flagged, const Params &P) {
  const double a = fin::aff_a0(aff_last, aff_i, exp_last, exp_i); // fromToVecExposure(last, i)[0], Q4's expression
  const bool few = (float)in < P.min_points_remaining * (float)(in + out);
  const bool bright = fabsf(logf((float)a)) > P.max_log_aff_fac_in_window;
  return (few || bright) && n - flagged > P.min_frames;
}

// F2 (:116-118, :123-125): the frames that may leave, and the targets a score counts
DSM_HD bool f2_candidate(int id, int id_last, const Params &P) { return !((long long)id > (long long)id_last - P.min_frame_age || id == 0); }
DSM_HD bool f2_counts(int id_t, int id_last, const Params &P) { return !((long long)id_t > (long long)id_last - P.min_frame_age + 1); }
// F2 (:121-128): host h's score over the old window; dist_h = distance_ll[h][.], ids = keyframe_id
DSM_HD double f2_score(const float *dist_h, const int *ids, int h, int n, const Params &P) {
  double s = 0.0;
  for (int t = 0; t < n; t++) {
    if (t == h || !f2_counts(ids[t], ids[n - 1], P)) continue;
    s += 1.0 / (1e-5 + (double)dist_h[t]);
  }
  return s * -(double)sqrtf(dist_h[n - 1]);
}
// F2 (:111, :130-133): the first candidate with the smallest score below 1; -1: none (the source dereferences a null pointer there)
DSM_HD int f2_pick(const double *score, const int *ids, int n, const Params &P) {
  double smallest = 1.0;
  int pick = -1;
  for (int h = 0; h < n; h++)
    if (f2_candidate(ids[h], ids[n - 1], P) && score[h] < smallest) smallest = score[h], pick = h;
  return pick;
}

// A6: residuals grouped by point in ascending order, every point's new residual behind its run
DSM_HD int run_end(const int *point, int n_res, int p) { // residuals of points <= p
  int lo = 0, hi = n_res;
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (point[mid] <= p)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}
DSM_HD int old_index(int r, int point_r) { return r + point_r; }
DSM_HD int new_index(int run_end_p, int p) { return run_end_p + p; }

} // namespace adm
} // namespace dsm
