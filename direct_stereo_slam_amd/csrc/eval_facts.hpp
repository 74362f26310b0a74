// eval_facts.hpp -- the three facts that let an evaluation run its per-point stages without the checks they settle (DESIGN.md
// section 4.1, "Settled checks"): what each fact states, where it is kept, and the pose rule, written once for the kernel, the
// diagnostic entry and the host form the CPU test calls (dsm_pose_fact_host, host_capi.cpp).
//
//   template fact  per tracker and level: every listed entry has 2^-64 <= id (not NaN, zero or negative) and finite x, y; with it
//                  the bounds of the list.  Set by the kernels that write a list, from the values they hold in registers.
//   image fact     per frame buffer and level: every pixel of the plane has |I| <= 2^100, so tap differences and bilinear sums
//                  of them are finite.  Set by the kernels that build a pyramid level, from the pixels they hold in registers.
//   pose fact      per evaluation: 2^-21 <= pt2 < 2^31 for every point inside the template's bounds (pose_fact below).
//
// A fact that is not established reads as 0 and selects the general code.  Only a stale 1 could give a wrong result, so whoever
// may write a list or a plane clears its fact first (dsm_tracker::announce_*_write in dsm_internal.hpp is the one place that does).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DSM_FACT_HD __host__ __device__
#else
#define DSM_FACT_HD
#endif

namespace dsm {

constexpr int kFactLevels = 6;     // DSM_MAX_LEVELS
constexpr int kFactImageSets = 4;  // the two frame slots' front and back buffers

// Bounds are kept as the int bits of an order-preserving key of the float (ordered_key below), so that atomicMin / atomicMax on ints
// -- exact and independent of the order of arrival -- maintain them.
struct LevelFacts {
  int tpl_plain;                    // 1: the template fact holds for this level's list
  int xmin, xmax, ymin, ymax, idmax; // ordered keys; meaningful while tpl_plain is 1
  int pad0, pad1;
};
struct TrackerFacts {
  LevelFacts lv[kFactLevels];
  int img_plain[kFactImageSets][kFactLevels]; // by buffer set (TrackerDev::img_set names the set behind each frame slot)
  int force_general;                          // diagnostics: 1 = evaluations of this tracker take the general code whatever the facts
  int pad[3];
};

// float -> int whose signed order is the floats' order (-0 below +0, NaNs at the ends) and back
DSM_FACT_HD inline int ordered_key(float f) {
  union { float f; int i; } u;
  u.f = f;
  return u.i >= 0 ? u.i : u.i ^ 0x7fffffff;
}
DSM_FACT_HD inline float ordered_value(int k) {
  union { float f; int i; } u;
  u.i = k >= 0 ? k : k ^ 0x7fffffff;
  return u.f;
}
constexpr int kKeyMinInit = 0x7f800000;        // key of +inf: above every finite value
constexpr int kKeyMaxInit = (int)0x807fffffu;  // key of -inf: below every finite value

// what one template entry contributes to the template fact
DSM_FACT_HD inline bool entry_plain(float x, float y, float id) {
  const float ax = x < 0 ? -x : x, ay = y < 0 ? -y : y;
  return id >= 0x1p-64f && ax < __builtin_inff() && ay < __builtin_inff(); // (every comparison is false for a NaN)
}
// what one pixel contributes to the image fact
DSM_FACT_HD inline bool pixel_plain(float v) { return (v < 0 ? -v : v) <= 0x1p100f; }

// The pose fact of mode 0: pt2 = ((M6 x + M7 y) + M8) + t2 id over the box [xmin, xmax] x [ymin, ymax] x [0, idmax].
//   A  bounds every term's magnitude, hence every intermediate of the float sum;  lo  is the exact minimum up to rounding.
// A <= 2^30 and lo - 2^-20 A >= 2^-20: the margin 2^-20 A is sixteen times the worst rounding of the four-term sum (six operations
// of relative error 2^-24 on magnitudes <= A) and covers the rounding of lo and A themselves, so the loop's own pt2 lies in
// [2^-21, 2^31): an ordinary divisor and positive, and with id >= 2^-64 the product id * (1 / pt2) is a positive normal number
// or +inf.  Any NaN or infinity among the inputs makes A a NaN or infinite: false.  Compiled with -ffp-contract=off wherever used.
DSM_FACT_HD inline bool pose_fact(float M6, float M7, float M8, float t2, float xmin, float xmax, float ymin, float ymax, float idmax) {
  const float X = __builtin_fmaxf(__builtin_fabsf(xmin), __builtin_fabsf(xmax));
  const float Y = __builtin_fmaxf(__builtin_fabsf(ymin), __builtin_fabsf(ymax));
  const float A = ((__builtin_fabsf(M6) * X + __builtin_fabsf(M7) * Y) + __builtin_fabsf(M8)) + __builtin_fabsf(t2) * idmax;
  const float lo = ((M8 + __builtin_fminf(M6 * xmin, M6 * xmax)) + __builtin_fminf(M7 * ymin, M7 * ymax)) + __builtin_fminf(0.0f, t2 * idmax);
  return A <= 0x1p30f && lo - 0x1p-20f * A >= 0x1p-20f;
}

} // namespace dsm
