// point_math.hpp -- what the arithmetic of the three point calls has in common (activation: DESIGN.md section 12, immature points:
// section 13, trace: section 14): the residual pattern, the projection of a host pixel into a target and the bilinear sample of an
// intensity plane with its gradients.  Every device kernel and every host form (points_host.cpp) takes them from here, so that all
// evaluate the same expression tree.  float32 throughout, no contraction (-ffp-contract=off), no fmaf.
#pragma once

#if defined(__HIPCC__)
#define DSM_HD __host__ __device__ __forceinline__
#else
#define DSM_HD inline
#endif

namespace dsm {
namespace pt {

// staticPattern[8] (UPSTREAM-DSO settings.cpp), U2
DSM_HD void pattern(int i, int &dx, int &dy) {
  constexpr signed char DX[8] = {0, -1, 1, -2, 0, 2, -1, 0}, DY[8] = {-2, -1, -1, 0, 0, 0, 1, 2};
  dx = DX[i], dy = DY[i];
}

struct Vec3 {
  float x, y, z;
};

// M (u, v, 1) for a row-major 3 x 3 M (K R K^-1, or PRE_RTll on a normalised pixel): each component (m0 u + m1 v) + m2
DSM_HD Vec3 rotate_uv1(const float *M, float u, float v) {
  return Vec3{(M[0] * u + M[1] * v) + M[2], (M[3] * u + M[4] * v) + M[5], (M[6] * u + M[7] * v) + M[8]};
}
// ... + t idepth: with rotate_uv1, ptp = KRKi (u, v, 1) + Kt idepth as ((m0 u + m1 v) + m2) + t idepth
DSM_HD Vec3 add_translation(const Vec3 &p, const float *t, float idepth) {
  return Vec3{p.x + t[0] * idepth, p.y + t[1] * idepth, p.z + t[2] * idepth};
}

DSM_HD float grad_fix(float d) { return __builtin_isfinite(d) ? d : 0.0f; } // makeImages: a non-finite gradient is zero

// getInterpolatedElement33 at (x, y) on texels (I, 0.5 (I[x+1] - I[x-1]), 0.5 (I[y+1] - I[y-1])), ix = (int)x, iy = (int)y
struct Tex4 { // the four texels of an intensity sample: rows iy (b) and iy + 1 (c), columns ix (1) and ix + 1 (2)
  float b1, b2, c1, c2;
};
struct Tex12 { // ... and the eight more of its gradients: rows iy - 1 .. iy + 2 (a .. d), columns ix - 1 .. ix + 2 (0 .. 3)
  float a0, a1, b0, b1, b2, b3, c0, c1, c2, c3, d0, d1;
};

DSM_HD Tex4 load4(const float *I, int w, float x, float y) { // the caller keeps ix in [0, w - 2], iy in [0, h - 2]
  const float *p = I + ((long long)(int)y * w + (int)x);
  return Tex4{p[0], p[1], p[w], p[w + 1]};
}
DSM_HD Tex12 load12(const float *I, int w, float x, float y) { // the caller keeps ix in [1, w - 3], iy in [1, h - 3]
  const float *p = I + ((long long)(int)y * w + (int)x);
  return Tex12{p[-w], p[-w + 1], p[-1], p[0], p[1], p[2], p[w - 1], p[w], p[w + 1], p[w + 2], p[2 * w], p[2 * w + 1]};
}

// U6, channel 0
DSM_HD float interp_I(const Tex4 &T, float x, float y) {
  const int ix = (int)x, iy = (int)y;
  const float fdx = x - ix, fdy = y - iy, dxdy = fdx * fdy;
  const float w11 = dxdy, w01 = fdy - dxdy, w10 = fdx - dxdy, w00 = 1 - fdx - fdy + dxdy;
  return ((w11 * T.c2 + w01 * T.c1) + w10 * T.b2) + w00 * T.b1;
}
// U6, all three channels
DSM_HD void interp_Ig(const Tex12 &T, float x, float y, float &hI, float &hx, float &hy) {
  const int ix = (int)x, iy = (int)y;
  const float fdx = x - ix, fdy = y - iy, dxdy = fdx * fdy;
  const float w11 = dxdy, w01 = fdy - dxdy, w10 = fdx - dxdy, w00 = 1 - fdx - fdy + dxdy;
  hI = ((w11 * T.c2 + w01 * T.c1) + w10 * T.b2) + w00 * T.b1;
  const float gx00 = grad_fix(0.5f * (T.b2 - T.b0)), gx10 = grad_fix(0.5f * (T.b3 - T.b1)), gx01 = grad_fix(0.5f * (T.c2 - T.c0)),
              gx11 = grad_fix(0.5f * (T.c3 - T.c1));
  const float gy00 = grad_fix(0.5f * (T.c1 - T.a0)), gy10 = grad_fix(0.5f * (T.c2 - T.a1)), gy01 = grad_fix(0.5f * (T.d0 - T.b1)),
              gy11 = grad_fix(0.5f * (T.d1 - T.b2));
  hx = ((w11 * gx11 + w01 * gx01) + w10 * gx10) + w00 * gx00;
  hy = ((w11 * gy11 + w01 * gy01) + w10 * gy10) + w00 * gy00;
}

} // namespace pt
} // namespace dsm
