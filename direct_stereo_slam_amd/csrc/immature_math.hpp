// immature_math.hpp -- one pattern pixel of ImmaturePoint::linearizeResidual as DESIGN.md section 13 states it (U2-U8): the one
// piece of arithmetic the device kernel (immature_kernels.hip) and the host form (host_capi.cpp) share, so that both evaluate the
// same expression tree.  float32 throughout, no contraction (-ffp-contract=off), no fmaf.
#pragma once

#if defined(__HIPCC__)
#define DSM_IMM_HD __host__ __device__ __forceinline__
#else
#define DSM_IMM_HD inline
#endif

namespace dsm {
namespace imm {

enum { RES_IN = 0, RES_OOB = 1, RES_OUTLIER = 2 }; // DSM_RES_*

// staticPattern[8] (UPSTREAM-DSO settings.cpp), U2
DSM_IMM_HD void pattern(int i, int &dx, int &dy) {
  constexpr signed char DX[8] = {0, -1, 1, -2, 0, 2, -1, 0}, DY[8] = {-2, -1, -1, 0, 0, 0, 1, 2};
  dx = DX[i], dy = DY[i];
}

struct Cam {
  float fx, fy, cx, cy, fxi, fyi;
  int w, h;
};

DSM_IMM_HD float grad_fix(float d) { return __builtin_isfinite(d) ? d : 0.0f; } // makeImages: a non-finite gradient is zero

// Pattern pixel (dx, dy) of the point (u, v) at inverse depth idepth against the frame plane I, with the pair's PRE_RTll R (row-major),
// PRE_tTll t and PRE_aff_mode aff.  False: the pixel fails (U4: projection or bounds; U6: non-finite intensity) and nothing is
// written.  True: tE, tH, tb are the pixel's terms of the energy, Hdd and bd (U7, U8); the caller adds them in pattern order.
DSM_IMM_HD bool tap(const Cam &C, const float *I, const float *R, const float *t, const float *aff, float u, float v, int dx, int dy,
                    float idepth, float color, float wt, float huber, float &tE, float &tH, float &tb) {
  const float k0 = ((u + (float)dx) - C.cx) * C.fxi, k1 = ((v + (float)dy) - C.cy) * C.fyi;
  const float p0 = ((R[0] * k0 + R[1] * k1) + R[2]) + t[0] * idepth;
  const float p1 = ((R[3] * k0 + R[4] * k1) + R[5]) + t[1] * idepth;
  const float p2 = ((R[6] * k0 + R[7] * k1) + R[8]) + t[2] * idepth;
  const float drescale = 1.0f / p2;
  if (!(drescale > 0.0f)) return false;
  const float up = p0 * drescale, vp = p1 * drescale;
  const float Ku = up * C.fx + C.cx, Kv = vp * C.fy + C.cy;
  if (!(Ku > 1.1f && Kv > 1.1f && Ku < (float)(C.w - 3) && Kv < (float)(C.h - 3))) return false;
  // getInterpolatedElement33 on texels (I, 0.5 (I[x+1] - I[x-1]), 0.5 (I[y+1] - I[y-1])): ix in [1, w - 4], iy in [1, h - 4], so the
  // twelve texels read lie in columns ix - 1 .. ix + 2 and rows iy - 1 .. iy + 2 of the plane
  const int ix = (int)Ku, iy = (int)Kv, w = C.w;
  const float fdx = Ku - ix, fdy = Kv - iy, dxdy = fdx * fdy;
  const float w11 = dxdy, w01 = fdy - dxdy, w10 = fdx - dxdy, w00 = 1 - fdx - fdy + dxdy;
  const float *p = I + ((long long)iy * w + ix);
  const float a0 = p[-w], a1 = p[-w + 1];
  const float b0 = p[-1], b1 = p[0], b2 = p[1], b3 = p[2];
  const float c0 = p[w - 1], c1 = p[w], c2 = p[w + 1], c3 = p[w + 2];
  const float d0 = p[2 * w], d1 = p[2 * w + 1];
  const float hI = ((w11 * c2 + w01 * c1) + w10 * b2) + w00 * b1;
  if (!__builtin_isfinite(hI)) return false;
  const float gx00 = grad_fix(0.5f * (b2 - b0)), gx10 = grad_fix(0.5f * (b3 - b1)), gx01 = grad_fix(0.5f * (c2 - c0)), gx11 = grad_fix(0.5f * (c3 - c1));
  const float gy00 = grad_fix(0.5f * (c1 - a0)), gy10 = grad_fix(0.5f * (c2 - a1)), gy01 = grad_fix(0.5f * (d0 - b1)), gy11 = grad_fix(0.5f * (d1 - b2));
  const float hx = ((w11 * gx11 + w01 * gx01) + w10 * gx10) + w00 * gx00;
  const float hy = ((w11 * gy11 + w01 * gy01) + w10 * gy10) + w00 * gy00;
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

} // namespace imm
} // namespace dsm
