// linearize_math.hpp -- PointFrameResidual::linearize as DESIGN.md section 16 states it (L2-L7) and the relative baseline of B3: the
// centre projection at the linearisation point, the geometric Jacobians, one pattern pixel with its twelve terms, and the verdict.
// The device kernel (linearize_kernels.hip) and the host form (points_host.cpp) share them, so that both evaluate one expression
// tree; each keeps its own way of adding a residual's terms in pattern order.  float32 throughout, no contraction
// (-ffp-contract=off), no fmaf; divisions and square roots are the correctly rounded ones.
#pragma once

#include "point_math.hpp"

namespace dsm {
namespace lin {

enum { RES_IN = 0, RES_OOB = 1, RES_OUTLIER = 2 }; // DSM_RES_*

// a RawResidualJacobian row (L8): 74 floats; the 2 x 2 blocks row-major (00, 01, 10, 11)
enum { J_RESF = 0, J_PDXI = 8, J_PDC = 20, J_PDD = 28, J_IDX = 30, J_ABF = 46, J_IDX2 = 62, J_ABJIDX = 66, J_AB2 = 70, J_FLOATS = 74 };
// the twelve sums of L6, in the order of the statement
enum { S_E = 0, S_XX, S_YY, S_XY, S_AX, S_AY, S_BX, S_BY, S_AA, S_AB, S_BB, S_WJI2, N_SUMS };
constexpr int kGeoFloats = 22; // Jpdxi[2][6], Jpdc[2][4], Jpdd[2]: a row's floats 8 .. 29, the same for the eight pixels

struct Cam {
  float fx, fy, cx, cy, fxi, fyi;
  int w, h;
};

struct Settings { // of dsm_linearize_params, what a residual reads
  float huber, c, scale_idepth, scale_f, scale_c;
};

DSM_HD bool in_image(const Cam &C, float Ku, float Kv) { return Ku > 1.1f && Kv > 1.1f && Ku < (float)(C.w - 3) && Kv < (float)(C.h - 3); }

// L2: the centre at the linearisation point (PRE_RTll_0 R, PRE_tTll_0 t, idepth_zero_scaled).  False: the projection fails.
struct Centre {
  float kx, ky;         // KliP
  float drescale, up, vp; // u', v'
  float Ku, Kv, new_idepth;
};
DSM_HD bool centre(const Cam &C, const float *R, const float *t, float u, float v, float idepth_zero, Centre &c) {
  c.kx = (u - C.cx) * C.fxi, c.ky = (v - C.cy) * C.fyi;
  const pt::Vec3 p = pt::add_translation(pt::rotate_uv1(R, c.kx, c.ky), t, idepth_zero);
  c.drescale = 1.0f / p.z;
  c.new_idepth = idepth_zero * c.drescale;
  if (!(c.drescale > 0.0f)) return false;
  c.up = p.x * c.drescale, c.vp = p.y * c.drescale;
  c.Ku = c.up * C.fx + C.cx, c.Kv = c.vp * C.fy + C.cy;
  return in_image(C, c.Ku, c.Kv);
}

// L3: G = Jpdxi[0][0..5], Jpdxi[1][0..5], Jpdc[0][0..3], Jpdc[1][0..3], Jpdd[0..1]
DSM_HD void geometric(const Cam &C, const float *R, const float *T, const Centre &c, const Settings &S, float *G) {
  const float dr = c.drescale, up = c.up, vp = c.vp, id = c.new_idepth;
  G[0] = id * C.fx, G[1] = 0.0f, G[2] = (-id * up) * C.fx, G[3] = (-up * vp) * C.fx, G[4] = (1 + up * up) * C.fx, G[5] = (-vp) * C.fx;
  G[6] = 0.0f, G[7] = id * C.fy, G[8] = (-id * vp) * C.fy, G[9] = (-(1 + vp * vp)) * C.fy, G[10] = (up * vp) * C.fy, G[11] = up * C.fy;
  const float cx2 = dr * (R[6] * up - R[0]);
  const float cx3 = ((C.fx * dr) * (R[7] * up - R[1])) * C.fyi;
  const float cy2 = ((C.fy * dr) * (R[6] * vp - R[3])) * C.fxi;
  const float cy3 = dr * (R[7] * vp - R[4]);
  G[12] = (c.kx * cx2 + up) * S.scale_f, G[13] = (c.ky * cx3) * S.scale_f, G[14] = (cx2 + 1) * S.scale_c, G[15] = cx3 * S.scale_c;
  G[16] = (c.kx * cy2) * S.scale_f, G[17] = (c.ky * cy3 + vp) * S.scale_f, G[18] = cy2 * S.scale_c, G[19] = (cy3 + 1) * S.scale_c;
  G[20] = ((dr * (T[0] - T[2] * up)) * S.scale_idepth) * C.fx;
  G[21] = ((dr * (T[1] - T[2] * vp)) * S.scale_idepth) * C.fy;
}

// L4-L6 for one pattern pixel at the current state (PRE_KRKiTll M, PRE_KtTll Kt, idepth_scaled).  False: the pixel fails (bounds or a
// non-finite intensity); Ku, Kv are set whenever the projection was formed.  True: the row entries of the pixel and its twelve terms
// T (S_*), which the caller adds in pattern order starting from +0.0f.
struct Pixel {
  float Ku, Kv;
  float resF, gx, gy, ja, jb; // resF, JIdx[0], JIdx[1], JabF[0], JabF[1] of the pixel (before zero_jab_*)
  float T[N_SUMS];
};
DSM_HD bool pixel(const Cam &C, const float *I, const float *M, const float *Kt, const float *aff, float b0, float u, float v, int dx, int dy,
                  float idepth, float color, float wt, const Settings &S, Pixel &P) {
  const pt::Vec3 p = pt::add_translation(pt::rotate_uv1(M, u + (float)dx, v + (float)dy), Kt, idepth);
  P.Ku = p.x / p.z, P.Kv = p.y / p.z;
  if (!in_image(C, P.Ku, P.Kv)) return false;
  // ix in [1, w - 4], iy in [1, h - 4]: the twelve texels lie in the plane
  float hI, hx, hy;
  pt::interp_Ig(pt::load12(I, C.w, P.Ku, P.Kv), P.Ku, P.Kv, hI, hx, hy);
  if (!__builtin_isfinite(hI)) return false;
  const float r = hI - (aff[0] * color + aff[1]);
  const float drdA = color - b0;
  float w = __builtin_sqrtf(S.c / (S.c + (hx * hx + hy * hy)));
  w = 0.5f * (w + wt);
  const float ar = __builtin_fabsf(r);
  float hw = ar < S.huber ? 1.0f : S.huber / ar;
  P.T[S_E] = ((((w * w) * hw) * r) * r) * (2 - hw);
  if (hw < 1) hw = __builtin_sqrtf(hw);
  hw = hw * w;
  const float gx = hx * hw, gy = hy * hw, ja = drdA * hw;
  P.resF = r * hw, P.gx = gx, P.gy = gy, P.ja = ja, P.jb = hw;
  P.T[S_XX] = gx * gx, P.T[S_YY] = gy * gy, P.T[S_XY] = gx * gy;
  P.T[S_AX] = ja * gx, P.T[S_AY] = ja * gy, P.T[S_BX] = hw * gx, P.T[S_BY] = hw * gy;
  P.T[S_AA] = ((drdA * drdA) * hw) * hw, P.T[S_AB] = ja * hw, P.T[S_BB] = hw * hw;
  P.T[S_WJI2] = (hw * hw) * (gx * gx + gy * gy);
  return true;
}

// L7: E becomes new_energy; returns the new state
DSM_HD int verdict(float &E, float wJI2, float th_host, float th_target) {
  const float th = th_host > th_target ? th_host : th_target;
  if (E > th || wJI2 < 2) {
    E = th;
    return RES_OUTLIER;
  }
  return RES_IN;
}

// B3: the relative baseline of a kept new residual
DSM_HD float rel_baseline(const float *M, const float *Kt, float u, float v, float idepth) {
  const pt::Vec3 inf = pt::rotate_uv1(M, u, v), p = pt::add_translation(inf, Kt, idepth);
  const float dx = inf.x / inf.z - p.x / p.z, dy = inf.y / inf.z - p.y / p.z;
  return (float)(0.01 * (double)__builtin_sqrtf(dx * dx + dy * dy));
}

} // namespace lin
} // namespace dsm
