// select_math.hpp -- the expressions of the pixel selection and of the ImmaturePoint constructor that the
// device kernels (select_kernels.hip) and the host form (dsm_select_pixels_host, points_host.cpp) share, so that both evaluate the same
// expression tree.  float32 throughout, no contraction (-ffp-contract=off), no fmaf; every cast to int is of a value that fits.
#pragma once
#include <cmath>

#include "../../include/dsm_hotpath.h"
#include "point_math.hpp"

namespace dsm {
namespace sel {

struct Dir {
  float x, y;
};
// P6: the 16 directions of PixelSelector::select, in upstream's order
DSM_HD Dir direction(int d) {
  constexpr float X[16] = {0.f,     0.3827f, 0.1951f, 0.9239f, 0.7071f, 0.3827f, 0.8315f, 0.8315f,
                           0.5556f, 0.9808f, 0.9239f, 0.7071f, 0.5556f, 0.9808f, 1.f,     0.1951f};
  constexpr float Y[16] = {1.f,      0.9239f, 0.9808f,  0.3827f,  0.7071f, -0.9239f, 0.5556f, -0.5556f,
                           -0.8315f, 0.1951f, -0.3827f, -0.7071f, 0.8315f, -0.1951f, 0.f,     -0.9808f};
  return Dir{X[d], Y[d]};
}
DSM_HD float dir_norm(float gx, float gy, Dir d) { return fabsf(gx * d.x + gy * d.y); }

// P1: central differences of an intensity plane on the flat index, as dip_gradients (frame_kernels.hip) forms them: zero on rows 0 and
// hl - 1; in columns 0 and wl - 1 of the other rows the x difference wraps into the neighbouring row (p[-1] is the last pixel of the
// row above, p[1] the first of the row below), both inside the plane
DSM_HD void gradient(const float *I, int wl, int hl, int x, int y, float &gx, float &gy) {
  gx = gy = 0.f;
  if (y < 1 || y > hl - 2) return;
  const float *p = I + ((long long)y * wl + x);
  gx = pt::grad_fix(0.5f * (p[1] - p[-1]));
  gy = pt::grad_fix(0.5f * (p[wl] - p[-wl]));
}
// P1: the squared gradient, weighted by the slope of the inverse response at the pixel's intensity if b_inv is given
DSM_HD float abs_grad(const float *I, int wl, int hl, int x, int y, const float *b_inv, float &gx, float &gy) {
  gradient(I, wl, hl, x, y, gx, gy);
  if (y < 1 || y > hl - 2) return 0.f;
  float ag = gx * gx + gy * gy;
  if (b_inv) {
    const float c = I[(long long)y * wl + x] + 0.5f;
    const int ci = !(c >= 5.f) ? 5 : (c > 250.f ? 250 : (int)c);
    const float gw = b_inv[ci + 1] - b_inv[ci];
    ag = ag * (gw * gw);
  }
  return ag;
}
DSM_HD float abs_grad(const float *I, int wl, int hl, int x, int y, const float *b_inv) {
  float gx, gy;
  return abs_grad(I, wl, hl, x, y, b_inv, gx, gy);
}

// P2: the pixels of a 32 x 32 block that its histogram counts, and their bin (the count of all is bin 0)
DSM_HD bool in_histogram(int it, int jt, int w, int h) { return it >= 1 && jt >= 1 && it <= w - 2 && jt <= h - 2; }
DSM_HD int hist_bin(float ag0) {
  const float s = sqrtf(ag0);
  return (s < 48.f ? (int)s : 48) + 1;
}
// P2: computeHistQuantil over 50 bins; bins 50 .. 90 count as zero
DSM_HD int hist_quantile(const int *hist, float cut) {
  int th = (int)((float)hist[0] * cut + 0.5f);
  for (int i = 0; i < 49; i++) {
    th -= hist[i + 1];
    if (th < 0) return i;
  }
  return 90;
}
// P3: the squared mean of the thresholds of a block and its existing neighbours, summed in upstream's order
DSM_HD float smoothed_threshold(const float *ths, int w32, int h32, int x, int y) {
  int num = 0;
  float sum = 0.f;
  if (x > 0) {
    if (y > 0) num++, sum += ths[x - 1 + (y - 1) * w32];
    if (y < h32 - 1) num++, sum += ths[x - 1 + (y + 1) * w32];
    num++, sum += ths[x - 1 + y * w32];
  }
  if (x < w32 - 1) {
    if (y > 0) num++, sum += ths[x + 1 + (y - 1) * w32];
    if (y < h32 - 1) num++, sum += ths[x + 1 + (y + 1) * w32];
    num++, sum += ths[x + 1 + y * w32];
  }
  if (y > 0) num++, sum += ths[x + (y - 1) * w32];
  if (y < h32 - 1) num++, sum += ths[x + (y + 1) * w32];
  num++, sum += ths[x + y * w32];
  return (sum / (float)num) * (sum / (float)num);
}
// P3: the block of a pixel, clamped into the table
DSM_HD int threshold_index(int xf, int yf, int w32, int h32) {
  const int bx = xf >> 5, by = yf >> 5;
  return (bx < w32 ? bx : w32 - 1) + (by < h32 ? by : h32 - 1) * w32;
}

// P5: the pixels select() looks at
DSM_HD bool in_scan_window(int xf, int yf, int w, int h) { return xf >= 4 && xf < w - 5 && yf >= 4 && yf <= h - 4; }

// P4: what the squared gradient of level l must exceed, from the smoothed threshold t0 of the pixel's block
DSM_HD float level_threshold(float t0, int l, const dsm_select_params &S) {
  const float dw = S.grad_downweight_per_level, t1 = t0 * dw, t2 = t1 * (dw * dw);
  return (l == 0 ? t0 : l == 1 ? t1 : t2) * S.th_factor;
}
// P8, P9: the squared gradient of level l = 1, 2 (plane Il of the level-0 size w x h shifted by l) that the level-0 pixel reads
DSM_HD float coarse_abs_grad(const float *Il, int w, int h, int l, int xf, int yf, const float *b_inv) {
  const float s = l == 1 ? 0.5f : 0.25f, o = l == 1 ? 0.25f : 0.125f;
  return abs_grad(Il, w >> l, h >> l, (int)((float)xf * s + o), (int)((float)yf * s + o), b_inv);
}

// What select() knows of one pixel: whether it passes the threshold of each level (P4) and the gradient its dirNorm is formed from.
struct Pixel {
  bool above[3];
  float ag[3], gx, gy;
};
DSM_HD Pixel pixel(const float *I0, const float *I1, const float *I2, int w, int h, int xf, int yf, const float *b_inv, float t0,
                   const dsm_select_params &S) {
  Pixel P;
  P.ag[0] = abs_grad(I0, w, h, xf, yf, b_inv, P.gx, P.gy);
  P.ag[1] = coarse_abs_grad(I1, w, h, 1, xf, yf, b_inv);
  P.ag[2] = coarse_abs_grad(I2, w, h, 2, xf, yf, b_inv);
  for (int l = 0; l < 3; l++) P.above[l] = P.ag[l] > level_threshold(t0, l, S);
  return P;
}
// P6: what a pixel is ranked by on level l under direction d
DSM_HD float rank_value(float gx, float gy, float ag_l, int d, const dsm_select_params &S) {
  return S.select_direction_distribution ? dir_norm(gx, gy, direction(d)) : ag_l;
}

// P10: after a pass with n2 + n3 + n4 hits at potential pot
struct Adapt {
  float quot;
  int ideal;    // the potential the job leaves with if this was its last pass (P12)
  int next_pot; // > 0: select again at this potential
};
DSM_HD Adapt adapt(int n2, int n3, int n4, float density, int pot, int recursions_left) {
  Adapt A;
  const float have = (float)(n2 + n3 + n4);
  A.quot = density / have;
  const float K = have * (float)(pot + 1) * (float)(pot + 1);
  const float r = sqrtf(K / density) - 1.f;
  A.ideal = r >= (float)DSM_SELECT_MAX_POTENTIAL ? DSM_SELECT_MAX_POTENTIAL : (int)r;
  if (A.ideal < 1) A.ideal = 1;
  A.next_pot = 0;
  if (recursions_left > 0 && A.quot > 1.25f && pot > 1)
    A.next_pot = A.ideal >= pot ? pot - 1 : A.ideal;
  else if (recursions_left > 0 && A.quot < 0.25f)
    A.next_pot = A.ideal <= pot ? (pot < DSM_SELECT_MAX_POTENTIAL ? pot + 1 : pot) : A.ideal;
  return A;
}
// P11: whether the map is thinned, and the byte a random number must not exceed
DSM_HD bool thinning(float quot, unsigned char &char_th) {
  if (!(quot < 0.95f)) return false;
  char_th = (unsigned char)(255.f * quot);
  return true;
}

// P13: the pixels the point loop visits
DSM_HD bool in_point_window(int x, int y, int w, int h, int pad) { return y >= pad + 1 && y < h - pad - 2 && x >= pad + 1 && x < w - pad - 2; }

// P14: the ImmaturePoint constructor at the integer pixel (x, y) of the point window; false: the point is dropped
struct NewPoint {
  float energy_th, grad_h[4], color[8], weights[8];
};
DSM_HD bool construct(const float *I0, int w, int h, int x, int y, const dsm_select_params &S, NewPoint &P) {
  P.grad_h[0] = P.grad_h[1] = P.grad_h[2] = P.grad_h[3] = 0.f;
  for (int k = 0; k < 8; k++) {
    int dx, dy;
    pt::pattern(k, dx, dy);
    P.color[k] = I0[(long long)(y + dy) * w + (x + dx)];
    if (!__builtin_isfinite(P.color[k])) return false;
    float gx, gy;
    gradient(I0, w, h, x + dx, y + dy, gx, gy);
    P.grad_h[0] += gx * gx, P.grad_h[1] += gx * gy, P.grad_h[2] += gx * gy, P.grad_h[3] += gy * gy;
    P.weights[k] = sqrtf(S.outlier_th_sum_component / (S.outlier_th_sum_component + (gx * gx + gy * gy)));
  }
  P.energy_th = (8.f * S.outlier_th) * (S.overall_energy_th_weight * S.overall_energy_th_weight);
  return __builtin_isfinite(P.energy_th);
}

} // namespace sel
} // namespace dsm
