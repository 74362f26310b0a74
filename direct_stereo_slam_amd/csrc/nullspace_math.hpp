// nullspace_math.hpp -- the window's nullspaces and their pseudo-inverse as DESIGN.md section 23 states them: a frame's numeric
// nullspaces (G1, G2; FrameHessian::setStateZero restated), the nine vectors of FrontEnd::getNullspaces (G4;
// dso_helpers/FrontEndOptimize.cpp:525-574, called from solveSystem :488-494), the normalised basis (G5) and the one-sided Jacobi SVD
// behind its pseudo-inverse (G6; EnergyFunctional::orthogonalize restated).  The device kernel (nullspace_kernels.hip) and the host
// form (nullspace_host.cpp) share every expression here; each keeps its own way of walking frames, columns, rows and pairs in the
// stated order.  exp, the product and the inverse are step_math.hpp's; the logarithm is new and restates Sophus' SO3::log and SE3::log.
// IEEE double, left to right as written, no contraction (-ffp-contract=off), no fma.
#pragma once

#include <cmath>

#include "step_math.hpp"

namespace dsm {
namespace nsp {

constexpr int kCols = 7;        // pose 0-5 and scale: the columns of the basis
constexpr int kLogs = 14;       // a frame's logarithms: P of the pose columns, their M, P and M of the scale column
constexpr int kRounds = 7;      // G6: the rounds of a sweep, three disjoint pairs each
constexpr int kSweepCap = 30;   // G6
constexpr double kStep = 1e-3;  // G1: eps
constexpr double kScaleFac = 1.00001, kDivisor = 2e-3;
constexpr double kTol = 0x1p-50; // G6
constexpr double kPi = 3.141592653589793;

struct Scales { // 1.0 / scale of dsm_nullspace_params, and solver_mode_delta
  double inv_trans, inv_rot, inv_a, inv_b, delta;
};
struct UnitPoses { // G1: exp(+eps e_i) (0-5) and exp(-eps e_i) (6-11), formed once on the host with stp::se3_exp
  double p[12][7];
};

inline void unit_poses(UnitPoses &U) { // host only: keeps sincos off the device path
  for (int c = 0; c < 12; c++) {
    double xi[6] = {0, 0, 0, 0, 0, 0};
    xi[c % 6] = c < 6 ? kStep : -kStep;
    stp::se3_exp(xi, U.p[c]);
  }
}

// G1: Sophus SE3::log; the tangent is [upsilon; omega].  branch (or null): bit 0 the atan branch, bit 1 the pi branch, bit 2 tan
DSM_HD void se3_log(const double T[7], double xi[6], int *branch = nullptr) {
  const double x = T[0], y = T[1], z = T[2], w = T[3];
  const double sn = (x * x + y * y) + z * z;
  const double n = sqrt(sn);
  double f;
  int br = 0;
  if (sn < 1e-20) {
    f = 2.0 / w - (2.0 * sn) / ((w * w) * w);
  } else if (fabs(w) < 1e-10) {
    f = (w > 0.0 ? kPi : -kPi) / n;
    br = 2;
  } else {
    f = (2.0 * atan(n / w)) / n;
    br = 1;
  }
  const double theta = f * n;
  const double om[3] = {f * x, f * y, f * z};
  const double O[9] = {0.0, -om[2], om[1], om[2], 0.0, -om[0], -om[1], om[0], 0.0};
  double k;
  if (fabs(theta) < 1e-10) {
    k = 1.0 / 12.0;
  } else {
    k = (1.0 - theta / (2.0 * tan(0.5 * theta))) / (theta * theta);
    br |= 4;
  }
  if (branch) *branch = br;
  double Vi[9];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      const double o2 = (O[i * 3 + 0] * O[0 * 3 + j] + O[i * 3 + 1] * O[1 * 3 + j]) + O[i * 3 + 2] * O[2 * 3 + j];
      Vi[i * 3 + j] = ((i == j ? 1.0 : 0.0) - 0.5 * O[i * 3 + j]) + k * o2;
    }
  for (int i = 0; i < 3; i++) xi[i] = (Vi[i * 3 + 0] * T[4] + Vi[i * 3 + 1] * T[5]) + Vi[i * 3 + 2] * T[6];
  xi[3] = om[0], xi[4] = om[1], xi[5] = om[2];
}

// G1, G2: logarithm c of a frame with evaluation pose T: c < 12 log((T unit_c) T^-1); 12 and 13 the scale column's P and M
DSM_HD void frame_log(const double T[7], const UnitPoses &U, int c, double xi[6], int *branch = nullptr) {
  double Ti[7], A[7], P[7];
  stp::se3_inverse(T, Ti);
  if (c < 12) {
    double u[7];
    for (int k = 0; k < 7; k++) u[k] = U.p[c][k];
    stp::se3_mul(T, u, A);
  } else {
    for (int k = 0; k < 4; k++) A[k] = T[k];
    for (int k = 4; k < 7; k++) A[k] = c == 12 ? T[k] * kScaleFac : T[k] / kScaleFac;
  }
  stp::se3_mul(A, Ti, P);
  se3_log(P, xi, branch);
}
// G1, G2: an entry of a frame's 6 x 7 block from the same entry of its two logarithms
DSM_HD double null_entry(double p, double m) { return (p - m) / kDivisor; }
// G4: row r (0-5) of a frame's block as the nine vectors carry it
DSM_HD double scaled_entry(double v, int r, const Scales &S) { return v * (r < 3 ? S.inv_trans : S.inv_rot); }
// G3: what a frame's affB column holds; both forms evaluate it on the host, so no device expf enters
inline double affine_b(double state_zero_a, double scale_a, float exposure) { return (double)(expf((float)(state_zero_a * scale_a)) * exposure); }
// G4: the affine columns' entries of a frame's rows 6 and 7: (1, 0) and (0, aff_b) times the inverse scales
DSM_HD void affine_rows(double aff_b, const Scales &S, double A[2], double B[2]) {
  A[0] = 1.0 * S.inv_a, A[1] = 0.0 * S.inv_b, B[0] = 0.0 * S.inv_a, B[1] = aff_b * S.inv_b;
}

// the dsum over ascending row of W[i][p] W[i][q]; W is N x 7, row-major
DSM_HD double col_dot(const double *W, int N, int p, int q) {
  double s = 0.0;
  for (int i = 0; i < N; i++) s += W[i * kCols + p] * W[i * kCols + q];
  return s;
}
// G6: pair k (0-2) of round r (0-6): columns (r + k + 1) mod 7 and (r - k - 1) mod 7, the smaller index first
DSM_HD void round_pair(int r, int k, int &p, int &q) {
  const int u = (r + k + 1) % kCols, v = (r + 2 * kCols - k - 1) % kCols;
  p = u < v ? u : v, q = u < v ? v : u;
}
// G6: whether the pair with a = p.p, b = q.q, c = p.q rotates, and the rotation
DSM_HD bool rotation(double a, double b, double c, double amax, double delta, double &cs, double &sn) {
  cs = 1.0, sn = 0.0;
  if (!(fabs(c) > kTol * sqrt(a * b) && fabs(c) > (kTol * (delta * delta)) * amax)) return false;
  const double zeta = (b - a) / (2.0 * c);
  const double t = (zeta < 0.0 ? -1.0 : 1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
  cs = 1.0 / sqrt(1.0 + t * t);
  sn = cs * t;
  return true;
}
DSM_HD void rotate(double &x, double &y, double cs, double sn) {
  const double x0 = x, y0 = y;
  x = cs * x0 - sn * y0;
  y = sn * x0 + cs * y0;
}
// G6: the kept inverses and the rank from the seven column norms
DSM_HD int kept_inverses(const double sing[kCols], double delta, double inv[kCols]) {
  double smax = 0.0;
  for (int k = 0; k < kCols; k++)
    if (sing[k] > smax) smax = sing[k];
  int rank = 0;
  for (int k = 0; k < kCols; k++) {
    const bool keep = sing[k] > delta * smax;
    inv[k] = keep ? 1.0 / sing[k] : 0.0;
    rank += keep ? 1 : 0;
  }
  return rank;
}
// G6: null_pinv[k][i] from row k of V, row i of the rotated matrix and the kept inverses
DSM_HD double pinv_entry(const double *Vk, const double *Wi, const double *inv) {
  double s = 0.0;
  for (int j = 0; j < kCols; j++) s += (Vk[j] * inv[j]) * (Wi[j] * inv[j]);
  return s;
}

} // namespace nsp
} // namespace dsm
