// icp_internal.hpp -- what the host side (dsm_icp_batch) and the kernels (icp_kernels.hip) of the ICP fallback share: the job
// descriptors, the per-job state the device keeps between iterations, and the Umeyama step with its 3x3 SVD.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace dsm {

constexpr int kIcpThreads = 256;        // one workgroup: the step, prep and fitness kernels of a job; one source block of the search
constexpr int kIcpTile = 256;           // target points staged in LDS per round of the nearest-neighbour scan
constexpr int kIcpIterationsLimit = 64; // largest max_iterations dsm_icp_batch accepts (the size of IcpState::corr)
constexpr int kIcpSvdSweeps = 16;       // sweeps of the one-sided Jacobi SVD at most (3x3 double: 4 to 6 in practice)

// end states: the values of PCL's DefaultConvergenceCriteria::ConvergenceState, plus "empty" (D3); 0 = still iterating
constexpr int kIcpRunning = 0, kIcpIterations = 1, kIcpTransform = 2, kIcpAbsMse = 3, kIcpNoCorrespondences = 5, kIcpEmpty = 6;

struct IcpJobDev {
  int n_src, n_tgt;
  long long off_src, off_tgt; // first row of the job in the call's source / target arrays
  double guess[16];           // tfm_target_source on entry, row-major
};

// one workgroup of the nearest-neighbour scan: 256 source points [src0, src0 + 256) of `job` against targets [tgt0, tgt1)
struct IcpNnBlock {
  int job, src0, tgt0, tgt1;
};

// per job, on the device for the whole call and read back once at its end
struct IcpState {
  float final_tf[16]; // PCL's final_transformation_ (Matrix4f), row-major
  double prev_mse;    // correspondences_prev_mse_ (DBL_MAX before the first iteration)
  double fitness;     // getFitnessScore() before its cast to float
  int state;          // kIcp*
  int iterations;     // nr_iterations_
  int searches;       // correspondence searches run: iterations, plus one if the last one found fewer than 3 pairs
  int pad;
  int corr[kIcpIterationsLimit]; // kept pairs of each search
};

// Sigma = U diag(s) V^T by one-sided (Hestenes) Jacobi in double: columns of A = Sigma are rotated pairwise until they are orthogonal,
// V accumulates the rotations, s = the column norms, in DESCENDING order as Eigen's JacobiSVD returns them.  A column whose norm is
// below 1e-13 of the largest (rank-deficient Sigma: planar or collinear pairs, or Sigma = 0) has no direction of its own: U is
// completed there by a unit vector orthogonal to the earlier columns (the coordinate axis least aligned with u0, then u0 x u1).
// Deterministic: a fixed operation order and at most kIcpSvdSweeps sweeps, the same on every job and on host and device.
__host__ __device__ inline void icp_svd3(const double S[9], double U[9], double s[3], double V[9]) {
  double A[9];
  for (int i = 0; i < 9; i++) A[i] = S[i], V[i] = (i % 4 == 0) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < kIcpSvdSweeps; sweep++) {
    bool rotated = false;
    for (int p = 0; p < 2; p++)
      for (int q = p + 1; q < 3; q++) {
        double alpha = 0, beta = 0, gamma = 0;
        for (int k = 0; k < 3; k++) {
          alpha += A[k * 3 + p] * A[k * 3 + p];
          beta += A[k * 3 + q] * A[k * 3 + q];
          gamma += A[k * 3 + p] * A[k * 3 + q];
        }
        if (!(fabs(gamma) > 1e-15 * sqrt(alpha * beta))) continue; // this pair is orthogonal (or a column is zero)
        rotated = true;
        const double zeta = (beta - alpha) / (2.0 * gamma);
        const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / sqrt(1.0 + t * t), sn = c * t;
        for (int k = 0; k < 3; k++) {
          const double ap = A[k * 3 + p], aq = A[k * 3 + q];
          A[k * 3 + p] = c * ap - sn * aq;
          A[k * 3 + q] = sn * ap + c * aq;
          const double vp = V[k * 3 + p], vq = V[k * 3 + q];
          V[k * 3 + p] = c * vp - sn * vq;
          V[k * 3 + q] = sn * vp + c * vq;
        }
      }
    if (!rotated) break;
  }
  double nrm[3];
  for (int c = 0; c < 3; c++) nrm[c] = sqrt(A[c] * A[c] + A[3 + c] * A[3 + c] + A[6 + c] * A[6 + c]);
  // descending norms (a stable sorting network; constant indices only, so that nothing goes to scratch memory on the device)
  for (int pass = 0; pass < 3; pass++) {
    const int p = pass == 1 ? 1 : 0, q = p + 1;
    if (nrm[p] < nrm[q]) {
      const double tn = nrm[p];
      nrm[p] = nrm[q], nrm[q] = tn;
      for (int k = 0; k < 3; k++) {
        const double ta = A[k * 3 + p], tv = V[k * 3 + p];
        A[k * 3 + p] = A[k * 3 + q], A[k * 3 + q] = ta;
        V[k * 3 + p] = V[k * 3 + q], V[k * 3 + q] = tv;
      }
    }
  }
  for (int c = 0; c < 3; c++) s[c] = nrm[c];
  const double tol = 1e-13 * s[0];
  for (int c = 0; c < 3; c++) {
    if (s[c] > tol && s[c] > 0) {
      for (int r = 0; r < 3; r++) U[r * 3 + c] = A[r * 3 + c] / s[c];
    } else if (c == 0) {
      for (int r = 0; r < 3; r++) U[r * 3] = r == 0 ? 1.0 : 0.0;
    } else if (c == 1) {
      const double a0 = fabs(U[0]), a1 = fabs(U[3]), a2 = fabs(U[6]);
      const int ax = (a1 < a0 && a1 <= a2) ? 1 : (a2 < a0 && a2 < a1) ? 2 : 0;
      const double d = ax == 0 ? U[0] : ax == 1 ? U[3] : U[6];
      double e[3];
      for (int r = 0; r < 3; r++) e[r] = (r == ax ? 1.0 : 0.0) - d * U[r * 3];
      const double ne = sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
      for (int r = 0; r < 3; r++) U[r * 3 + 1] = e[r] / ne;
    } else {
      U[2] = U[3] * U[7] - U[6] * U[4];
      U[5] = U[6] * U[1] - U[0] * U[7];
      U[8] = U[0] * U[4] - U[3] * U[1];
    }
  }
}

__host__ __device__ inline double icp_det3(const double M[9]) {
  return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
}

// Eigen::umeyama(src, dst, with_scaling = false) from the cross-covariance Sigma = (1/n) sum dst_c src_c^T and the means (P4):
// R = U diag(1, 1, +-1) V^T, the sign negative iff det(U) det(V) < 0; t = dst_mean - R src_mean.  All in double (D1).
__host__ __device__ inline void icp_umeyama(const double Sigma[9], const double src_mean[3], const double dst_mean[3], double R[9], double t[3]) {
  double U[9], s[3], V[9];
  icp_svd3(Sigma, U, s, V);
  const double d = icp_det3(U) * icp_det3(V) < 0 ? -1.0 : 1.0;
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) R[r * 3 + c] = (U[r * 3] * V[c * 3] + U[r * 3 + 1] * V[c * 3 + 1]) + d * U[r * 3 + 2] * V[c * 3 + 2];
  for (int r = 0; r < 3; r++) t[r] = dst_mean[r] - ((R[r * 3] * src_mean[0] + R[r * 3 + 1] * src_mean[1]) + R[r * 3 + 2] * src_mean[2]);
}

} // namespace dsm
