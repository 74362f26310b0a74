// nullspace_kernels.hip -- what FrontEnd::solveSystem builds before every solve (dso_helpers/FrontEndOptimize.cpp:488-494): the frames'
// numeric nullspaces, the nine vectors of getNullspaces (:525-574), the normalised basis of the pose and scale vectors and its
// pseudo-inverse, on the device for the windows of many sequences in one call.  Semantics: G1-G7 and V of DESIGN.md section 23.
//
// One dsm_window_nullspace_batch = one staged copy in the call arena (call_arena.hpp), ONE launch, one read-back:
//   nsp_kernel  one 256-lane workgroup per job.
//     A  lane f 14 + c forms logarithm c of frame f (6 P, 6 M, 2 for the scale column: 224 lanes at 16 frames); the twelve poses
//        exp(+-eps e_i) are kernel arguments formed on the host, so no sincos runs here.  Through LDS, lane f 7 + i forms column i of
//        the frame's block (G1, G2); the lanes then lay out the nine vectors (G4) and the N x 7 working matrix in LDS.
//     B  lanes k < 7: one chain per column (G5); every lane divides its entries.
//     C  the one-sided Jacobi SVD (G6) on the matrix and V in LDS.  A round's three pairs are disjoint, so nine lanes form their nine
//        inner products side by side, three lanes form the rotations, and lane i rotates row i (lanes N .. N + 6 the rows of V).
//        The matrix stays in LDS because the pair's columns are run-time values: a per-lane array indexed by them would be scratch.
// Every result is one sequential chain in one lane, independent of the launch geometry and of the other jobs; the sweep cap bounds the
// only loop whose trip count depends on the data.  No scratch, no atomics, no wait on another workgroup.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "call_arena.hpp"
#include "nullspace_launch.hpp"

using namespace dsm;

namespace {

constexpr int kBlock = 256;
constexpr int kMaxF = DSM_WINDOW_MAX_FRAMES, kMaxN = 4 + 8 * kMaxF;
static_assert(kMaxF * nsp::kLogs <= kBlock && kMaxN + nsp::kCols <= kBlock, "one lane per logarithm, and per row of the matrix and of V");

struct NspJob {
  int n, N;
  // doubles into the staged doubles; q_fn -1: no frame_null_in
  int q_eval, q_aff, q_fn;
  // doubles into the arena's read-back part; o_fn, o_pre -1: not asked for.  o_words: rank and flags, two ints in one double's room
  int o_basis, o_pinv, o_sing, o_words, o_fn, o_pre;
};

__global__ __launch_bounds__(kBlock) void nsp_kernel(const NspJob *jobs, const double *sq, double *out, nsp::Scales S, nsp::UnitPoses U) {
  using namespace nsp;
  const NspJob J = jobs[blockIdx.x];
  const int n = J.n, N = J.N, tid = threadIdx.x;
  __shared__ double sLog[kMaxF * kLogs * 6], sFn[kMaxF * 42], sW[kMaxN * kCols], sV[kCols * kCols];
  __shared__ double sDot[9], sCs[3], sSn[3], sNorm[kCols], sSing[kCols], sInv[kCols], sAmax;
  __shared__ int sRot[3], sBad[kBlock / 64], sRank;
  bool bad = false;

  // ---- A: G1, G2 (or the caller's blocks), G3, G4 ----
  if (J.q_fn < 0) {
    if (tid < n * kLogs) {
      const int f = tid / kLogs, c = tid - f * kLogs;
      double T[7], xi[6];
#pragma unroll
      for (int k = 0; k < 7; k++) T[k] = sq[J.q_eval + 7 * f + k];
      frame_log(T, U, c, xi);
#pragma unroll
      for (int r = 0; r < 6; r++) sLog[tid * 6 + r] = xi[r];
    }
    __syncthreads();
    if (tid < n * kCols) {
      const int f = tid / kCols, i = tid - f * kCols;
      const double *P = sLog + (f * kLogs + (i < 6 ? i : 12)) * 6, *M = sLog + (f * kLogs + (i < 6 ? 6 + i : 13)) * 6;
#pragma unroll
      for (int r = 0; r < 6; r++) sFn[f * 42 + r * 7 + i] = null_entry(P[r], M[r]);
    }
  } else {
    for (int e = tid; e < n * 42; e += kBlock) sFn[e] = sq[J.q_fn + e];
  }
  __syncthreads();
  if (J.o_fn >= 0)
    for (int e = tid; e < n * 42; e += kBlock) out[J.o_fn + e] = sFn[e];
  for (int e = tid; e < N * kCols; e += kBlock) {
    const int row = e / kCols, k = e - row * kCols;
    double v = 0.0;
    if (row >= 4) {
      const int f = (row - 4) >> 3, r = (row - 4) & 7;
      if (r < 6) v = scaled_entry(sFn[f * 42 + r * 7 + k], r, S);
    }
    sW[e] = v;
    if (J.o_pre >= 0) out[J.o_pre + row * 9 + (k < 6 ? k : 8)] = v;
  }
  if (J.o_pre >= 0 && tid < N) {
    double A = 0.0, B = 0.0;
    if (tid >= 4 && ((tid - 4) & 7) >= 6) {
      double a[2], b[2];
      affine_rows(sq[J.q_aff + ((tid - 4) >> 3)], S, a, b);
      const bool last = ((tid - 4) & 7) == 7;
      A = last ? a[1] : a[0], B = last ? b[1] : b[0];
    }
    out[J.o_pre + tid * 9 + 6] = A, out[J.o_pre + tid * 9 + 7] = B;
  }
  __syncthreads();

  // ---- B: G5 ----
  if (tid < kCols) {
    const double s = col_dot(sW, N, tid, tid);
    sNorm[tid] = s > 0.0 ? sqrt(s) : 0.0; // 0: the column stays as it is
  }
  __syncthreads();
  for (int e = tid; e < N * kCols; e += kBlock) {
    const double d = sNorm[e % kCols];
    double v = sW[e];
    if (d > 0.0) v = v / d, sW[e] = v;
    out[J.o_basis + e] = v;
    bad = bad || !isfinite(v);
  }
  if (tid < kCols * kCols) sV[tid] = tid % (kCols + 1) == 0 ? 1.0 : 0.0;
  __syncthreads();

  // ---- C: G6 ----
  if (tid < kCols) sDot[tid] = col_dot(sW, N, tid, tid);
  __syncthreads();
  if (tid == 0) {
    double amax = 0.0;
    for (int k = 0; k < kCols; k++)
      if (sDot[k] > amax) amax = sDot[k];
    sAmax = amax;
  }
  __syncthreads();
  bool capped = true;
  for (int sweep = 0; sweep < kSweepCap; sweep++) {
    int rotated = 0;
    for (int r = 0; r < kRounds; r++) {
      if (tid < 9) { // pair tid / 3: p.p, q.q, p.q
        int p, q;
        round_pair(r, tid / 3, p, q);
        const int which = tid % 3;
        sDot[tid] = col_dot(sW, N, which == 1 ? q : p, which == 0 ? p : q);
      }
      __syncthreads();
      if (tid < 3) {
        double cs, sn;
        sRot[tid] = rotation(sDot[3 * tid], sDot[3 * tid + 1], sDot[3 * tid + 2], sAmax, S.delta, cs, sn) ? 1 : 0;
        sCs[tid] = cs, sSn[tid] = sn;
      }
      __syncthreads();
      rotated |= sRot[0] | sRot[1] | sRot[2];
      if (tid < N + kCols) {
        double *row = tid < N ? sW + tid * kCols : sV + (tid - N) * kCols;
        for (int k = 0; k < 3; k++)
          if (sRot[k]) {
            int p, q;
            round_pair(r, k, p, q);
            rotate(row[p], row[q], sCs[k], sSn[k]);
          }
      }
      __syncthreads();
    }
    if (!rotated) {
      capped = false;
      break;
    }
  }
  if (tid < kCols) {
    const double s = sqrt(col_dot(sW, N, tid, tid));
    sSing[tid] = s, out[J.o_sing + tid] = s;
    bad = bad || !isfinite(s);
  }
  __syncthreads();
  if (tid == 0) {
    double sing[kCols], inv[kCols];
#pragma unroll
    for (int k = 0; k < kCols; k++) sing[k] = sSing[k];
    sRank = kept_inverses(sing, S.delta, inv);
#pragma unroll
    for (int k = 0; k < kCols; k++) sInv[k] = inv[k];
  }
  __syncthreads();
  for (int e = tid; e < kCols * N; e += kBlock) {
    const int k = e / N, i = e - k * N;
    const double v = pinv_entry(sV + k * kCols, sW + i * kCols, sInv);
    out[J.o_pinv + e] = v;
    bad = bad || !isfinite(v);
  }

  // ---- G7 ----
  const bool wave_bad = __ballot(bad) != 0;
  if ((tid & 63) == 0) sBad[tid >> 6] = wave_bad ? 1 : 0;
  __syncthreads();
  if (tid == 0) {
    int flags = capped ? DSM_NULLSPACE_SWEEP_CAP : 0;
    for (int w = 0; w < kBlock / 64; w++)
      if (sBad[w]) flags |= DSM_NULLSPACE_NONFINITE;
    for (int k = 0; k < kCols; k++)
      if (!(sNorm[k] > 0.0)) flags |= DSM_NULLSPACE_UNNORMALISED;
    int *words = reinterpret_cast<int *>(out + J.o_words);
    words[0] = sRank, words[1] = flags;
  }
}

} // namespace

extern "C" int dsm_window_nullspace_batch(dsm_context *ctx, int n_jobs, const dsm_nullspace_job *jobs, const dsm_nullspace_params *params) {
  if (!ctx) return invalid("dsm_window_nullspace_batch: bad argument");
  dsm_nullspace_params P;
  int rc = nullspace_check("dsm_window_nullspace_batch", n_jobs, jobs, params, P);
  if (rc) return rc;
  const nsp::Scales S = nullspace_scales(P);
  nsp::UnitPoses U;
  nsp::unit_poses(U);

  // staged [job table | doubles: per job eval, affB, frame_null_in], read back [doubles: per job basis, pinv, sing, rank and flags,
  // as asked for: the blocks, the nine vectors]
  std::vector<NspJob> T(n_jobs);
  size_t in_doubles = 0, out_doubles = 0;
  for (int j = 0; j < n_jobs; j++) {
    const dsm_nullspace_job &G = jobs[j];
    const int n = G.n_frames, N = 4 + 8 * n;
    NspJob &K = T[j];
    K.n = n, K.N = N;
    auto in = [&](size_t m) { return in_doubles += m, (int)(in_doubles - m); };
    auto out = [&](size_t m) { return out_doubles += m, (int)(out_doubles - m); };
    K.q_eval = in(7 * (size_t)n), K.q_aff = in(n), K.q_fn = G.frame_null_in ? in(42 * (size_t)n) : -1;
    K.o_basis = out(7 * (size_t)N), K.o_pinv = out(7 * (size_t)N), K.o_sing = out(7), K.o_words = out(1);
    K.o_fn = G.frame_null_out ? out(42 * (size_t)n) : -1, K.o_pre = G.null_x0_pre ? out(9 * (size_t)N) : -1;
  }
  if (in_doubles > 0x7fffffffu || out_doubles > 0x7fffffffu) return invalid("dsm_window_nullspace_batch: too many jobs for one call");
  CallArena A;
  const size_t o_jobs = A.in.take(sizeof(NspJob) * n_jobs), o_sq = A.in.take(8 * in_doubles);
  A.out.take(8 * out_doubles);
  if ((rc = A.bind(ctx))) return rc;
  memcpy(A.host_in<NspJob>(o_jobs), T.data(), sizeof(NspJob) * n_jobs);
  double *hq = A.host_in<double>(o_sq);
  for (int j = 0; j < n_jobs; j++) {
    const dsm_nullspace_job &G = jobs[j];
    const NspJob &K = T[j];
    memcpy(hq + K.q_eval, G.world_to_cam_eval, 56 * (size_t)K.n);
    for (int f = 0; f < K.n; f++) hq[K.q_aff + f] = nsp::affine_b(G.state_zero[8 * f + 6], P.scale_a, G.exposure[f]); // G3
    if (G.frame_null_in) memcpy(hq + K.q_fn, G.frame_null_in, 8 * 42 * (size_t)K.n);
  }
  if ((rc = A.upload())) return rc;
  hipLaunchKernelGGL(nsp_kernel, dim3(n_jobs), dim3(kBlock), 0, ctx->stream, A.dev_in<const NspJob>(o_jobs), A.dev_in<const double>(o_sq),
                     A.dev_out<double>(), S, U);
  DSM_HIP(hipGetLastError());
  if ((rc = A.fetch(A.out.used))) return rc;
  const double *ho = A.host_out<double>(0);
  for (int j = 0; j < n_jobs; j++) {
    const dsm_nullspace_job &G = jobs[j];
    const NspJob &K = T[j];
    memcpy(G.null_basis, ho + K.o_basis, 56 * (size_t)K.N), memcpy(G.null_pinv, ho + K.o_pinv, 56 * (size_t)K.N), memcpy(G.sing, ho + K.o_sing, 56);
    memcpy(G.rank, ho + K.o_words, 4), memcpy(G.flags, reinterpret_cast<const int *>(ho + K.o_words) + 1, 4);
    if (G.frame_null_out) memcpy(G.frame_null_out, ho + K.o_fn, 8 * 42 * (size_t)K.n);
    if (G.null_x0_pre) memcpy(G.null_x0_pre, ho + K.o_pre, 72 * (size_t)K.N);
  }
  return DSM_OK;
}
