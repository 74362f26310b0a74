// admit_kernels.hip -- the head of FrontEnd::makeKeyFrame (FrontEnd.cpp:722-762, with flagFramesForMarginalization of
// dso_helpers/FrontEndMarginalize.cpp:62-146) on the device, for the windows of many sequences in one call.  Semantics: A1-A6 and V of
// DESIGN.md section 26.
//
// One dsm_window_admit_batch = one staged copy in the call arena (call_arena.hpp, laid out by admit_launch.hpp), ONE launch, one
// read-back.
//   adm_kernel  grid (1 + P, jobs), 256 lanes, P <= 8.
//     workgroup 0 of a job: lanes k <= n: the new frame's A1 (lane n), then D2 on the primed values (the double sincos lives here);
//       lanes 0-3: D1's cam and c_delta.  Poses, aff and the states pass through LDS across one barrier.  Lane h (n+1) + t: Q1-Q4 of
//       pair (h, t), its adHost and adTarget (A3, written to the read-back block and read again by the same lane for its eight
//       adHTdeltaF entries) and its distance, the distance also into LDS.  After a second barrier lane 0 walks F1's chain (it carries
//       `flagged`) while lane h < n forms F2's score of host h; after a third, lane 0 takes the first minimum.
//     workgroups 1 .. P, strided: A6's moves and new residuals, last_res, and the zero-padded copies of A5.
// Every result is one sequential chain in one lane, independent of the launch geometry and of the other jobs.  No scratch, no atomics,
// no wait on another workgroup, vector stores only.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "admit_launch.hpp"
#include "call_arena.hpp"
#include "rescale_launch.hpp"

using namespace dsm;

namespace {

constexpr int kBlock = kAdmBlock;
constexpr int kMaxF = DSM_WINDOW_MAX_FRAMES;
static_assert(kMaxF * kMaxF <= kBlock, "one lane per pair");

struct AdmIn {
  const double *q;
  const float *f;
  const int *i;
  const unsigned char *b;
};
struct AdmOut {
  double *q;
  float *f;
  int *i;
  unsigned char *b;
};

// A5: `in` (N x N, or N with rows == 1) in the top left of `out`, the rest zeros or `tail`
__device__ void grow_matrix(const double *in, double *out, int N, int M, int first, int stride) {
  for (int e = first; e < M * M; e += stride) {
    const int i = e / M, j = e - i * M;
    out[e] = i < N && j < N ? in[i * N + j] : 0.0;
  }
}
__device__ void grow_vector(const double *in, double *out, const double *tail, int N, int M, int first, int stride) {
  for (int i = first; i < M; i += stride) out[i] = i < N ? in[i] : tail ? tail[i - N] : 0.0;
}

__global__ __launch_bounds__(kBlock) void adm_kernel(const AdmJob *jobs, AdmIn in, AdmOut out, stp::Scales S, adm::Params P) {
  const AdmJob &J = jobs[blockIdx.y];
  const int n = J.n, m = n + 1, tid = threadIdx.x;
  if (blockIdx.x > 0) { // A6, A5
    const int stride = ((int)gridDim.x - 1) * kBlock, first = ((int)blockIdx.x - 1) * kBlock + tid;
    const int N = 4 + 8 * n, M = N + 8;
    const int *point = in.i + J.i_point;
    for (int r = first; r < J.n_res; r += stride) {
      const int pt = point[r], to = adm::old_index(r, pt);
      out.i[J.oi_point + to] = pt, out.i[J.oi_target + to] = in.i[J.i_target + r], out.b[J.ob_state + to] = in.b[J.b_state + r];
      out.f[J.of_energy + to] = in.f[J.f_energy + r], out.b[J.ob_new + to] = in.b[J.b_new + r], out.i[J.oi_res + r] = to;
    }
    for (int p = first; p < J.n_pts; p += stride) {
      const int to = adm::new_index(adm::run_end(point, J.n_res, p), p), l0 = in.i[J.i_last + 2 * p];
      out.i[J.oi_point + to] = p, out.i[J.oi_target + to] = n, out.b[J.ob_state + to] = DSM_RES_IN, out.f[J.of_energy + to] = 0.0f;
      out.b[J.ob_new + to] = 1, out.i[J.oi_new + p] = to;
      out.i[J.oi_last + 2 * p] = to, out.i[J.oi_last + 2 * p + 1] = l0 >= 0 ? adm::old_index(l0, point[l0]) : -1;
      out.b[J.ob_last + 2 * p] = DSM_RES_IN, out.b[J.ob_last + 2 * p + 1] = in.b[J.b_last + 2 * p];
    }
    if (J.q_HM >= 0) grow_matrix(in.q + J.q_HM, out.q + J.oq_HM, N, M, first, stride);
    if (J.q_bM >= 0) grow_vector(in.q + J.q_bM, out.q + J.oq_bM, nullptr, N, M, first, stride);
    if (J.q_HL >= 0) grow_matrix(in.q + J.q_HL, out.q + J.oq_HL, N, M, first, stride);
    if (J.q_bL >= 0) grow_vector(in.q + J.q_bL, out.q + J.oq_bL, nullptr, N, M, first, stride);
    if (J.q_prior >= 0) {
      grow_vector(in.q + J.q_prior, out.q + J.oq_prior, in.q + J.q_prior_f, N, M, first, stride);
      grow_vector(in.q + J.q_prior0, out.q + J.oq_prior0, in.q + J.q_prior_f0, N, M, first, stride);
    }
    return; // uniform over the workgroup
  }
  __shared__ double sEval[kMaxF * 7], sEi[kMaxF * 7], sW[kMaxF * 7], sC[kMaxF * 7], sAff[kMaxF * 2], sAff0[kMaxF * 2], sState[kMaxF * 8], sZero[kMaxF * 8];
  __shared__ double sScore[kMaxF];
  __shared__ float sCam[6], sExp[kMaxF], sDist[kMaxF * kMaxF];
  __shared__ int sId[kMaxF], sF2;
  __shared__ unsigned char sFlag[kMaxF];
  if (tid < m) { // A1, then D2 on the primed values
    double state[8], zero[8], eval[7], delta_f[8], aff[2], aff0[2], W[7], C[7], Ei[7];
    float expo, eth;
    int id;
    if (tid == n) {
      double ctr[7], ref[7], ctr_out[7], c2w[7];
#pragma unroll
      for (int k = 0; k < 7; k++) ctr[k] = in.q[J.q_ctr + k], ref[k] = in.q[J.q_ref + k];
      const double g2l[2] = {in.q[J.q_aff], in.q[J.q_aff + 1]};
      rsc::newest_frame(ctr, ref, g2l, 1.0f, S, ctr_out, c2w, eval, state);
#pragma unroll
      for (int k = 0; k < 8; k++) {
        zero[k] = state[k];
        out.q[J.oq_fprior + k] = in.q[J.q_prior_f + k], out.q[J.oq_fdelta + k] = state[k] - in.q[J.q_prior_f0 + k]; // A5: takeData
      }
#pragma unroll
      for (int k = 0; k < 7; k++) out.q[J.oq_c2w + k] = c2w[k];
      expo = J.new_exposure, eth = J.new_eth, id = J.new_id;
    } else {
#pragma unroll
      for (int k = 0; k < 8; k++) state[k] = in.q[J.q_state + 8 * tid + k], zero[k] = in.q[J.q_zero + 8 * tid + k];
#pragma unroll
      for (int k = 0; k < 7; k++) eval[k] = in.q[J.q_eval + 7 * tid + k];
      expo = in.f[J.f_exp + tid], eth = in.f[J.f_eth + tid], id = in.i[J.i_id + tid];
    }
    fin::frame_pose(state, zero, eval, S, delta_f, aff, aff0, W, C);
    stp::se3_inverse(eval, Ei);
    double *eval_out = out.q + J.oq_eval + 7 * tid, *zero_out = out.q + J.oq_zero + 8 * tid, *st_out = out.q + J.oq_state + 8 * tid;
    double *dx = out.q + J.oq_dx + 4 + 8 * tid;
#pragma unroll
    for (int k = 0; k < 8; k++) sState[8 * tid + k] = state[k], sZero[8 * tid + k] = zero[k], st_out[k] = state[k], zero_out[k] = zero[k], dx[k] = delta_f[k];
#pragma unroll
    for (int k = 0; k < 7; k++)
      sEval[7 * tid + k] = eval[k], sEi[7 * tid + k] = Ei[k], sW[7 * tid + k] = W[k], sC[7 * tid + k] = C[k], eval_out[k] = eval[k], out.q[J.oq_W + 7 * tid + k] = W[k];
    sAff[2 * tid] = aff[0], sAff[2 * tid + 1] = aff[1], sAff0[2 * tid] = aff0[0], sAff0[2 * tid + 1] = aff0[1];
    sExp[tid] = expo, sId[tid] = id, sFlag[tid] = 0;
    out.f[J.of_exp + tid] = expo, out.f[J.of_eth + tid] = eth, out.i[J.oi_id + tid] = id;
  }
  if (tid < 4) { // D1 on the calibration given
    float cam, c_delta;
    fin::calib_cam(tid, in.q[J.q_cval + tid], in.q[J.q_czero + tid], S, cam, c_delta);
    sCam[tid] = cam, out.f[J.of_cd + tid] = c_delta, out.q[J.oq_dx + tid] = (double)c_delta; // E1's first four
    if (tid < 2) sCam[4 + tid] = stp::cam_inverse(cam);
  }
  __syncthreads();
  if (tid < 6) out.f[J.of_cam + tid] = sCam[tid];
  if (tid < m * m) {
    const int h = tid / m, t = tid - h * m, m2 = m * m;
    const float exp_h = sExp[h], exp_t = sExp[t];
    stp::PairRow o;
    float dist = 0.0f;
    if (h != t) { // Q1-Q4 and the distance
      float cam[6];
#pragma unroll
      for (int k = 0; k < 6; k++) cam[k] = sCam[k];
      stp::pair_row(sEval + 7 * t, sEi + 7 * h, sW + 7 * t, sC + 7 * h, cam, exp_h, exp_t, sAff + 2 * h, sAff + 2 * t, sZero[8 * h + 7], S.b, o);
      dist = adm::distance_ll(sW + 7 * t, sC + 7 * h);
    } else {
#pragma unroll
      for (int k = 0; k < 9; k++) o.R0[k] = 0.0f, o.M[k] = 0.0f;
#pragma unroll
      for (int k = 0; k < 3; k++) o.t0[k] = 0.0f, o.Kt[k] = 0.0f;
      o.aff[0] = o.aff[1] = o.b0 = 0.0f;
    }
    float *q = out.f + J.of_pre; // the six tables back to back
#pragma unroll
    for (int k = 0; k < 9; k++) q[9 * tid + k] = o.R0[k], q[12 * m2 + 9 * tid + k] = o.M[k];
#pragma unroll
    for (int k = 0; k < 3; k++) q[9 * m2 + 3 * tid + k] = o.t0[k], q[21 * m2 + 3 * tid + k] = o.Kt[k];
    q[24 * m2 + 2 * tid] = o.aff[0], q[24 * m2 + 2 * tid + 1] = o.aff[1], q[26 * m2 + tid] = o.b0;
    sDist[h * kMaxF + t] = dist, out.f[J.of_dist + tid] = dist;
    double *ah = out.q + J.oq_adh + 64 * tid, *at = out.q + J.oq_adt + 64 * tid; // A3: every pair
    double Adj[36];
    fin::adjoint(sEval + 7 * t, sEi + 7 * h, Adj);
    fin::adjoint_pair(Adj, fin::aff_a0(sAff0 + 2 * h, sAff0 + 2 * t, exp_h, exp_t), S, ah, at);
    float *dp = out.f + J.of_adht + 8 * tid; // setDeltaF on them
    for (int c = 0; c < 8; c++)
      dp[c] = h != t ? ad_ht_delta_entry(ah, at, sState + 8 * h, sZero + 8 * h, sState + 8 * t, sZero + 8 * t, c) : 0.0f;
  }
  __syncthreads();
  // A4 over the n old frames
  const bool f0 = adm::f0_branch(P);
  if (tid == 0) {
    int count = 0;
    for (int i = 0; i < n; i++) {
      bool flag;
      if (f0)
        flag = adm::f0_flagged(i, n, P);
      else
        flag = adm::f1_flagged(in.i[J.i_in + i], in.i[J.i_out + i], sExp[n - 1], sExp[i], sAff + 2 * (n - 1), sAff + 2 * i, n, count, P);
      if (flag) sFlag[i] = 1, count++;
    }
    sF2 = !f0 && n - count >= P.max_frames;
  }
  // the scores are formed while lane 0 walks F1, whose count decides only afterwards whether F2 runs: a few hundred operations per
  // lane that need no barrier of their own.  Masking them by sF2 below is what keeps dist_score equal to the host form's, which
  // forms no score where F2 does not run
  if (tid < n) sScore[tid] = !f0 && adm::f2_candidate(sId[tid], sId[n - 1], P) ? adm::f2_score(sDist + tid * kMaxF, sId, tid, n, P) : 0.0;
  __syncthreads();
  if (tid == 0 && sF2) {
    const int pick = adm::f2_pick(sScore, sId, n, P);
    if (pick >= 0) sFlag[pick] = 1;
  }
  __syncthreads();
  if (tid < n) out.q[J.oq_score + tid] = sF2 ? sScore[tid] : 0.0;
  if (tid < m) out.b[J.ob_flagged + tid] = sFlag[tid];
  if (tid == 0) {
    int n_flagged = 0;
    for (int i = 0; i < n; i++) n_flagged += sFlag[i];
    out.i[J.oi_words] = J.n_res + J.n_pts, out.i[J.oi_words + 1] = n_flagged;
  }
}

} // namespace

extern "C" int dsm_window_admit_batch(dsm_context *ctx, int n_jobs, const dsm_admit_job *jobs, const dsm_linearize_params *lp,
                                      const dsm_step_params *sp, const dsm_admit_params *ap) {
  if (!ctx) return invalid("dsm_window_admit_batch: bad argument");
  dsm_linearize_params LP;
  dsm_step_params SP;
  adm::Params AP;
  int rc = admit_check("dsm_window_admit_batch", n_jobs, jobs, lp, sp, ap, LP, SP, AP);
  if (rc) return rc;
  const stp::Scales S = rescale_scales(LP, SP);

  std::vector<AdmJob> T(n_jobs);
  AdmTotals tot;
  for (int j = 0; j < n_jobs; j++) admit_layout(jobs[j], T[j], tot);
  if (n_jobs > 65535 || !tot.fits()) return invalid("dsm_window_admit_batch: too many jobs for one call");

  CallArena A;
  const size_t o_jobs = A.in.take(sizeof(AdmJob) * n_jobs), o_q = A.in.take(8 * tot.q), o_f = A.in.take(4 * tot.f), o_i = A.in.take(4 * tot.i);
  const size_t o_b = A.in.take(tot.b);
  const size_t o_oq = A.out.take(8 * tot.oq), o_of = A.out.take(4 * tot.of), o_oi = A.out.take(4 * tot.oi), o_ob = A.out.take(tot.ob);
  if ((rc = A.bind(ctx))) return rc;
  memcpy(A.host_in<AdmJob>(o_jobs), T.data(), sizeof(AdmJob) * n_jobs);
  for (int j = 0; j < n_jobs; j++)
    admit_stage(jobs[j], T[j], A.host_in<double>(o_q), A.host_in<float>(o_f), A.host_in<int>(o_i), A.host_in<unsigned char>(o_b));
  if ((rc = A.upload())) return rc;
  const int list_blocks = std::min(kAdmListBlocks, (tot.max_list + kBlock - 1) / kBlock);
  const AdmIn in{A.dev_in<const double>(o_q), A.dev_in<const float>(o_f), A.dev_in<const int>(o_i), A.dev_in<const unsigned char>(o_b)};
  const AdmOut out{A.dev_out<double>(o_oq), A.dev_out<float>(o_of), A.dev_out<int>(o_oi), A.dev_out<unsigned char>(o_ob)};
  hipLaunchKernelGGL(adm_kernel, dim3(1 + list_blocks, n_jobs), dim3(kBlock), 0, ctx->stream, A.dev_in<const AdmJob>(o_jobs), in, out, S, AP);
  DSM_HIP(hipGetLastError());
  if ((rc = A.fetch(A.out.used))) return rc;
  for (int j = 0; j < n_jobs; j++)
    admit_unstage(jobs[j], T[j], A.host_out<double>(o_oq), A.host_out<float>(o_of), A.host_out<int>(o_oi), A.host_out<unsigned char>(o_ob));
  return DSM_OK;
}
