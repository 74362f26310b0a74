// rescale_kernels.hip -- what FrontEnd::optimizeScale does behind its scale search (FrontEnd.cpp:1010-1061, gated at :806) on the device,
// for the windows of many sequences in one call.  Semantics: S0-S6 and V of DESIGN.md section 25.
//
// One dsm_window_rescale_batch = the decisions on the host (S0, S1), one staged copy of the ACCEPTED jobs in the call arena
// (call_arena.hpp), ONE launch, one read-back; a job that is not accepted gets its byte copies on the host (S6) and is not staged.
//   rsc_kernel  grid (1 + P, accepted jobs), 256 lanes, P <= 8.
//     workgroup 0 of a job: lanes k < n: the newest frame's S3 (lane n - 1), then D2 on the primed values (the double sincos lives
//       here); lanes 0-3: D1's cam and c_delta.  Poses, aff and the states pass through LDS across one barrier.  Lane h n + t: Q1-Q4
//       of pair (h, t) and the pair's eight adHTdeltaF entries from the job's staged matrices (S4); the diagonal is written as zeros.
//     workgroups 1 .. P: S2, the points grid-strided: consecutive lanes load consecutive floats and store two.
// Every result is one sequential chain in one lane, independent of the launch geometry and of the other jobs.  No scratch, no atomics,
// no wait on another workgroup, vector stores only.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "call_arena.hpp"
#include "rescale_launch.hpp"

using namespace dsm;

namespace {

constexpr int kBlock = kRscBlock;
constexpr int kMaxF = DSM_WINDOW_MAX_FRAMES;
static_assert(kMaxF * kMaxF <= kBlock, "one lane per pair");

struct RscJob {
  int n, n_pts;
  float new_scale;
  // doubles into the staged doubles
  int q_eval, q_state, q_zero, q_ctr, q_ref, q_aff, q_cval, q_czero, q_adh, q_adt;
  // floats into the staged floats
  int f_exp, f_idepth;
  // doubles into the read-back doubles; o_C -1: not asked for
  int o_eval, o_state, o_zero, o_ctr, o_c2w, o_W, o_C, o_dx;
  // floats into the read-back floats; o_pre: the six tables back to back
  int o_pre, o_adht, o_cam, o_cd, o_idepth, o_ids;
};

__global__ __launch_bounds__(kBlock) void rsc_kernel(const RscJob *jobs, const double *sq, const float *sf, double *oq, float *of, stp::Scales S) {
  const RscJob &J = jobs[blockIdx.y];
  const int n = J.n, f = n - 1, tid = threadIdx.x;
  if (blockIdx.x > 0) { // S2
    const int stride = ((int)gridDim.x - 1) * kBlock;
    const float scale = J.new_scale;
    for (int p = ((int)blockIdx.x - 1) * kBlock + tid; p < J.n_pts; p += stride) {
      const float id = rsc::point_idepth(sf[J.f_idepth + p], scale);
      of[J.o_idepth + p] = id, of[J.o_ids + p] = stp::point_idepth_scaled(S.idepth, id);
    }
    return; // uniform over the workgroup
  }
  __shared__ double sEval[kMaxF * 7], sEi[kMaxF * 7], sW[kMaxF * 7], sC[kMaxF * 7], sAff[kMaxF * 2], sState[kMaxF * 8], sZero[kMaxF * 8];
  __shared__ float sCam[6];
  if (tid < n) { // S3, then D2 on the primed values
    double state[8], zero[8], eval[7], delta_f[8], aff[2], aff0[2], W[7], C[7], Ei[7];
#pragma unroll
    for (int k = 0; k < 8; k++) state[k] = sq[J.q_state + 8 * tid + k], zero[k] = sq[J.q_zero + 8 * tid + k];
#pragma unroll
    for (int k = 0; k < 7; k++) eval[k] = sq[J.q_eval + 7 * tid + k];
    if (tid == f) {
      double ctr[7], ref[7], ctr_out[7], c2w[7], fresh[8];
#pragma unroll
      for (int k = 0; k < 7; k++) ctr[k] = sq[J.q_ctr + k], ref[k] = sq[J.q_ref + k];
      const double g2l[2] = {sq[J.q_aff], sq[J.q_aff + 1]};
      rsc::newest_frame(ctr, ref, g2l, J.new_scale, S, ctr_out, c2w, eval, fresh);
#pragma unroll
      for (int k = 0; k < 8; k++) state[k] = zero[k] = fresh[k];
#pragma unroll
      for (int k = 0; k < 7; k++) oq[J.o_ctr + k] = ctr_out[k], oq[J.o_c2w + k] = c2w[k];
    }
    fin::frame_pose(state, zero, eval, S, delta_f, aff, aff0, W, C);
    stp::se3_inverse(eval, Ei);
    double *eval_out = oq + J.o_eval + 7 * tid, *zero_out = oq + J.o_zero + 8 * tid, *st_out = oq + J.o_state + 8 * tid, *dx = oq + J.o_dx + 4 + 8 * tid;
#pragma unroll
    for (int k = 0; k < 8; k++) sState[8 * tid + k] = state[k], sZero[8 * tid + k] = zero[k], st_out[k] = state[k], zero_out[k] = zero[k], dx[k] = delta_f[k];
#pragma unroll
    for (int k = 0; k < 7; k++)
      sEval[7 * tid + k] = eval[k], sEi[7 * tid + k] = Ei[k], sW[7 * tid + k] = W[k], sC[7 * tid + k] = C[k], eval_out[k] = eval[k], oq[J.o_W + 7 * tid + k] = W[k];
    if (J.o_C >= 0) {
#pragma unroll
      for (int k = 0; k < 7; k++) oq[J.o_C + 7 * tid + k] = C[k];
    }
    sAff[2 * tid] = aff[0], sAff[2 * tid + 1] = aff[1];
  }
  if (tid < 4) { // D1 on the calibration given
    float cam, c_delta;
    fin::calib_cam(tid, sq[J.q_cval + tid], sq[J.q_czero + tid], S, cam, c_delta);
    sCam[tid] = cam, of[J.o_cd + tid] = c_delta, oq[J.o_dx + tid] = (double)c_delta; // E1's first four
    if (tid < 2) sCam[4 + tid] = stp::cam_inverse(cam);
  }
  __syncthreads();
  if (tid < 6) of[J.o_cam + tid] = sCam[tid];
  if (tid < n * n) {
    const int h = tid / n, t = tid - h * n, n2 = n * n;
    stp::PairRow o;
    if (h != t) { // Q1-Q4
      float cam[6];
#pragma unroll
      for (int k = 0; k < 6; k++) cam[k] = sCam[k];
      stp::pair_row(sEval + 7 * t, sEi + 7 * h, sW + 7 * t, sC + 7 * h, cam, sf[J.f_exp + h], sf[J.f_exp + t], sAff + 2 * h, sAff + 2 * t, sZero[8 * h + 7], S.b, o);
    } else {
#pragma unroll
      for (int k = 0; k < 9; k++) o.R0[k] = 0.0f, o.M[k] = 0.0f;
#pragma unroll
      for (int k = 0; k < 3; k++) o.t0[k] = 0.0f, o.Kt[k] = 0.0f;
      o.aff[0] = o.aff[1] = o.b0 = 0.0f;
    }
    float *q = of + J.o_pre; // the six tables back to back
#pragma unroll
    for (int k = 0; k < 9; k++) q[9 * tid + k] = o.R0[k], q[12 * n2 + 9 * tid + k] = o.M[k];
#pragma unroll
    for (int k = 0; k < 3; k++) q[9 * n2 + 3 * tid + k] = o.t0[k], q[21 * n2 + 3 * tid + k] = o.Kt[k];
    q[24 * n2 + 2 * tid] = o.aff[0], q[24 * n2 + 2 * tid + 1] = o.aff[1], q[26 * n2 + tid] = o.b0;
    const double *ah = sq + J.q_adh + 64 * tid, *at = sq + J.q_adt + 64 * tid; // setDeltaF on the adjoints as given
    float *dp = of + J.o_adht + 8 * tid;
    for (int c = 0; c < 8; c++)
      dp[c] = h != t ? ad_ht_delta_entry(ah, at, sState + 8 * h, sZero + 8 * h, sState + 8 * t, sZero + 8 * t, c) : 0.0f;
  }
}

} // namespace

extern "C" int dsm_window_rescale_batch(dsm_context *ctx, int n_jobs, const dsm_rescale_job *jobs, const dsm_linearize_params *lp,
                                        const dsm_step_params *sp) {
  if (!ctx) return invalid("dsm_window_rescale_batch: bad argument");
  dsm_linearize_params LP;
  dsm_step_params SP;
  int rc = rescale_check("dsm_window_rescale_batch", n_jobs, jobs, lp, sp, LP, SP);
  if (rc) return rc;
  const stp::Scales S = rescale_scales(LP, SP);

  // S0, S1: the decisions, on the inputs alone
  std::vector<int> accepted;
  for (int j = 0; j < n_jobs; j++) {
    const dsm_rescale_job &G = jobs[j];
    if (rsc::decide(G.enabled, G.scale_error, G.new_scale, G.thres, G.trapped, G.fails).decision == DSM_RESCALE_ACCEPTED) accepted.push_back(j);
  }

  // staged [job table | doubles: per job eval, state, state_zero, the three of the newest frame, the calibration, the adjoints | floats:
  // exposure, idepth], read back [doubles: eval, state, state_zero, the newest frame's two poses, both pose tables, delta_x | floats:
  // the six tables, adHTdeltaF, cam, c_delta, the points' two arrays]
  const int na = (int)accepted.size();
  std::vector<RscJob> T(na);
  size_t in_q = 0, in_f = 0, out_q = 0, out_f = 0;
  int max_pts = 0;
  for (int a = 0; a < na; a++) {
    const dsm_rescale_job &G = jobs[accepted[a]];
    const size_t n = G.n_frames, n2 = n * n, np = G.n_pts;
    RscJob &K = T[a];
    K.n = G.n_frames, K.n_pts = G.n_pts, K.new_scale = G.new_scale;
    max_pts = std::max(max_pts, G.n_pts);
    auto iq = [&](size_t m) { return in_q += m, (int)(in_q - m); };
    auto jf = [&](size_t m) { return in_f += m, (int)(in_f - m); };
    auto oq = [&](size_t m) { return out_q += m, (int)(out_q - m); };
    auto of = [&](size_t m) { return out_f += m, (int)(out_f - m); };
    K.q_eval = iq(7 * n), K.q_state = iq(8 * n), K.q_zero = iq(8 * n), K.q_ctr = iq(7), K.q_ref = iq(7), K.q_aff = iq(2), K.q_cval = iq(4), K.q_czero = iq(4);
    K.q_adh = iq(64 * n2), K.q_adt = iq(64 * n2);
    K.f_exp = jf(n), K.f_idepth = jf(np);
    K.o_eval = oq(7 * n), K.o_state = oq(8 * n), K.o_zero = oq(8 * n), K.o_ctr = oq(7), K.o_c2w = oq(7), K.o_W = oq(7 * n);
    K.o_C = G.cam_to_world_out_all ? oq(7 * n) : -1, K.o_dx = oq(4 + 8 * n);
    K.o_pre = of(27 * n2), K.o_adht = of(8 * n2), K.o_cam = of(6), K.o_cd = of(4), K.o_idepth = of(np), K.o_ids = of(np);
  }
  if (na > 65535 || in_q > 0x7fffffffu || in_f > 0x7fffffffu || out_q > 0x7fffffffu || out_f > 0x7fffffffu)
    return invalid("dsm_window_rescale_batch: too many jobs for one call");

  if (na) {
    CallArena A;
    const size_t o_jobs = A.in.take(sizeof(RscJob) * na), o_sq = A.in.take(8 * in_q), o_sf = A.in.take(4 * in_f);
    const size_t o_oq = A.out.take(8 * out_q), o_of = A.out.take(4 * out_f);
    if ((rc = A.bind(ctx))) return rc;
    memcpy(A.host_in<RscJob>(o_jobs), T.data(), sizeof(RscJob) * na);
    double *hq = A.host_in<double>(o_sq);
    float *hf = A.host_in<float>(o_sf);
    for (int a = 0; a < na; a++) {
      const dsm_rescale_job &G = jobs[accepted[a]];
      const RscJob &K = T[a];
      const size_t n = K.n, n2 = n * n;
      memcpy(hq + K.q_eval, G.world_to_cam_eval, 56 * n), memcpy(hq + K.q_state, G.state, 64 * n), memcpy(hq + K.q_zero, G.state_zero, 64 * n);
      memcpy(hq + K.q_ctr, G.cam_to_tracking_ref, 56), memcpy(hq + K.q_ref, G.ref_cam_to_world, 56), memcpy(hq + K.q_aff, G.aff_g2l, 16);
      memcpy(hq + K.q_cval, G.calib_value, 32), memcpy(hq + K.q_czero, G.calib_zero, 32);
      memcpy(hq + K.q_adh, G.ad_host, 512 * n2), memcpy(hq + K.q_adt, G.ad_target, 512 * n2);
      memcpy(hf + K.f_exp, G.exposure, 4 * n);
      if (K.n_pts) memcpy(hf + K.f_idepth, G.idepth, 4 * (size_t)K.n_pts);
    }
    if ((rc = A.upload())) return rc;
    const int point_blocks = std::min(kRscPointBlocks, (max_pts + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(rsc_kernel, dim3(1 + point_blocks, na), dim3(kBlock), 0, ctx->stream, A.dev_in<const RscJob>(o_jobs), A.dev_in<const double>(o_sq),
                       A.dev_in<const float>(o_sf), A.dev_out<double>(o_oq), A.dev_out<float>(o_of), S);
    DSM_HIP(hipGetLastError());
    if ((rc = A.fetch(A.out.used))) return rc;
    const double *ho = A.host_out<double>(o_oq);
    const float *hp = A.host_out<float>(o_of);
    for (int a = 0; a < na; a++) {
      const dsm_rescale_job &G = jobs[accepted[a]];
      const RscJob &K = T[a];
      const size_t n = K.n, n2 = n * n, np = K.n_pts;
      memcpy(G.world_to_cam_eval_out, ho + K.o_eval, 56 * n), memcpy(G.state_out, ho + K.o_state, 64 * n), memcpy(G.state_zero_out, ho + K.o_zero, 64 * n);
      memcpy(G.cam_to_tracking_ref_out, ho + K.o_ctr, 56), memcpy(G.cam_to_world_out, ho + K.o_c2w, 56), memcpy(G.world_to_cam_out, ho + K.o_W, 56 * n);
      if (G.cam_to_world_out_all) memcpy(G.cam_to_world_out_all, ho + K.o_C, 56 * n);
      memcpy(G.delta_x_out, ho + K.o_dx, 8 * (4 + 8 * n));
      const float *q = hp + K.o_pre;
      memcpy(G.pre_RTll_0_out, q, 36 * n2), memcpy(G.pre_tTll_0_out, q + 9 * n2, 12 * n2), memcpy(G.pre_KRKiTll_out, q + 12 * n2, 36 * n2);
      memcpy(G.pre_KtTll_out, q + 21 * n2, 12 * n2), memcpy(G.pre_aff_mode_out, q + 24 * n2, 8 * n2), memcpy(G.pre_b0_mode_out, q + 26 * n2, 4 * n2);
      memcpy(G.ad_ht_delta_out, hp + K.o_adht, 32 * n2), memcpy(G.cam_out, hp + K.o_cam, 24), memcpy(G.c_delta_out, hp + K.o_cd, 16);
      if (np) { // S2: the two scaled depths are one value, and deltaF becomes 0
        memcpy(G.idepth_out, hp + K.o_idepth, 4 * np), memcpy(G.idepth_scaled_out, hp + K.o_ids, 4 * np);
        memcpy(G.idepth_zero_scaled_out, hp + K.o_ids, 4 * np), memset(G.delta_out, 0, 4 * np);
      }
    }
  }
  for (int j = 0; j < n_jobs; j++) // the words of every job, S6 for the rest
    if (rescale_decide(jobs[j]) != DSM_RESCALE_ACCEPTED) rescale_copy_through(jobs[j]);
  return DSM_OK;
}
