// step_kernels.hip -- doStepFromBackup and setPrecalcValues of FrontEnd::optimize (dso_helpers/FrontEndOptimize.cpp:182-262, :300-323)
// on the device, in front of the trial step of dsm_window_solve_batch, for the windows of many sequences in one call.  Semantics:
// D1-D4, Q1-Q4, E1-E3, V of DESIGN.md section 19.
//
// One dsm_window_step_batch = the staged copy of dsm_window_solve_batch (solve_launch.hpp) with the step's inputs on top, TWO launches,
// the EIGHT launches of dsm_window_solve_batch on the same stream and arena, one read-back:
//   stp_frame_kernel  one 256-lane workgroup per job.  Lanes f < n: D2 (the double sincos lives here); lanes 0-3: D1; lane 255: the
//                     frames' part of D4.  Poses, aff, the state and cam pass through LDS across one barrier.  Lane h n + t: Q1-Q4 of
//                     pair (h, t) (n = 16 fills the workgroup), written where linearize_kernel reads the job's precalc tables.  Lanes
//                     i < N: E1-E3, one row's sum per lane; lane 0 adds the rows' terms of the M energy in ascending order.  (Lane i
//                     walks row i of H_M, so at each j a wave's lanes read addresses 8 N bytes apart: uncoalesced, accepted
//                     knowingly.  N <= 132, the launch is one workgroup per job and bound by latency, and a transposed walk would
//                     need H_M staged through LDS for nothing measurable.)
//   stp_point_kernel  one lane per point: D3, written where linearize_kernel reads idepth_scaled and idepth_zero_scaled.  ONE MORE
//                     workgroup per job for the two float chains of D4 over the points: its lanes form the terms of 256 points at a
//                     time in LDS, lane 0 adds them in ascending index and, with the frames' sums that stp_frame_kernel left, forms
//                     can_break: the chains feed nothing else, so they run beside the point lanes and add no launch.
// After the upload the arena's input part is ordinary device memory: the kernels of sections 16-18 see other values at the same
// offsets and are unchanged.  Every result is one sequential chain in one lane; no kernel waits for another workgroup; no scratch.
// The call's host side is the pieces of step_launch.hpp, which dsm_window_optimize_batch (optimize_kernels.hip) runs too.
#include <algorithm>
#include <cstddef>
#include <cstring>
#include <string>
#include <vector>

#include "step_launch.hpp"

#include "step_math.hpp"

using namespace dsm;

namespace {

constexpr int kFrameBlock = 256; // stp_frame_kernel: DSM_WINDOW_MAX_FRAMES^2 pair lanes
constexpr int kPointBlock = 256; // stp_point_kernel: points per workgroup
constexpr int kMaxF = DSM_WINDOW_MAX_FRAMES, kMaxN = 4 + 8 * kMaxF;
static_assert(kMaxF * kMaxF <= kFrameBlock && kMaxN < kFrameBlock, "one lane per pair and per row");

struct StpJob {
  int n, n_pts, N;
  float stepfac[5];
  // doubles into the step's staged doubles; q_prior, q_pzero -1: no prior
  int q_eval, q_zero, q_backup, q_step, q_czero, q_cbackup, q_cstep, q_prior, q_pzero;
  // 4-byte words into the step's staged floats
  int f_idb, f_ids, f_exp;
  // doubles into the solve's staged doubles (SolView); d_HM, d_bM -1: zeros
  long long d_HL, d_bL, d_HM, d_bM, d_dx;
  // 4-byte words from the start of the arena's device-only part, every one at a multiple of eight bytes; -1: not asked for
  long long o_state, o_calib, o_idepth, o_W, o_C, o_can, o_sums, o_em, o_cam, o_pre, o_dx, o_HL, o_bL;
};

__device__ __forceinline__ double *dbl(float *base, long long word) { return reinterpret_cast<double *>(base + word); }

__global__ __launch_bounds__(kFrameBlock) void stp_frame_kernel(const StpJob *jobs, LinJob *lin_jobs, float *stage, double *sd, const double *sq,
                                                                const float *sf, float *base, stp::Scales S) {
  const StpJob &J = jobs[blockIdx.x];
  LinJob &L = lin_jobs[blockIdx.x];
  const int n = J.n, N = J.N, tid = threadIdx.x;
  __shared__ double sW[kMaxF * 7], sC[kMaxF * 7], sEi[kMaxF * 7], sAff[kMaxF * 2], sState[kMaxF * 8], sDx[kMaxN], sTerm[kMaxN];
  __shared__ float sCam[6];
  if (tid < n) { // D2
    double state[8], delta_f[8], aff[2], W[7], C[7], Ei[7];
    const double *eval = sq + J.q_eval + 7 * tid;
    stp::frame_state(sq + J.q_backup + 8 * tid, sq + J.q_step + 8 * tid, sq + J.q_zero + 8 * tid, eval, J.stepfac, S, state, delta_f, aff, W, C);
    stp::se3_inverse(eval, Ei);
    double *state_out = dbl(base, J.o_state) + 8 * tid, *W_out = dbl(base, J.o_W) + 7 * tid;
#pragma unroll
    for (int k = 0; k < 8; k++) sState[8 * tid + k] = state[k], state_out[k] = state[k], sDx[4 + 8 * tid + k] = delta_f[k];
#pragma unroll
    for (int k = 0; k < 7; k++) sW[7 * tid + k] = W[k], sC[7 * tid + k] = C[k], sEi[7 * tid + k] = Ei[k], W_out[k] = W[k];
    if (J.o_C >= 0) {
      double *C_out = dbl(base, J.o_C) + 7 * tid;
#pragma unroll
      for (int k = 0; k < 7; k++) C_out[k] = C[k];
    }
    sAff[2 * tid] = aff[0], sAff[2 * tid + 1] = aff[1];
  }
  if (tid < 4) { // D1
    double value;
    float cam, c_delta;
    stp::calib_entry(tid, sq[J.q_cbackup + tid], J.stepfac[0], sq[J.q_cstep + tid], sq[J.q_czero + tid], S, value, cam, c_delta);
    dbl(base, J.o_calib)[tid] = value;
    sCam[tid] = cam, sDx[tid] = (double)c_delta; // E1's first four
    if (tid < 2) sCam[4 + tid] = stp::cam_inverse(cam);
  }
  if (tid == kFrameBlock - 1) { // D4, the frames' part
    float sums[4];
    stp::frame_sums(sq + J.q_step, n, sums);
#pragma unroll
    for (int k = 0; k < 4; k++) base[J.o_sums + k] = sums[k];
  }
  __syncthreads();
  if (tid == 0) L.fx = sCam[0], L.fy = sCam[1], L.cx = sCam[2], L.cy = sCam[3], L.fxi = sCam[4], L.fyi = sCam[5];
  if (tid < 6 && J.o_cam >= 0) base[J.o_cam + tid] = sCam[tid];
  if (tid < n * n) { // Q1-Q4
    const int h = tid / n, t = tid - h * n;
    stp::PairRow o;
    if (h != t) {
      float cam[6];
#pragma unroll
      for (int k = 0; k < 6; k++) cam[k] = sCam[k];
      stp::pair_row(sq + J.q_eval + 7 * t, sEi + 7 * h, sW + 7 * t, sC + 7 * h, cam, sf[J.f_exp + h], sf[J.f_exp + t], sAff + 2 * h, sAff + 2 * t,
                    sq[J.q_zero + 8 * h + 7], S.b, o);
    } else {
#pragma unroll
      for (int k = 0; k < 9; k++) o.R0[k] = 0.0f, o.M[k] = 0.0f;
#pragma unroll
      for (int k = 0; k < 3; k++) o.t0[k] = 0.0f, o.Kt[k] = 0.0f;
      o.aff[0] = o.aff[1] = o.b0 = 0.0f;
    }
    const int n2 = n * n;
    float *R0 = stage + L.off_R0 + 9 * tid, *t0 = stage + L.off_t0 + 3 * tid, *M = stage + L.off_M + 9 * tid, *Kt = stage + L.off_Kt + 3 * tid;
#pragma unroll
    for (int k = 0; k < 9; k++) R0[k] = o.R0[k], M[k] = o.M[k];
#pragma unroll
    for (int k = 0; k < 3; k++) t0[k] = o.t0[k], Kt[k] = o.Kt[k];
    stage[L.off_aff + 2 * tid] = o.aff[0], stage[L.off_aff + 2 * tid + 1] = o.aff[1], stage[L.off_b0 + tid] = o.b0;
    if (J.o_pre >= 0) { // the six tables back to back
      float *q = base + J.o_pre;
#pragma unroll
      for (int k = 0; k < 9; k++) q[9 * tid + k] = o.R0[k], q[12 * n2 + 9 * tid + k] = o.M[k];
#pragma unroll
      for (int k = 0; k < 3; k++) q[9 * n2 + 3 * tid + k] = o.t0[k], q[21 * n2 + 3 * tid + k] = o.Kt[k];
      q[24 * n2 + 2 * tid] = o.aff[0], q[24 * n2 + 2 * tid + 1] = o.aff[1], q[26 * n2 + tid] = o.b0;
    }
  }
  if (tid < N) { // E1-E3
    const double dxi = sDx[tid];
    sd[J.d_dx + tid] = dxi;
    if (J.o_dx >= 0) dbl(base, J.o_dx)[tid] = dxi;
    sTerm[tid] = stp::energy_m_term(J.d_HM >= 0 ? sd + J.d_HM + (long long)tid * N : nullptr, J.d_bM >= 0 ? sd + J.d_bM : nullptr, sDx, tid, N);
    if (J.q_prior >= 0) {
      const double pr = sq[J.q_prior + tid], dp = tid < 4 ? dxi : sState[tid - 4] - sq[J.q_pzero + tid];
      double *hl = sd + J.d_HL + (long long)tid * N + tid, *bl = sd + J.d_bL + tid;
      *hl = stp::prior_h(*hl, pr), *bl = stp::prior_b(*bl, pr, dp);
    }
  }
  __syncthreads();
  if (tid == 0) {
    double e = 0.0;
    for (int i = 0; i < N; i++) e += sTerm[i];
    *dbl(base, J.o_em) = e;
  }
  if (J.o_HL >= 0)
    for (int e = tid; e < N * N; e += kFrameBlock) dbl(base, J.o_HL)[e] = sd[J.d_HL + e];
  if (J.o_bL >= 0 && tid < N) dbl(base, J.o_bL)[tid] = sd[J.d_bL + tid];
}

__global__ __launch_bounds__(kPointBlock) void stp_point_kernel(const StpJob *jobs, const LinJob *lin_jobs, float *stage, const float *sf, float *base,
                                                                stp::Scales S) {
  const StpJob &J = jobs[blockIdx.y];
  const LinJob &L = lin_jobs[blockIdx.y];
  if (blockIdx.x == gridDim.x - 1) { // D4: the points' chains and can_break
    // the lanes form the terms of a chunk of points side by side (each one product or one fabsf, rounded as the chain's own would be),
    // lane 0 adds them in ascending point index
    __shared__ float sq[kPointBlock], ab[kPointBlock];
    float id = 0.0f, nid = 0.0f, num = 0.0f;
    for (int p0 = 0; p0 < J.n_pts; p0 += kPointBlock) {
      const int p = p0 + (int)threadIdx.x, m = min(kPointBlock, J.n_pts - p0);
      if (p < J.n_pts) sq[threadIdx.x] = stp::point_sq(sf[J.f_ids + p]), ab[threadIdx.x] = fabsf(sf[J.f_idb + p]);
      __syncthreads();
      if (threadIdx.x == 0)
        for (int k = 0; k < m; k++) id += sq[k], nid += ab[k], num += 1.0f;
      __syncthreads();
    }
    if (threadIdx.x != 0) return;
    float sums[6];
#pragma unroll
    for (int k = 0; k < 4; k++) sums[k] = base[J.o_sums + k];
    sums[4] = id / num, sums[5] = nid / num;
    base[J.o_sums + 4] = sums[4], base[J.o_sums + 5] = sums[5];
    reinterpret_cast<int *>(base)[J.o_can] = stp::can_break(sums, S.th);
    return;
  }
  const int p = blockIdx.x * kPointBlock + threadIdx.x;
  if (p >= J.n_pts) return;
  const float idepth = stp::point_idepth(sf[J.f_idb + p], J.stepfac[4], sf[J.f_ids + p]); // D3
  const float scaled = stp::point_idepth_scaled(S.idepth, idepth);
  base[J.o_idepth + p] = idepth;
  stage[L.off_id + p] = scaled, stage[L.off_idz + p] = scaled;
}

} // namespace

extern "C" int dsm_window_step_batch(dsm_context *ctx, int n_jobs, const dsm_step_job *jobs, const dsm_linearize_params *lp, const dsm_step_params *sp) {
  StpPlan P;
  int rc = step_check("dsm_window_step_batch", ctx, n_jobs, jobs, lp, sp, P);
  if (rc) return rc;
  CallArena A;
  step_layout(P, A);
  if ((rc = A.bind(ctx))) return rc;
  step_stage(P, A);
  if ((rc = A.upload())) return rc;
  if ((rc = step_launch(ctx, P, A, *lp, *sp))) return rc;
  if ((rc = A.fetch(A.out.used))) return rc;
  step_unpack(P, A, *lp);
  return DSM_OK;
}

namespace dsm {

int step_check(const char *call, dsm_context *ctx, int n_jobs, const dsm_step_job *jobs, const dsm_linearize_params *lp, const dsm_step_params *sp,
               StpPlan &P) {
  auto bad = [call](const char *msg) { return invalid((std::string(call) + ": " + msg).c_str()); };
  if (!ctx || n_jobs < 1 || !jobs) return bad("bad argument");
  if (const char *e = linearize_params_error(lp)) return bad(e);
  if (const char *e = step_params_error(sp)) return bad(e);
  size_t zeros = kMaxN;
  for (int j = 0; j < n_jobs; j++) {
    if (const char *e = step_job_error(jobs[j])) return bad(e);
    const dsm_linearize_job &L = jobs[j].sol.hes.lin;
    zeros = std::max(zeros, std::max((size_t)9 * L.n_frames * L.n_frames, (size_t)L.n_pts));
  }
  // the solve call's rules and pieces see the job completed with placeholders of the right size for what the device forms: the staged
  // zeros are overwritten by stp_frame_kernel and stp_point_kernel before any kernel reads them
  P.n_jobs = n_jobs, P.jobs = jobs;
  P.zero.assign(zeros, 0.0);
  const float *zf = reinterpret_cast<const float *>(P.zero.data());
  std::vector<dsm_solve_job> &T = P.T;
  T.resize(n_jobs);
  std::vector<const dsm_linearize_job *> lin;
  for (int j = 0; j < n_jobs; j++) {
    T[j] = jobs[j].sol;
    dsm_linearize_job &L = T[j].hes.lin;
    L.cam[0] = L.cam[1] = L.cam_inv[0] = L.cam_inv[1] = 1.0f, L.cam[2] = L.cam[3] = 0.0f;
    L.pre_RTll_0 = L.pre_tTll_0 = L.pre_KRKiTll = L.pre_KtTll = L.pre_aff_mode = L.pre_b0_mode = zf;
    L.idepth_scaled = L.idepth_zero_scaled = zf;
    T[j].delta_x = P.zero.data();
    lin.push_back(&L);
  }
  size_t res = 0;
  int rc = linearize_check_jobs(call, ctx, n_jobs, lin.data(), lp, &res);
  if (rc) return rc;
  for (int j = 0; j < n_jobs; j++) {
    if (const char *e = hessian_job_error(T[j].hes, false)) return bad(e);
    if (const char *e = solve_job_error(T[j])) return bad(e);
  }
  return DSM_OK;
}

// on top of the solve call's parts: staged [job table | doubles: eval, state_zero, state_backup, frame_step, the calibration's three,
// the priors | floats: idepth_backup, idepth_step, exposure], read back [per job: state, calib, W, energy_m, sums, can_break, idepth,
// as asked for: C, cam, the six tables, delta_x, H_L, b_L]
void step_layout(StpPlan &P, CallArena &A) {
  const int n_jobs = P.n_jobs;
  for (int j = 0; j < n_jobs; j++) P.sol.jobs.push_back(&P.T[j]);
  solve_layout(P.sol, A);
  P.at.assign(n_jobs, StpWhere());
  for (int j = 0; j < n_jobs; j++) {
    const dsm_step_job &S = P.jobs[j];
    const size_t n = S.sol.hes.lin.n_frames, np = S.sol.hes.lin.n_pts, N = 4 + 8 * n;
    StpWhere &w = P.at[j];
    P.doubles += 7 * n + 3 * 8 * n + 12 + (S.prior ? 2 * N : 0);
    P.floats += 2 * np + n;
    w.state = A.out.take(64 * n), w.calib = A.out.take(32), w.W = A.out.take(56 * n), w.em = A.out.take(8), w.sums = A.out.take(24), w.can = A.out.take(4);
    w.idepth = A.out.take(4 * np);
    if (S.cam_to_world_out) w.C = (long long)A.out.take(56 * n);
    if (S.cam_out) w.cam = (long long)A.out.take(24);
    if (S.pre_RTll_0_out || S.pre_tTll_0_out || S.pre_KRKiTll_out || S.pre_KtTll_out || S.pre_aff_mode_out || S.pre_b0_mode_out)
      w.pre = (long long)A.out.take(4 * 27 * n * n);
    if (S.delta_x_out) w.dx = (long long)A.out.take(8 * N);
    if (S.H_L_out) w.HL = (long long)A.out.take(8 * N * N);
    if (S.b_L_out) w.bL = (long long)A.out.take(8 * N);
    P.max_pts = std::max(P.max_pts, (int)np);
  }
  P.o_stp = A.in.take(sizeof(StpJob) * n_jobs), P.o_sq = A.in.take(8 * P.doubles), P.o_sf = A.in.take(4 * P.floats);
  P.stp_stride = sizeof(StpJob), P.stp_stepfac = offsetof(StpJob, stepfac);
}

void step_stage(StpPlan &P, CallArena &A) {
  const int n_jobs = P.n_jobs;
  solve_stage(P.sol, A);
  StpJob *hj = A.host_in<StpJob>(P.o_stp);
  double *hq = A.host_in<double>(P.o_sq);
  WordPacker F{A.host_in<float>(P.o_sf)};
  size_t used = 0;
  auto put = [&](const double *a, size_t m) {
    memcpy(hq + used, a, 8 * m);
    used += m;
    return (int)(used - m);
  };
  const long long out0 = P.sol.hes.out0;
  auto word = [out0](long long bytes) { return bytes < 0 ? -1ll : out0 + bytes / 4; };
  P.view.assign(n_jobs, StpView());
  for (int j = 0; j < n_jobs; j++) {
    const dsm_step_job &S = P.jobs[j];
    const size_t n = S.sol.hes.lin.n_frames, np = S.sol.hes.lin.n_pts, N = 4 + 8 * n;
    const StpWhere &w = P.at[j];
    const SolView &V = P.sol.view[j];
    StpJob &G = hj[j];
    memset(&G, 0, sizeof G);
    G.n = (int)n, G.n_pts = (int)np, G.N = (int)N;
    memcpy(G.stepfac, S.stepfac, sizeof G.stepfac);
    G.q_eval = put(S.world_to_cam_eval, 7 * n), G.q_zero = put(S.state_zero, 8 * n), G.q_backup = put(S.state_backup, 8 * n);
    G.q_step = put(S.frame_step, 8 * n), G.q_czero = put(S.calib_zero, 4), G.q_cbackup = put(S.calib_backup, 4), G.q_cstep = put(S.calib_step, 4);
    G.q_prior = S.prior ? put(S.prior, N) : -1, G.q_pzero = S.prior ? put(S.prior_zero, N) : -1;
    F.put(&G.f_idb, S.idepth_backup, np), F.put(&G.f_ids, S.idepth_step, np), F.put(&G.f_exp, S.exposure, n);
    G.d_HL = V.d_HL, G.d_bL = V.d_bL, G.d_HM = V.d_HM, G.d_bM = V.d_bM, G.d_dx = V.d_dx;
    G.o_state = word((long long)w.state), G.o_calib = word((long long)w.calib), G.o_idepth = word((long long)w.idepth), G.o_W = word((long long)w.W);
    G.o_can = word((long long)w.can), G.o_sums = word((long long)w.sums), G.o_em = word((long long)w.em);
    G.o_C = word(w.C), G.o_cam = word(w.cam), G.o_pre = word(w.pre), G.o_dx = word(w.dx), G.o_HL = word(w.HL), G.o_bL = word(w.bL);
    P.view[j] = StpView{G.q_backup, G.q_step, G.q_cbackup, G.q_cstep, G.q_prior, G.f_idb, G.f_ids, G.o_state, G.o_calib, G.o_idepth, G.o_em, G.o_can, G.o_W};
  }
}

int step_launch(dsm_context *ctx, StpPlan &P, CallArena &A, const dsm_linearize_params &lp, const dsm_step_params &sp) {
  const stp::Scales Sc{sp.scale_xi_trans, sp.scale_xi_rot, sp.scale_a, sp.scale_b, sp.th_opt_iterations, lp.scale_f, lp.scale_c, lp.scale_idepth};
  const StpJob *dj = A.dev_in<const StpJob>(P.o_stp);
  LinJob *dl = A.dev_in<LinJob>(P.sol.hes.o_lin);
  float *dstage = A.dev_in<float>(P.sol.hes.o_stage);
  hipLaunchKernelGGL(stp_frame_kernel, dim3(P.n_jobs), dim3(kFrameBlock), 0, ctx->stream, dj, dl, dstage, A.dev_in<double>(P.sol.o_sd),
                     A.dev_in<const double>(P.o_sq), A.dev_in<const float>(P.o_sf), P.sol.hes.dev_base, Sc);
  hipLaunchKernelGGL(stp_point_kernel, dim3((P.max_pts + kPointBlock - 1) / kPointBlock + 1, P.n_jobs), dim3(kPointBlock), 0, ctx->stream, dj, dl, dstage,
                     A.dev_in<const float>(P.o_sf), P.sol.hes.dev_base, Sc);
  DSM_HIP(hipGetLastError());
  return solve_launch(ctx, P.sol, A, lp);
}

void step_unpack(const StpPlan &P, const CallArena &A, const dsm_linearize_params &lp) {
  solve_unpack(P.sol, A, lp);
  const unsigned char *ho = A.host_out<unsigned char>(0);
  for (int j = 0; j < P.n_jobs; j++) {
    const dsm_step_job &S = P.jobs[j];
    const size_t n = S.sol.hes.lin.n_frames, np = S.sol.hes.lin.n_pts, N = 4 + 8 * n, n2 = n * n;
    const StpWhere &w = P.at[j];
    memcpy(S.state_out, ho + w.state, 64 * n), memcpy(S.calib_out, ho + w.calib, 32), memcpy(S.world_to_cam_out, ho + w.W, 56 * n);
    if (np) memcpy(S.idepth_out, ho + w.idepth, 4 * np);
    memcpy(S.can_break, ho + w.can, 4), memcpy(S.step_sums, ho + w.sums, 24), memcpy(S.energy_m, ho + w.em, 8);
    if (S.cam_to_world_out) memcpy(S.cam_to_world_out, ho + w.C, 56 * n);
    if (S.cam_out) memcpy(S.cam_out, ho + w.cam, 24);
    const unsigned char *pre = ho + (w.pre < 0 ? 0 : w.pre);
    if (S.pre_RTll_0_out) memcpy(S.pre_RTll_0_out, pre, 36 * n2);
    if (S.pre_tTll_0_out) memcpy(S.pre_tTll_0_out, pre + 36 * n2, 12 * n2);
    if (S.pre_KRKiTll_out) memcpy(S.pre_KRKiTll_out, pre + 48 * n2, 36 * n2);
    if (S.pre_KtTll_out) memcpy(S.pre_KtTll_out, pre + 84 * n2, 12 * n2);
    if (S.pre_aff_mode_out) memcpy(S.pre_aff_mode_out, pre + 96 * n2, 8 * n2);
    if (S.pre_b0_mode_out) memcpy(S.pre_b0_mode_out, pre + 104 * n2, 4 * n2);
    if (S.delta_x_out) memcpy(S.delta_x_out, ho + w.dx, 8 * N);
    if (S.H_L_out) memcpy(S.H_L_out, ho + w.HL, 8 * N * N);
    if (S.b_L_out) memcpy(S.b_L_out, ho + w.bL, 8 * N);
  }
}

} // namespace dsm

