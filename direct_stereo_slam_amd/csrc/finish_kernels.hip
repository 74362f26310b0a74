// finish_kernels.hip -- what FrontEnd::optimize does behind its loop (dso_helpers/FrontEndOptimize.cpp:455-486, :39-72, :145-176,
// :504-523) on the device, in the same call as the loop, for the windows of many sequences.  Semantics: Z1-Z8, V of DESIGN.md section 22.
//
// One dsm_window_finish_batch = the staged copy and the passes of dsm_window_optimize_batch (optimize_launch.hpp) with the finish's
// inputs on top, and behind the call's last pass FOUR launches on the same stream and arena:
//   fin_frame_kernel   workgroup 0 of a job, 256 lanes.  Lanes k < n: Z1 and D2 at the new evaluation point (the double sincos lives
//                      here); lanes 0-3: D1's cam and c_delta at the committed calibration.  Poses, aff and the states pass through
//                      LDS across one barrier.  Lane h n + t: Q1-Q4 of pair (h, t), written where the finish's OWN LinJob reads its
//                      precalc tables; for a pair of the newest frame Z2's two matrices, written to the read-back part; then the
//                      pair's eight adHTdeltaF entries, from those or from the job's staged matrices.  The job's OTHER workgroups,
//                      one lane per residual: the state and energy the last pass left in its heads become the final
//                      linearisation's inputs, with the is_new bit.
//   linearize_kernel   (linearize_kernels.hip, unchanged) on the finish's job table, with the fix flag: Z4
//   fin_point_kernel   one lane per point over its staged residual list in ascending index: Z5, Z6
//   fin_prefix_kernel  one 256-lane workgroup per job: tiles of 256 residuals, then of 256 points, with a running offset in ascending
//                      index (Z7; counts within a tile by ballot, integers have no order to pin); on the residuals' walk the lanes
//                      stage the tile's new_energy in LDS as doubles and lane 0 adds them in ascending index (B1); lane 0 forms Z8.
// The four read what the loop's last pass left (the heads, the state, the calibration, world_to_cam, the scaled depths, frame_energy_th)
// and write ONLY a region of their own, so the loop's outputs stay those of the last pass.  They run once: with force_accept right
// behind the passes (one host wait), otherwise after the read-back that tells whether more passes are needed (two).  Every result is one sequential chain in one lane;
// no kernel waits for another workgroup; no atomics; no scratch; no MFMA.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "optimize_launch.hpp"

#include "finish_math.hpp"

using namespace dsm;

namespace {

constexpr int kBlock = 256;
constexpr int kMaxF = DSM_WINDOW_MAX_FRAMES;
static_assert(kMaxF * kMaxF <= kBlock, "one lane per pair");

struct FinJob {
  int n, n_pts, n_res, N;
  int q_eval, q_zero, q_czero, q_adh, q_adt; // doubles into the finish's staged doubles
  // 4-byte words from the start of the loop's staged inputs (what linearize_kernel's off_* count from): the finish's staged inputs,
  int f_exp, f_isnew, f_ngood, f_mrb, f_lastres, f_laststate;
  // ... the inputs of the final linearisation, which fin_frame_kernel writes (the six tables are the finish LinJob's off_*),
  int f_eth, f_flags, f_ein;
  // ... and what the loop staged: frame_energy_th and the points' residual lists
  int off_eth, off_pt_start, off_pt_list;
  // 4-byte words from the start of the arena's device-only part: what the loop's last pass left ...
  long long o_state, o_calib, o_W, o_head;
  // ... and the finish's part of the read-back (o_C -1: not asked for)
  long long o_eval, o_zero, o_st, o_C, o_ad, o_adht, o_cd, o_dx, o_pre, o_cam, o_fhead, o_ngood, o_mrb, o_lastres, o_laststate, o_kept, o_dropped,
      o_residx, o_ptidx, o_scal;
};

struct Scalars { // o_scal
  double energy;
  int n_res_out, n_pts_out, lost;
  float rmse;
};

__device__ __forceinline__ double *dbl(float *base, long long word) { return reinterpret_cast<double *>(base + word); }

__global__ __launch_bounds__(kBlock) void fin_frame_kernel(const FinJob *jobs, LinJob *lin_jobs, const opt::State *states, float *stage, const double *fq,
                                                           float *base, stp::Scales S) {
  const FinJob &J = jobs[blockIdx.y];
  LinJob &L = lin_jobs[blockIdx.y];
  const int n = J.n, f = n - 1, tid = threadIdx.x;
  if (blockIdx.x > 0) { // Z4's inputs, one lane per residual: the last pass's new_state / new_energy are the committed ones (applyRes), with the is_new bit
    const int r = (blockIdx.x - 1) * kBlock + tid;
    if (r < J.n_res) {
      const float *head = base + J.o_head + (long long)kLinHeadWords * r;
      reinterpret_cast<int *>(stage)[J.f_flags + r] = (__float_as_int(head[0]) & 0xff) | (reinterpret_cast<const int *>(stage)[J.f_isnew + r] ? 256 : 0);
      stage[J.f_ein + r] = head[1];
    }
    return; // uniform over the workgroup
  }
  __shared__ double sEval[kMaxF * 7], sEi[kMaxF * 7], sW[kMaxF * 7], sC[kMaxF * 7], sAff[kMaxF * 2], sAff0[kMaxF * 2], sState[kMaxF * 8], sZero[kMaxF * 8];
  __shared__ float sCam[6];
  if (tid < n) { // Z1, then D2 on the primed values
    double state[8], zero[8], eval[7], delta_f[8], aff[2], aff0[2], W[7], C[7], Ei[7];
    const double *st = dbl(base, J.o_state) + 8 * tid;
#pragma unroll
    for (int k = 0; k < 8; k++) state[k] = st[k], zero[k] = fq[J.q_zero + 8 * tid + k];
#pragma unroll
    for (int k = 0; k < 7; k++) eval[k] = fq[J.q_eval + 7 * tid + k];
    if (tid == f) {
      const double *Wf = dbl(base, J.o_W) + 7 * f;
#pragma unroll
      for (int k = 0; k < 7; k++) eval[k] = Wf[k];
      double fresh[8];
      fin::newest_state(state, fresh);
#pragma unroll
      for (int k = 0; k < 8; k++) state[k] = zero[k] = fresh[k];
    }
    fin::frame_pose(state, zero, eval, S, delta_f, aff, aff0, W, C);
    stp::se3_inverse(eval, Ei);
    double *eval_out = dbl(base, J.o_eval) + 7 * tid, *zero_out = dbl(base, J.o_zero) + 8 * tid, *st_out = dbl(base, J.o_st) + 8 * tid;
    double *dx = dbl(base, J.o_dx) + 4 + 8 * tid;
#pragma unroll
    for (int k = 0; k < 8; k++) sState[8 * tid + k] = state[k], sZero[8 * tid + k] = zero[k], st_out[k] = state[k], zero_out[k] = zero[k], dx[k] = delta_f[k];
#pragma unroll
    for (int k = 0; k < 7; k++) sEval[7 * tid + k] = eval[k], sEi[7 * tid + k] = Ei[k], sW[7 * tid + k] = W[k], sC[7 * tid + k] = C[k], eval_out[k] = eval[k];
    if (J.o_C >= 0) {
      double *C_out = dbl(base, J.o_C) + 7 * tid;
#pragma unroll
      for (int k = 0; k < 7; k++) C_out[k] = C[k];
    }
    sAff[2 * tid] = aff[0], sAff[2 * tid + 1] = aff[1], sAff0[2 * tid] = aff0[0], sAff0[2 * tid + 1] = aff0[1];
    stage[J.f_eth + tid] = tid == f ? states[blockIdx.y].eth_out : stage[J.off_eth + tid]; // Z4: what stands after the last pass
  }
  if (tid < 4) { // D1 at the committed calibration
    float cam, c_delta;
    fin::calib_cam(tid, dbl(base, J.o_calib)[tid], fq[J.q_czero + tid], S, cam, c_delta);
    sCam[tid] = cam, base[J.o_cd + tid] = c_delta, dbl(base, J.o_dx)[tid] = (double)c_delta; // E1's first four
    if (tid < 2) sCam[4 + tid] = stp::cam_inverse(cam);
  }
  __syncthreads();
  if (tid == 0) L.fx = sCam[0], L.fy = sCam[1], L.cx = sCam[2], L.cy = sCam[3], L.fxi = sCam[4], L.fyi = sCam[5];
  if (tid < 6) base[J.o_cam + tid] = sCam[tid];
  if (tid < n * n) {
    const int h = tid / n, t = tid - h * n, n2 = n * n;
    const float exp_h = stage[J.f_exp + h], exp_t = stage[J.f_exp + t];
    stp::PairRow o;
    if (h != t) { // Q1-Q4
      float cam[6];
#pragma unroll
      for (int k = 0; k < 6; k++) cam[k] = sCam[k];
      stp::pair_row(sEval + 7 * t, sEi + 7 * h, sW + 7 * t, sC + 7 * h, cam, exp_h, exp_t, sAff + 2 * h, sAff + 2 * t, sZero[8 * h + 7], S.b, o);
    } else {
#pragma unroll
      for (int k = 0; k < 9; k++) o.R0[k] = 0.0f, o.M[k] = 0.0f;
#pragma unroll
      for (int k = 0; k < 3; k++) o.t0[k] = 0.0f, o.Kt[k] = 0.0f;
      o.aff[0] = o.aff[1] = o.b0 = 0.0f;
    }
    float *R0 = stage + L.off_R0 + 9 * tid, *t0 = stage + L.off_t0 + 3 * tid, *M = stage + L.off_M + 9 * tid, *Kt = stage + L.off_Kt + 3 * tid;
    float *q = base + J.o_pre; // the six tables back to back
#pragma unroll
    for (int k = 0; k < 9; k++) R0[k] = o.R0[k], M[k] = o.M[k], q[9 * tid + k] = o.R0[k], q[12 * n2 + 9 * tid + k] = o.M[k];
#pragma unroll
    for (int k = 0; k < 3; k++) t0[k] = o.t0[k], Kt[k] = o.Kt[k], q[9 * n2 + 3 * tid + k] = o.t0[k], q[21 * n2 + 3 * tid + k] = o.Kt[k];
    stage[L.off_aff + 2 * tid] = o.aff[0], stage[L.off_aff + 2 * tid + 1] = o.aff[1], stage[L.off_b0 + tid] = o.b0;
    q[24 * n2 + 2 * tid] = o.aff[0], q[24 * n2 + 2 * tid + 1] = o.aff[1], q[26 * n2 + tid] = o.b0;

    const double *ah = fq + J.q_adh + 64 * tid, *at = fq + J.q_adt + 64 * tid;
    if (h == f || t == f) { // Z2: slot t for (f, t), slot n + h for (h, f), h < f; the two matrices back to back
      double *slot = dbl(base, J.o_ad) + 128 * (h == f ? t : n + h);
      double Adj[36];
      fin::adjoint(sEval + 7 * t, sEi + 7 * h, Adj);
      fin::adjoint_pair(Adj, fin::aff_a0(sAff0 + 2 * h, sAff0 + 2 * t, exp_h, exp_t), S, slot, slot + 64);
      ah = slot, at = slot + 64;
    }
    float *dp = base + J.o_adht + 8 * tid; // Z3: setDeltaF
    for (int c = 0; c < 8; c++)
      dp[c] = h != t ? ad_ht_delta_entry(ah, at, sState + 8 * h, sZero + 8 * h, sState + 8 * t, sZero + 8 * t, c) : 0.0f;
  }
}

struct DevRes { // the final linearisation as finish_math.hpp's point_book asks for it
  const float *head;
  const int *flags;
  __device__ bool keep(int r) const { return (__float_as_int(head[(long long)kLinHeadWords * r]) >> 8) & 1; }
  __device__ bool is_new(int r) const { return (flags[r] >> 8) != 0; }
  __device__ float rel_bs(int r) const { return head[(long long)kLinHeadWords * r + 3]; }
  __device__ int new_state(int r) const { return __float_as_int(head[(long long)kLinHeadWords * r]) & 0xff; }
};

__global__ __launch_bounds__(kBlock) void fin_point_kernel(const FinJob *jobs, const float *stage, float *base) {
  const FinJob &J = jobs[blockIdx.y];
  const int p = blockIdx.x * kBlock + threadIdx.x;
  if (p >= J.n_pts) return;
  const int *stage_i = reinterpret_cast<const int *>(stage);
  const int s = stage_i[J.off_pt_start + p], e = stage_i[J.off_pt_start + p + 1];
  const DevRes R{base + J.o_fhead, stage_i + J.f_flags};
  const int last_res[2] = {stage_i[J.f_lastres + 2 * p], stage_i[J.f_lastres + 2 * p + 1]};
  const int last_state[2] = {stage_i[J.f_laststate + 2 * p], stage_i[J.f_laststate + 2 * p + 1]};
  fin::PointBook b;
  fin::point_book(stage_i + J.off_pt_list + s, e - s, R, stage_i[J.f_ngood + p], stage[J.f_mrb + p], last_res, last_state, b);
  int *out_i = reinterpret_cast<int *>(base);
  out_i[J.o_ngood + p] = b.n_good, base[J.o_mrb + p] = b.max_rel_baseline;
  out_i[J.o_lastres + 2 * p] = b.last_res[0], out_i[J.o_lastres + 2 * p + 1] = b.last_res[1];
  unsigned char *ls = reinterpret_cast<unsigned char *>(base + J.o_laststate);
  ls[2 * p] = b.last_state[0], ls[2 * p + 1] = b.last_state[1];
  out_i[J.o_kept + p] = b.n_kept;
  reinterpret_cast<unsigned char *>(base + J.o_dropped)[p] = b.dropped;
}

// the index of every set flag of a tile among the set ones, from `running` on; every lane of the workgroup calls it
__device__ __forceinline__ int tile_index(bool flag, int &running, unsigned *wave_count) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long mask = __ballot(flag);
  if (lane == 0) wave_count[wave] = (unsigned)__popcll(mask);
  __syncthreads();
  int before = running, total = 0;
  for (int k = 0; k < kBlock / 64; k++) {
    if (k < wave) before += (int)wave_count[k];
    total += (int)wave_count[k];
  }
  running += total;
  return before + __popcll(mask & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(kBlock) void fin_prefix_kernel(const FinJob *jobs, float *base) {
  const FinJob &J = jobs[blockIdx.x];
  const int tid = threadIdx.x;
  __shared__ double sE[kBlock];
  __shared__ unsigned sCount[2][kBlock / 64];
  int *out_i = reinterpret_cast<int *>(base);
  double e = 0.0;
  int kept = 0, stay = 0, tile = 0;
  for (int r0 = 0; r0 < J.n_res; r0 += kBlock, tile++) { // Z7 over the residuals, B1
    const int r = r0 + tid, m = min(kBlock, J.n_res - r0);
    bool flag = false;
    if (r < J.n_res) {
      const float *head = base + J.o_fhead + (long long)kLinHeadWords * r;
      flag = (__float_as_int(head[0]) >> 8) & 1;
      sE[tid] = (double)head[1];
    }
    const int at = tile_index(flag, kept, sCount[tile & 1]); // (its barrier also publishes the tile's energies)
    if (r < J.n_res) out_i[J.o_residx + r] = flag ? at : -1;
    if (tid == 0) {
      if (m == kBlock) { // sixteen values ahead in registers, as opt_decide_kernel's B1d: the LDS latency stays off the chain of adds
        double a[16], b[16];
#pragma unroll
        for (int i = 0; i < 16; i++) a[i] = sE[i];
        for (int k = 0; k < kBlock; k += 32) {
#pragma unroll
          for (int i = 0; i < 16; i++) b[i] = sE[k + 16 + i];
#pragma unroll
          for (int i = 0; i < 16; i++) e += a[i];
#pragma unroll
          for (int i = 0; i < 16; i++) a[i] = sE[(k + 32 + i) & (kBlock - 1)]; // (the last trip reads the tile's head again, unused)
#pragma unroll
          for (int i = 0; i < 16; i++) e += b[i];
        }
      } else {
        for (int k = 0; k < m; k++) e += sE[k];
      }
    }
    __syncthreads();
  }
  const unsigned char *dropped = reinterpret_cast<const unsigned char *>(base + J.o_dropped);
  for (int p0 = 0; p0 < J.n_pts; p0 += kBlock, tile++) { // Z7 over the points
    const int p = p0 + tid;
    const bool flag = p < J.n_pts && !dropped[p];
    const int at = tile_index(flag, stay, sCount[tile & 1]);
    if (p < J.n_pts) out_i[J.o_ptidx + p] = flag ? at : -1;
  }
  if (tid == 0) { // Z8
    Scalars *o = reinterpret_cast<Scalars *>(base + J.o_scal);
    o->energy = e, o->n_res_out = kept, o->n_pts_out = stay, o->lost = fin::lost(e), o->rmse = fin::rmse(e, kept);
  }
}

struct FinWhere { // bytes into out
  size_t eval, zero, st, ad, adht, cd, dx, pre, cam, head, ngood, mrb, lastres, laststate, kept, dropped, residx, ptidx, scal;
  long long C = -1, J = -1;
};

} // namespace

extern "C" int dsm_window_finish_batch(dsm_context *ctx, int n_jobs, const dsm_finish_job *jobs, const dsm_linearize_params *lp,
                                       const dsm_step_params *sp, const dsm_optimize_params *op) {
  auto bad = [](const char *msg) { return invalid((std::string("dsm_window_finish_batch: ") + msg).c_str()); };
  std::vector<const dsm_optimize_job *> list;
  for (int j = 0; jobs && j < n_jobs; j++) list.push_back(&jobs[j].opt);
  OptPlan P;
  int rc = optimize_check("dsm_window_finish_batch", ctx, n_jobs, jobs ? list.data() : nullptr, lp, sp, op, P);
  if (rc) return rc;
  for (int j = 0; j < n_jobs; j++)
    if (const char *e = finish_job_error(jobs[j])) return bad(e);

  // on top of the optimize call's parts: staged [job table | the finish's LinJob table | doubles: eval, state_zero, calib_zero, ad_host,
  // ad_target | words: exposure, is_new, the points' counters and last residuals; then, written by fin_frame_kernel, the six tables,
  // frame_energy_th, flags and energy_in of the final linearisation], read back [per job: the outputs of Z1-Z8]
  CallArena A;
  optimize_layout(P, A);
  std::vector<FinWhere> at(n_jobs);
  size_t doubles = 0, words = 0;
  int max_res = 0, max_pts = 0;
  for (int j = 0; j < n_jobs; j++) {
    const dsm_linearize_job &L = jobs[j].opt.step.sol.hes.lin;
    const size_t n = L.n_frames, np = L.n_pts, nr = L.n_res, N = 4 + 8 * n, n2 = n * n;
    doubles += 7 * n + 8 * n + 4 + 128 * n2;
    words += n + nr + 6 * np + 27 * n2 + n + 2 * nr;
    FinWhere &w = at[j];
    w.eval = A.out.take(56 * n), w.zero = A.out.take(64 * n), w.st = A.out.take(64 * n), w.ad = A.out.take(8 * 128 * (2 * n - 1));
    w.adht = A.out.take(32 * n2), w.cd = A.out.take(16), w.dx = A.out.take(8 * N), w.pre = A.out.take(4 * 27 * n2), w.cam = A.out.take(24);
    w.head = A.out.take(4 * kLinHeadWords * nr), w.ngood = A.out.take(4 * np), w.mrb = A.out.take(4 * np), w.lastres = A.out.take(8 * np);
    w.laststate = A.out.take(2 * np), w.kept = A.out.take(4 * np), w.dropped = A.out.take(np), w.residx = A.out.take(4 * nr);
    w.ptidx = A.out.take(4 * np), w.scal = A.out.take(sizeof(Scalars));
    if (jobs[j].cam_to_world_out) w.C = (long long)A.out.take(56 * n);
    if (jobs[j].J_out && nr) w.J = (long long)A.out.take(4 * lin::J_FLOATS * nr);
    max_res = std::max(max_res, L.n_res), max_pts = std::max(max_pts, L.n_pts);
  }
  const size_t o_fin = A.in.take(sizeof(FinJob) * n_jobs), o_flin = A.in.take(sizeof(LinJob) * n_jobs), o_fq = A.in.take(8 * doubles),
               o_fw = A.in.take(4 * words);
  if ((rc = A.bind(ctx))) return rc;
  optimize_stage(P, A, *op);

  const HesPlan &H = P.stp.sol.hes;
  const long long out0 = H.out0;
  auto word = [out0](long long bytes) { return bytes < 0 ? -1ll : out0 + bytes / 4; };
  FinJob *hj = A.host_in<FinJob>(o_fin);
  LinJob *hf = A.host_in<LinJob>(o_flin);
  const LinJob *hl = A.host_in<LinJob>(H.o_lin);
  double *hq = A.host_in<double>(o_fq);
  WordPacker W{A.host_in<float>(o_fw)};
  const int rel = (int)((o_fw - H.o_stage) / 4); // the finish's words as the loop's stage pointer counts them
  size_t used = 0;
  auto put = [&](const double *a, size_t m) {
    memcpy(hq + used, a, 8 * m);
    used += m;
    return (int)(used - m);
  };
  for (int j = 0; j < n_jobs; j++) {
    const dsm_finish_job &F = jobs[j];
    const dsm_step_job &S = F.opt.step;
    const dsm_linearize_job &L = S.sol.hes.lin;
    const size_t n = L.n_frames, np = L.n_pts, nr = L.n_res, n2 = n * n;
    const FinWhere &w = at[j];
    const StpView &V = P.stp.view[j];
    FinJob &G = hj[j];
    memset(&G, 0, sizeof G);
    G.n = (int)n, G.n_pts = (int)np, G.n_res = (int)nr, G.N = (int)(4 + 8 * n);
    G.q_eval = put(S.world_to_cam_eval, 7 * n), G.q_zero = put(S.state_zero, 8 * n), G.q_czero = put(S.calib_zero, 4);
    G.q_adh = put(S.sol.hes.ad_host, 64 * n2), G.q_adt = put(S.sol.hes.ad_target, 64 * n2);
    W.put(&G.f_exp, S.exposure, n);
    int *is_new = (int *)W.reserve(&G.f_isnew, nr), *last_state = nullptr;
    for (size_t r = 0; r < nr; r++) is_new[r] = L.is_new[r] != 0;
    W.put(&G.f_ngood, F.n_good_residuals_in, np), W.put(&G.f_mrb, F.max_rel_baseline_in, np), W.put(&G.f_lastres, F.last_res, 2 * np);
    last_state = (int *)W.reserve(&G.f_laststate, 2 * np);
    for (size_t i = 0; i < 2 * np; i++) last_state[i] = F.last_state_in[i];
    LinJob &D = hf[j]; // the loop's entry with the finish's own tables, inputs and outputs
    D = hl[j];
    D.fix = 1;
    W.reserve(&D.off_R0, 9 * n2), W.reserve(&D.off_t0, 3 * n2), W.reserve(&D.off_M, 9 * n2), W.reserve(&D.off_Kt, 3 * n2);
    W.reserve(&D.off_aff, 2 * n2), W.reserve(&D.off_b0, n2), W.reserve(&D.off_eth, n), W.reserve(&D.off_flags, nr), W.reserve(&D.off_ein, nr);
    int *mine[] = {&G.f_exp, &G.f_isnew, &G.f_ngood, &G.f_mrb, &G.f_lastres, &G.f_laststate, &D.off_R0, &D.off_t0, &D.off_M,
                   &D.off_Kt, &D.off_aff, &D.off_b0, &D.off_eth, &D.off_flags, &D.off_ein};
    for (int *o : mine) *o += rel;
    G.f_eth = D.off_eth, G.f_flags = D.off_flags, G.f_ein = D.off_ein;
    D.o_head = word((long long)w.head), D.o_J = word(w.J), D.o_cpt = -1, D.o_proj = -1;
    G.off_eth = hl[j].off_eth, G.off_pt_start = H.view[j].off_pt_start, G.off_pt_list = H.view[j].off_pt_list;
    G.o_state = V.o_state, G.o_calib = V.o_calib, G.o_W = V.o_W, G.o_head = hl[j].o_head;
    G.o_eval = word((long long)w.eval), G.o_zero = word((long long)w.zero), G.o_st = word((long long)w.st), G.o_C = word(w.C);
    G.o_ad = word((long long)w.ad), G.o_adht = word((long long)w.adht), G.o_cd = word((long long)w.cd), G.o_dx = word((long long)w.dx);
    G.o_pre = word((long long)w.pre), G.o_cam = word((long long)w.cam), G.o_fhead = D.o_head, G.o_ngood = word((long long)w.ngood);
    G.o_mrb = word((long long)w.mrb), G.o_lastres = word((long long)w.lastres), G.o_laststate = word((long long)w.laststate);
    G.o_kept = word((long long)w.kept), G.o_dropped = word((long long)w.dropped), G.o_residx = word((long long)w.residx);
    G.o_ptidx = word((long long)w.ptidx), G.o_scal = word((long long)w.scal);
  }
  if ((rc = A.upload())) return rc;

  const stp::Scales Sc{sp->scale_xi_trans, sp->scale_xi_rot, sp->scale_a, sp->scale_b, sp->th_opt_iterations, lp->scale_f, lp->scale_c, lp->scale_idepth};
  const dsm_window *win = jobs[0].opt.step.sol.hes.lin.window;
  auto finish = [&]() {
    const FinJob *dj = A.dev_in<const FinJob>(o_fin);
    float *stage = A.dev_in<float>(H.o_stage);
    hipLaunchKernelGGL(fin_frame_kernel, dim3(1 + (max_res + kBlock - 1) / kBlock, n_jobs), dim3(kBlock), 0, ctx->stream, dj, A.dev_in<LinJob>(o_flin), optimize_dev_states(P, A), stage,
                       A.dev_in<const double>(o_fq), H.dev_base, Sc);
    DSM_HIP(hipGetLastError());
    if (max_res)
      if (int e = linearize_launch(ctx, n_jobs, max_res, A.dev_in<const LinJob>(o_flin), stage, H.dev_base, win->w, win->h, *lp)) return e;
    if (max_pts) hipLaunchKernelGGL(fin_point_kernel, dim3((max_pts + kBlock - 1) / kBlock, n_jobs), dim3(kBlock), 0, ctx->stream, dj, stage, H.dev_base);
    hipLaunchKernelGGL(fin_prefix_kernel, dim3(n_jobs), dim3(kBlock), 0, ctx->stream, dj, H.dev_base);
    DSM_HIP(hipGetLastError());
    return (int)DSM_OK;
  };
  // The finish runs ONCE, behind the call's last pass.  force_accept: every job's pass count is known in advance, the finish follows
  // the passes at once and the call has one host wait.  Otherwise the read-back of the first group tells whether a job rejected a step
  // and needs the remaining passes; the finish follows them, or the first group if none are needed, and the call has two host waits.
  const bool known = op->force_accept != 0;
  if ((rc = optimize_passes(ctx, P, A, *lp, *sp, 1 + P.max_it))) return rc;
  if (known && (rc = finish())) return rc;
  if ((rc = A.fetch(A.out.used))) return rc;
  if (!known) {
    if (optimize_unfinished(P, A) && (rc = optimize_passes(ctx, P, A, *lp, *sp, P.max_it))) return rc;
    if ((rc = finish())) return rc;
    if ((rc = A.fetch(A.out.used))) return rc;
  }
  optimize_unpack(P, A, *lp);

  const unsigned char *ho = A.host_out<unsigned char>(0);
  for (int j = 0; j < n_jobs; j++) {
    const dsm_finish_job &F = jobs[j];
    const dsm_hessian_job &Hj = F.opt.step.sol.hes;
    const dsm_linearize_job &L0 = Hj.lin;
    const size_t n = L0.n_frames, np = L0.n_pts, nr = L0.n_res, n2 = n * n, f = n - 1;
    const FinWhere &w = at[j];
    memcpy(F.world_to_cam_eval_out, ho + w.eval, 56 * n), memcpy(F.state_zero_out, ho + w.zero, 64 * n), memcpy(F.state_out, ho + w.st, 64 * n);
    memcpy(F.ad_host_out, Hj.ad_host, 512 * n2), memcpy(F.ad_target_out, Hj.ad_target, 512 * n2);
    for (size_t h = 0; h < n; h++)
      for (size_t t = 0; t < n; t++) {
        if (h != f && t != f) continue;
        const unsigned char *slot = ho + w.ad + 1024 * (h == f ? t : n + h);
        memcpy(F.ad_host_out + 64 * (h * n + t), slot, 512), memcpy(F.ad_target_out + 64 * (h * n + t), slot + 512, 512);
      }
    memcpy(F.ad_ht_delta_out, ho + w.adht, 32 * n2), memcpy(F.c_delta_out, ho + w.cd, 16), memcpy(F.delta_x_out, ho + w.dx, 8 * (4 + 8 * n));
    const unsigned char *pre = ho + w.pre;
    memcpy(F.pre_RTll_0_out, pre, 36 * n2), memcpy(F.pre_tTll_0_out, pre + 36 * n2, 12 * n2), memcpy(F.pre_KRKiTll_out, pre + 48 * n2, 36 * n2);
    memcpy(F.pre_KtTll_out, pre + 84 * n2, 12 * n2), memcpy(F.pre_aff_mode_out, pre + 96 * n2, 8 * n2), memcpy(F.pre_b0_mode_out, pre + 104 * n2, 4 * n2);
    memcpy(F.cam_out, ho + w.cam, 24);
    if (F.cam_to_world_out) memcpy(F.cam_to_world_out, ho + w.C, 56 * n);
    // Z4: the heads; B2 on the host from the read-back, as dsm_linearize_residuals_batch forms it (B1 is the device's ordered sum)
    dsm_linearize_job L = L0;
    double host_energy = 0.0;
    L.fix_linearization = 1, L.new_state = F.new_state, L.new_energy = F.new_energy, L.new_energy_with_outlier = F.new_energy_with_outlier;
    L.keep = F.keep, L.rel_bs = F.rel_bs, L.J_out = F.J_out, L.center_projected_to = nullptr, L.projected_to = nullptr;
    L.energy_out = &host_energy, L.new_frame_energy_th_out = F.frame_energy_th_out;
    linearize_unpack(L, reinterpret_cast<const float *>(ho), (long long)(w.head / 4), -1, -1, w.J < 0 ? -1 : w.J / 4);
    linearize_job_summary(L, *lp);
    if (np) {
      memcpy(F.n_good_residuals_out, ho + w.ngood, 4 * np), memcpy(F.max_rel_baseline_out, ho + w.mrb, 4 * np), memcpy(F.last_res_out, ho + w.lastres, 8 * np);
      memcpy(F.last_state_out, ho + w.laststate, 2 * np), memcpy(F.n_res_kept, ho + w.kept, 4 * np), memcpy(F.point_dropped, ho + w.dropped, np);
      memcpy(F.point_index_out, ho + w.ptidx, 4 * np);
    }
    if (nr) memcpy(F.res_index_out, ho + w.residx, 4 * nr);
    const Scalars &sc = *reinterpret_cast<const Scalars *>(ho + w.scal);
    *F.energy = sc.energy, *F.n_res_out = sc.n_res_out, *F.n_pts_out = sc.n_pts_out, *F.lost = sc.lost, *F.rmse = sc.rmse;
  }
  return DSM_OK;
}
