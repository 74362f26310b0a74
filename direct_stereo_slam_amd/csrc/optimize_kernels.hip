// optimize_kernels.hip -- the accept / reject loop of FrontEnd::optimize (dso_helpers/FrontEndOptimize.cpp:362-371, :382-453) on the
// device, for the windows of many sequences in one call, every window with its own lambda, factors, iteration count and break.
// Semantics: O1-O4, B1d, B2d, C, Z, V of DESIGN.md section 20.
//
// One dsm_window_optimize_batch = the staged copy of dsm_window_step_batch (step_launch.hpp) with the loop's state on top, then PASSES
// back to back on the context's stream with no host wait between them.  A pass is the ten launches of dsm_window_step_batch and TWO more:
//   opt_decide_kernel  one 256-lane workgroup per job.  Restores the 2 N doubles into which stp_frame_kernel added the prior (E3 is in
//                      place), so that the next pass finds H_L and b_L as staged.  B1d: the lanes stage 256 residuals' new_energy at a
//                      time in LDS as doubles, lane 0 adds them in ascending index.  B2d: a radix select, four sweeps of eight bits over
//                      256 LDS counters, on the bit patterns of new_energy_with_outlier >= 0 of the residuals against the newest frame
//                      (non-negative floats order like their bit patterns; integer counts have no order to pin); the first sweep rides
//                      on B1d's walk over the heads, which also compacts the keys that count into a list for the other three.  Lane 0 then runs
//                      opt::judge (optimize_math.hpp): the log, the decision, lambda, the heuristic, the phase; writes the next pass's
//                      StpJob::stepfac, SolJob::lambda and frame_energy_th[n - 1]; with a commit the lanes copy the frames' and the
//                      calibration's part.  The job's state is mirrored into the read-back part.
//   opt_commit_kernel  one lane per point and per residual of a job that commits: idepth_backup, idepth_step, state_in, energy_in.
// A finished job is FROZEN: opt_decide_kernel restores H_L / b_L and returns, nothing else of its inputs is written, and every later
// pass recomputes the same bytes.  After the upload the arena's input part is ordinary device memory: the kernels of sections 16-19
// see other values at the same offsets and are unchanged.  No kernel waits for another workgroup; no scratch.
// The call's host side is the pieces of optimize_launch.hpp, which dsm_window_finish_batch (finish_kernels.hip) runs too.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "optimize_launch.hpp"

using namespace dsm;

namespace {

// opt_decide_kernel: the tile of B1d's walk, on which the select's first sweep rides; the later sweeps read the compacted list
// kSweepLoads * kBlock keys a trip.  opt_commit_kernel: lanes per workgroup
constexpr int kBlock = 256, kSweepLoads = 4;
static_assert(8 * DSM_WINDOW_MAX_FRAMES <= kBlock && opt::kMaxN <= kBlock, "one lane per state entry and per row");
static_assert(sizeof(opt::State) % 8 == 0, "the state is mirrored word by word and holds doubles");

struct OptJob {
  opt::Rules R;
  int n, n_pts, n_res, N;
  long long a_stepfac, a_lambda; // bytes from the start of the arena: StpJob::stepfac and SolJob::lambda of the job
  int q_backup, q_step, q_cbackup, q_cstep; // doubles into the step's staged doubles
  int f_idb, f_ids;                         // 4-byte words into the step's staged floats
  long long d_HL, d_bL;                     // doubles into the solve's staged doubles
  long long d_keep;                         // doubles into this call's staged doubles: the diagonal of H_L, then b_L; -1: no prior
  int off_eth, off_ein, off_flags, off_target; // 4-byte words into the linearisation's staged inputs
  // 4-byte words from the start of the arena's device-only part, every one at a multiple of eight bytes
  long long o_head, o_state, o_calib, o_idepth, o_em, o_can, o_x, o_step, o_log;
  long long o_keys; // the select's list, n_res words, in the device-only part
};

struct Median { // the settings of B2
  float thn, fac_median, cw, ow;
};

__device__ __forceinline__ double *dbl(float *base, long long word) { return reinterpret_cast<double *>(base + word); }

__global__ __launch_bounds__(kBlock) void opt_decide_kernel(const OptJob *jobs, opt::State *states, unsigned char *arena, double *sq, double *sd,
                                                            const double *keep, float *stage, float *base, Median T) {
  const OptJob &J = jobs[blockIdx.x];
  opt::State &S = states[blockIdx.x];
  const int tid = threadIdx.x, n = J.n, N = J.N, n_res = J.n_res;
  __shared__ double sE[2][kBlock];
  __shared__ unsigned cnt[kBlock];
  __shared__ unsigned sel[2]; // the select's prefix and the rank left within it
  __shared__ unsigned sKept;
  __shared__ int sCommit;
  const bool frozen = S.phase == opt::DONE;
  if (J.d_keep >= 0 && tid < N) // E3 was applied in place: back to what was staged
    sd[J.d_HL + (long long)tid * N + tid] = keep[J.d_keep + tid], sd[J.d_bL + tid] = keep[J.d_keep + N + tid];
  if (frozen) return; // uniform over the workgroup
  cnt[tid] = 0;
  if (tid == 0) sKept = 0;
  __syncthreads(); // (and every lane has read the phase before lane 0 advances it)

  // ONE walk over the heads.  B1d: the lanes stage a tile of 256 new_energy values as doubles, lane 0 adds them in ascending index;
  // the next tile's loads are in flight and the other buffer is being filled meanwhile, one barrier per tile.  B2d: the keys of the
  // residuals that count go to the job's list (in any order: an order statistic does not see it) and into the first sweep's counters.
  const float4 *head = reinterpret_cast<const float4 *>(base + J.o_head);
  const int *target = reinterpret_cast<const int *>(stage) + J.off_target;
  unsigned *keys = reinterpret_cast<unsigned *>(base + J.o_keys);
  float4 h = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  int tg = -1;
  if (tid < n_res) h = head[tid], tg = target[tid];
  double e = 0.0;
  for (int r0 = 0, tile = 0; r0 < n_res; r0 += kBlock, tile++) {
    const float4 cur = h;
    const int cur_t = tg, r = r0 + tid, next = r + kBlock, m = min(kBlock, n_res - r0);
    if (next < n_res) h = head[next], tg = target[next];
    double *buf = sE[tile & 1];
    if (r < n_res) {
      buf[tid] = (double)cur.y;
      if (cur_t == n - 1 && cur.z >= 0.0f) {
        unsigned key = __float_as_uint(cur.z);
        if (key == 0x80000000u) key = 0; // -0 >= 0 holds and sorts with +0; its square root gives the same threshold
        keys[atomicAdd(&sKept, 1u)] = key;
        atomicAdd(&cnt[key >> 24], 1u);
      }
    }
    __syncthreads();
    if (tid == 0) {
      if (m == kBlock) { // sixteen values ahead in registers: the LDS latency stays off the chain of adds
        double a[16], b[16];
#pragma unroll
        for (int i = 0; i < 16; i++) a[i] = buf[i];
        for (int k = 0; k < kBlock; k += 32) {
#pragma unroll
          for (int i = 0; i < 16; i++) b[i] = buf[k + 16 + i];
#pragma unroll
          for (int i = 0; i < 16; i++) e += a[i];
#pragma unroll
          for (int i = 0; i < 16; i++) a[i] = buf[(k + 32 + i) & (kBlock - 1)]; // (the last trip reads the tile's head again, unused)
#pragma unroll
          for (int i = 0; i < 16; i++) e += b[i];
        }
      } else {
        for (int k = 0; k < m; k++) e += buf[k];
      }
    }
  }
  __syncthreads();

  const unsigned kept = sKept; // uniform; 0: no residual against the newest frame
  unsigned prefix = 0, mask = 0;
  if (tid == 0) sel[1] = (unsigned)(int)(T.thn * (float)kept); // a float32 product, below the count for every thn < 1
  for (int shift = 24; kept && shift >= 0; shift -= 8) { // a radix select: eight bits a sweep, the first sweep's counts are there
    if (shift < 24) {
      cnt[tid] = 0;
      __syncthreads();
      for (unsigned i0 = 0; i0 < kept; i0 += kSweepLoads * kBlock) { // kSweepLoads loads in flight per lane
        unsigned k[kSweepLoads];
        bool in[kSweepLoads];
#pragma unroll
        for (int u = 0; u < kSweepLoads; u++) {
          const unsigned i = i0 + u * kBlock + tid;
          in[u] = i < kept, k[u] = in[u] ? keys[i] : 0u;
        }
#pragma unroll
        for (int u = 0; u < kSweepLoads; u++)
          if (in[u] && (k[u] & mask) == prefix) atomicAdd(&cnt[(k[u] >> shift) & 255u], 1u);
      }
      __syncthreads();
    }
    if (tid == 0) {
      unsigned rem = sel[1];
      int d = 0;
      while (d < 255 && cnt[d] <= rem) rem -= cnt[d], d++;
      sel[0] = prefix | ((unsigned)d << shift), sel[1] = rem;
    }
    __syncthreads();
    prefix = sel[0], mask |= 255u << shift;
  }

  if (tid == 0) {
    const float th = kept ? opt::energy_th(__uint_as_float(prefix), T.fac_median, T.cw, T.ow) : DSM_LINEARIZE_EMPTY_FRAME_ENERGY_TH;
    opt::judge(S, J.R, e, *dbl(base, J.o_em), reinterpret_cast<const int *>(base)[J.o_can], th, dbl(base, J.o_x), N);
    if (S.phase != opt::DONE) { // a finished job keeps its inputs
      stage[J.off_eth + n - 1] = th;
      float *fac = reinterpret_cast<float *>(arena + J.a_stepfac);
      for (int k = 0; k < 5; k++) fac[k] = S.cur_fac;
      *reinterpret_cast<double *>(arena + J.a_lambda) = opt::solve_lambda(S, J.R);
    }
    sCommit = S.commit;
  }
  __syncthreads();
  if (sCommit) { // C, the frames' and the calibration's part
    const double *x = dbl(base, J.o_x);
    if (tid < 8 * n) sq[J.q_backup + tid] = dbl(base, J.o_state)[tid], sq[J.q_step + tid] = -x[4 + tid];
    if (tid < 4) sq[J.q_cbackup + tid] = dbl(base, J.o_calib)[tid], sq[J.q_cstep + tid] = -x[tid];
  }
  const int *from = reinterpret_cast<const int *>(&S);
  int *to = reinterpret_cast<int *>(base + J.o_log);
  for (int i = tid; i < (int)(sizeof(opt::State) / 4); i += kBlock) to[i] = from[i];
}

__global__ __launch_bounds__(kBlock) void opt_commit_kernel(const OptJob *jobs, const opt::State *states, float *sf, float *stage, const float *base) {
  const OptJob &J = jobs[blockIdx.y];
  if (!states[blockIdx.y].commit) return; // uniform over the workgroup
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < J.n_pts) sf[J.f_idb + i] = base[J.o_idepth + i], sf[J.f_ids + i] = base[J.o_step + i];
  if (i < J.n_res) { // applyRes
    const float *head = base + J.o_head + (long long)kLinHeadWords * i;
    int *flags = reinterpret_cast<int *>(stage) + J.off_flags + i;
    stage[J.off_ein + i] = head[1];
    *flags = (*flags & ~0xff) | (__float_as_int(head[0]) & 0xff);
  }
}

} // namespace

extern "C" int dsm_window_optimize_batch(dsm_context *ctx, int n_jobs, const dsm_optimize_job *jobs, const dsm_linearize_params *lp,
                                         const dsm_step_params *sp, const dsm_optimize_params *op) {
  std::vector<const dsm_optimize_job *> list;
  for (int j = 0; jobs && j < n_jobs; j++) list.push_back(jobs + j);
  OptPlan P;
  int rc = optimize_check("dsm_window_optimize_batch", ctx, n_jobs, jobs ? list.data() : nullptr, lp, sp, op, P);
  if (rc) return rc;
  CallArena A;
  optimize_layout(P, A);
  if ((rc = A.bind(ctx))) return rc;
  optimize_stage(P, A, *op);
  if ((rc = A.upload())) return rc;
  // enough when nothing is rejected; a rejected iteration costs one more pass
  if ((rc = optimize_passes(ctx, P, A, *lp, *sp, 1 + P.max_it))) return rc;
  if ((rc = A.fetch(A.out.used))) return rc;
  if (optimize_unfinished(P, A)) {
    if ((rc = optimize_passes(ctx, P, A, *lp, *sp, P.max_it))) return rc;
    if ((rc = A.fetch(A.out.used))) return rc;
  }
  optimize_unpack(P, A, *lp);
  return DSM_OK;
}

namespace dsm {

int optimize_check(const char *call, dsm_context *ctx, int n_jobs, const dsm_optimize_job *const *jobs, const dsm_linearize_params *lp,
                   const dsm_step_params *sp, const dsm_optimize_params *op, OptPlan &P) {
  auto bad = [call](const char *msg) { return invalid((std::string(call) + ": " + msg).c_str()); };
  if (!ctx || n_jobs < 1 || !jobs) return bad("bad argument");
  if (const char *e = optimize_params_error(op)) return bad(e);
  size_t zeros = 4;
  int max_it = 0;
  for (int j = 0; j < n_jobs; j++) {
    if (const char *e = optimize_job_error(*jobs[j])) return bad(e);
    const dsm_linearize_job &L = jobs[j]->step.sol.hes.lin;
    zeros = std::max(zeros, std::max((size_t)8 * L.n_frames, (size_t)L.n_pts / 2 + 1));
    max_it = std::max(max_it, jobs[j]->max_iterations);
  }
  const double lambda0 = op->fixed_lambda >= 0.0 ? op->fixed_lambda : op->lambda_init;
  // the step call's rules and pieces see pass 0: zero steps, zero factors, the first lambda
  P.n_jobs = n_jobs, P.max_it = max_it;
  P.jobs.assign(jobs, jobs + n_jobs);
  P.zero.assign(zeros, 0.0);
  P.first.resize(n_jobs);
  for (int j = 0; j < n_jobs; j++) P.first[j] = optimize_first_pass(*jobs[j], P.zero.data(), lambda0);
  return step_check(call, ctx, n_jobs, P.first.data(), lp, sp, P.stp);
}

// on top of the step call's parts: staged [job table | the jobs' states | doubles: per job with a prior the diagonal of H_L and
// b_L as given], device only [per job: the select's list of keys], read back [per job: its state, mirrored after every pass]
void optimize_layout(OptPlan &P, CallArena &A) {
  const int n_jobs = P.n_jobs;
  step_layout(P.stp, A);
  P.log.assign(n_jobs, 0), P.keys.assign(n_jobs, 0);
  for (int j = 0; j < n_jobs; j++) {
    const dsm_linearize_job &L = P.first[j].sol.hes.lin;
    if (P.first[j].prior) P.doubles += 2 * (4 + 8 * (size_t)L.n_frames);
    P.max_lanes = std::max(P.max_lanes, std::max((size_t)L.n_pts, (size_t)L.n_res));
    P.log[j] = A.out.take(sizeof(opt::State)), P.keys[j] = A.work.take(4 * (size_t)L.n_res);
  }
  P.o_opt = A.in.take(sizeof(OptJob) * n_jobs), P.o_states = A.in.take(sizeof(opt::State) * n_jobs), P.o_keep = A.in.take(8 * P.doubles);
}

void optimize_stage(OptPlan &P, CallArena &A, const dsm_optimize_params &op) {
  const int n_jobs = P.n_jobs;
  const opt::Rules R{op.lambda_accept_fac, op.lambda_reject_fac, op.fixed_lambda, op.min_iterations, op.force_accept != 0, op.step_momentum != 0};
  StpPlan &T = P.stp;
  step_stage(T, A);
  OptJob *hj = A.host_in<OptJob>(P.o_opt);
  opt::State *hs = A.host_in<opt::State>(P.o_states);
  double *hk = A.host_in<double>(P.o_keep);
  const long long out0 = T.sol.hes.out0;
  const LinJob *hl = A.host_in<LinJob>(T.sol.hes.o_lin);
  size_t used = 0;
  for (int j = 0; j < n_jobs; j++) {
    const dsm_step_job &S = P.first[j];
    const dsm_linearize_job &L = S.sol.hes.lin;
    const int n = L.n_frames, N = 4 + 8 * n;
    const StpView &V = T.view[j];
    OptJob &G = hj[j];
    memset(&G, 0, sizeof G);
    G.R = R, G.n = n, G.n_pts = L.n_pts, G.n_res = L.n_res, G.N = N;
    G.a_stepfac = (long long)(T.o_stp + T.stp_stride * j + T.stp_stepfac), G.a_lambda = (long long)(T.sol.o_sol + T.sol.sol_stride * j + T.sol.sol_lambda);
    G.q_backup = V.q_backup, G.q_step = V.q_step, G.q_cbackup = V.q_cbackup, G.q_cstep = V.q_cstep, G.f_idb = V.f_idb, G.f_ids = V.f_ids;
    G.d_HL = T.sol.view[j].d_HL, G.d_bL = T.sol.view[j].d_bL, G.d_keep = -1;
    if (S.prior) {
      G.d_keep = (long long)used;
      for (int i = 0; i < N; i++) hk[used + i] = S.sol.H_L[(size_t)i * N + i], hk[used + N + i] = S.sol.b_L[i];
      used += 2 * (size_t)N;
    }
    G.off_eth = hl[j].off_eth, G.off_ein = hl[j].off_ein, G.off_flags = hl[j].off_flags, G.off_target = hl[j].off_target;
    G.o_head = hl[j].o_head, G.o_state = V.o_state, G.o_calib = V.o_calib, G.o_idepth = V.o_idepth, G.o_em = V.o_em, G.o_can = V.o_can;
    G.o_x = out0 + (long long)(T.sol.at[j].x / 4), G.o_step = out0 + (long long)(T.sol.at[j].step / 4), G.o_log = out0 + (long long)(P.log[j] / 4);
    G.o_keys = (long long)(P.keys[j] / 4);
    opt::state_init(hs[j], op.lambda_init, P.jobs[j]->max_iterations);
  }
}

int optimize_passes(dsm_context *ctx, OptPlan &P, CallArena &A, const dsm_linearize_params &lp, const dsm_step_params &sp, int count) {
  StpPlan &T = P.stp;
  const int n_jobs = P.n_jobs;
  const OptJob *dj = A.dev_in<const OptJob>(P.o_opt);
  opt::State *ds = A.dev_in<opt::State>(P.o_states);
  const Median M{lp.thn, lp.fac_median, lp.cw, lp.ow};
  const int commit_blocks = (int)((P.max_lanes + kBlock - 1) / kBlock);
  for (int k = 0; k < count; k++) {
    if (int e = step_launch(ctx, T, A, lp, sp)) return e;
    hipLaunchKernelGGL(opt_decide_kernel, dim3(n_jobs), dim3(kBlock), 0, ctx->stream, dj, ds, A.dev_in<unsigned char>(0), A.dev_in<double>(T.o_sq),
                       A.dev_in<double>(T.sol.o_sd), A.dev_in<const double>(P.o_keep), A.dev_in<float>(T.sol.hes.o_stage), T.sol.hes.dev_base, M);
    if (commit_blocks)
      hipLaunchKernelGGL(opt_commit_kernel, dim3(commit_blocks, n_jobs), dim3(kBlock), 0, ctx->stream, dj, ds, A.dev_in<float>(T.o_sf),
                         A.dev_in<float>(T.sol.hes.o_stage), T.sol.hes.dev_base);
    DSM_HIP(hipGetLastError());
  }
  return DSM_OK;
}

int optimize_unfinished(const OptPlan &P, const CallArena &A) {
  int open = 0;
  for (int j = 0; j < P.n_jobs; j++) open += A.host_out<opt::State>(P.log[j])->phase != opt::DONE;
  return open;
}

void optimize_unpack(const OptPlan &P, const CallArena &A, const dsm_linearize_params &lp) {
  step_unpack(P.stp, A, lp);
  for (int j = 0; j < P.n_jobs; j++) {
    const dsm_optimize_job &J = *P.jobs[j];
    const opt::State &S = *A.host_out<opt::State>(P.log[j]);
    const size_t its = J.max_iterations, np = 1 + 2 * its;
    *J.n_iterations = S.iteration, *J.n_passes = S.n_passes;
    memcpy(J.pass_energy, S.pass_energy, 16 * np), memcpy(J.pass_lambda, S.pass_lambda, 8 * np);
    if (its) memcpy(J.pattern, S.pattern, its), memcpy(J.iter_stepsize, S.iter_stepsize, 4 * its), memcpy(J.iter_can_break, S.iter_can, its);
    J.last_energy[0] = S.last[0], J.last_energy[1] = S.last[1], *J.lambda_out = S.lambda, *J.frame_energy_th_out = S.eth_out;
  }
}

} // namespace dsm
