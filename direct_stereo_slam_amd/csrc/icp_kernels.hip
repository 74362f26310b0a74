// icp_kernels.hip -- the ICP fallback of loop closure (icp.h:44-71, called at LoopHandler.cpp:284-288 when direct alignment rejects a
// ScanContext match) on the device, batched over independent matches: PCL's IterativeClosestPoint<PointXYZ, PointXYZ> with the
// reference's settings, restated as the quirks P1-P9 / deviations D1-D5 of DESIGN.md section 10.
//
// One call = one launch sequence and one read-back:
//   icp_prep_kernel      (one workgroup per job)  P1: both clouds to float, the guess applied in double; state reset
//   per iteration:
//     icp_nn_kernel      (one workgroup per (job, 256 source points, target slice))  P2: exact brute-force nearest neighbour,
//                        target tiles staged in LDS, per-slice minimum merged by a 64-bit atomic min of the packed key
//                        (float_bits(dist2) << 32 | target index): unsigned order = (distance, smaller index), so the merge order
//                        of the slices does not matter (the ring-key scan's key, ringkey_kernels.hip)
//     icp_step_kernel    (one workgroup per job)  P3-P6: moments of the kept pairs in double (fixed tree order), Umeyama, the
//                        float increment, the convergence tests, final = inc * final, the working cloud moved; keys reset
//   icp_fitness_prep_kernel + icp_nn_kernel + icp_fitness_kernel  P9: the original source moved by `final`, unbounded search, mean
// A job whose state is final leaves every later launch at its first instruction: no host round trip per iteration.
// The sequence is written once (icp_launch): dsm_icp_batch runs it to its end, the test aid dsm_diag_icp_stages stops inside it.
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <string>
#include <vector>

#include "call_arena.hpp"
#include "icp_internal.hpp"

using namespace dsm;

namespace {

constexpr unsigned long long kIcpNoKey = ~0ull; // no candidate yet: its distance bits are a NaN, which never passes a `<=` test

// P5: ((r0 x + r1 y) + r2 z) + t per row, in float (-ffp-contract=off: no fused multiply-add)
__device__ __forceinline__ float4 apply_tf(const float *T, float4 p) {
  float4 o;
  o.x = ((T[0] * p.x + T[1] * p.y) + T[2] * p.z) + T[3];
  o.y = ((T[4] * p.x + T[5] * p.y) + T[6] * p.z) + T[7];
  o.z = ((T[8] * p.x + T[9] * p.y) + T[10] * p.z) + T[11];
  o.w = 0.f;
  return o;
}

// sum of one value per thread over the workgroup, in a fixed tree order (the same on every job and every call)
__device__ __forceinline__ double block_sum(double v, double *red) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
  for (int s = kIcpThreads / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(kIcpThreads) void icp_prep_kernel(const IcpJobDev *__restrict__ jobs, const double *__restrict__ in_src,
                                                               const double *__restrict__ in_tgt, float4 *__restrict__ orig,
                                                               float4 *__restrict__ work, float4 *__restrict__ tgt,
                                                               unsigned long long *__restrict__ keys, IcpState *__restrict__ states) {
  const IcpJobDev &J = jobs[blockIdx.x];
  const int tid = threadIdx.x;
  const double *G = J.guess;
  for (int i = tid; i < J.n_src; i += kIcpThreads) {
    const double *p = in_src + 3 * (J.off_src + i);
    const double x = p[0], y = p[1], z = p[2];
    float4 o; // P1: T [p; 1] in double, rounded to float
    o.x = (float)(((G[0] * x + G[1] * y) + G[2] * z) + G[3]);
    o.y = (float)(((G[4] * x + G[5] * y) + G[6] * z) + G[7]);
    o.z = (float)(((G[8] * x + G[9] * y) + G[10] * z) + G[11]);
    o.w = 0.f;
    orig[J.off_src + i] = o;
    work[J.off_src + i] = o;
    keys[J.off_src + i] = kIcpNoKey;
  }
  for (int i = tid; i < J.n_tgt; i += kIcpThreads) {
    const double *p = in_tgt + 3 * (J.off_tgt + i);
    tgt[J.off_tgt + i] = make_float4((float)p[0], (float)p[1], (float)p[2], 0.f);
  }
  if (tid < 16) states[blockIdx.x].final_tf[tid] = (tid % 5 == 0) ? 1.f : 0.f;
  if (tid < kIcpIterationsLimit) states[blockIdx.x].corr[tid] = -1;
  if (tid == 0) {
    IcpState &S = states[blockIdx.x];
    S.prev_mse = DBL_MAX;
    S.fitness = INFINITY;
    S.state = (J.n_src == 0 || J.n_tgt == 0) ? kIcpEmpty : kIcpRunning; // D3
    S.iterations = 0;
    S.searches = 0;
    S.pad = 0;
  }
}

// P2 / P9: for each source point of the block, the nearest target of the slice by ((dx dx) + dy dy) + dz dz in float, d = source -
// target; strict `<` over ascending target indices keeps the smallest index of a tie, the atomic min the smallest across slices.
// fitness: the pass of getFitnessScore (every non-empty job) instead of an iteration's (running jobs only).
__global__ __launch_bounds__(kIcpThreads) void icp_nn_kernel(const IcpNnBlock *__restrict__ blocks, const IcpJobDev *__restrict__ jobs,
                                                             const IcpState *__restrict__ states, const float4 *__restrict__ work,
                                                             const float4 *__restrict__ tgt, unsigned long long *__restrict__ keys,
                                                             int fitness) {
  __shared__ float4 tile[kIcpTile];
  const IcpNnBlock B = blocks[blockIdx.x];
  const int st = states[B.job].state;
  if (fitness ? st == kIcpEmpty : st != kIcpRunning) return;
  const IcpJobDev &J = jobs[B.job];
  const int i = B.src0 + threadIdx.x;
  const bool has = i < J.n_src;
  const float4 p = has ? work[J.off_src + i] : make_float4(0.f, 0.f, 0.f, 0.f);
  float best = INFINITY;
  int bi = -1;
  for (int t0 = B.tgt0; t0 < B.tgt1; t0 += kIcpTile) {
    const int m = min(kIcpTile, B.tgt1 - t0);
    __syncthreads();
    if ((int)threadIdx.x < m) tile[threadIdx.x] = tgt[J.off_tgt + t0 + threadIdx.x];
    __syncthreads();
    for (int k = 0; k < m; k++) {
      const float4 q = tile[k];
      const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
      const float d = (dx * dx + dy * dy) + dz * dz;
      if (d < best) best = d, bi = t0 + k;
    }
  }
  if (has && bi >= 0) atomicMin(&keys[J.off_src + i], ((unsigned long long)__float_as_uint(best) << 32) | (unsigned)bi);
}

// P3-P6 for one job: one workgroup
__global__ __launch_bounds__(kIcpThreads) void icp_step_kernel(const IcpJobDev *__restrict__ jobs, IcpState *__restrict__ states,
                                                               float4 *__restrict__ work, const float4 *__restrict__ tgt,
                                                               unsigned long long *__restrict__ keys, int max_iterations, double eps,
                                                               double max_dist2) {
  __shared__ double red[kIcpThreads];
  __shared__ float inc_s[16];
  IcpState &S = states[blockIdx.x];
  if (S.state != kIcpRunning) return;
  const IcpJobDev &J = jobs[blockIdx.x];
  const int tid = threadIdx.x;
  const float4 *W = work + J.off_src, *T = tgt + J.off_tgt;
  unsigned long long *K = keys + J.off_src;
  // pass 1: count, the two sums and the sum of the pairs' distances (P2's test: dist2 <= max_dist^2, in double)
  int cnt = 0;
  double ss[3] = {0, 0, 0}, ts[3] = {0, 0, 0}, ds = 0;
  for (int i = tid; i < J.n_src; i += kIcpThreads) {
    const unsigned long long k = K[i];
    const float d = __uint_as_float((unsigned)(k >> 32));
    if (!((double)d <= max_dist2)) continue;
    const float4 a = W[i], b = T[(unsigned)k];
    cnt++;
    ss[0] += a.x, ss[1] += a.y, ss[2] += a.z;
    ts[0] += b.x, ts[1] += b.y, ts[2] += b.z;
    ds += d;
  }
  const int n = (int)block_sum((double)cnt, red);
  if (tid == 0) S.corr[S.searches] = n;
  if (n < 3) { // P3: the loop ends, final stays as it is; the keys are reset by the fitness pass
    if (tid == 0) S.searches++, S.state = kIcpNoCorrespondences;
    return;
  }
  const double one_over_n = 1.0 / (double)n;
  double sm[3], tm[3];
  for (int c = 0; c < 3; c++) sm[c] = block_sum(ss[c], red) * one_over_n;
  for (int c = 0; c < 3; c++) tm[c] = block_sum(ts[c], red) * one_over_n;
  const double mse = block_sum(ds, red) / (double)n;
  // pass 2: Sigma = (1/n) sum (dst - dst_mean)(src - src_mean)^T (D1: double, fixed order)
  double sg[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = tid; i < J.n_src; i += kIcpThreads) {
    const unsigned long long k = K[i];
    const float d = __uint_as_float((unsigned)(k >> 32));
    if (!((double)d <= max_dist2)) continue;
    const float4 a = W[i], b = T[(unsigned)k];
    const double sc[3] = {a.x - sm[0], a.y - sm[1], a.z - sm[2]}, dc[3] = {b.x - tm[0], b.y - tm[1], b.z - tm[2]};
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) sg[r * 3 + c] += dc[r] * sc[c];
  }
  double Sigma[9];
  for (int e = 0; e < 9; e++) Sigma[e] = block_sum(sg[e], red) * one_over_n;
  if (tid == 0) {
    double R[9], t[3];
    icp_umeyama(Sigma, sm, tm, R, t);
    float inc[16]; // P4: the Matrix4f PCL holds
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++) inc[r * 4 + c] = (float)R[r * 3 + c];
      inc[r * 4 + 3] = (float)t[r];
    }
    inc[12] = inc[13] = inc[14] = 0.f, inc[15] = 1.f;
    // P5: final = inc * final, float, k = 0 .. 3 left to right
    float F[16];
    for (int r = 0; r < 4; r++)
      for (int c = 0; c < 4; c++)
        F[r * 4 + c] = ((inc[r * 4] * S.final_tf[c] + inc[r * 4 + 1] * S.final_tf[4 + c]) + inc[r * 4 + 2] * S.final_tf[8 + c]) +
                       inc[r * 4 + 3] * S.final_tf[12 + c];
    for (int e = 0; e < 16; e++) S.final_tf[e] = F[e], inc_s[e] = inc[e];
    const int it = ++S.iterations;
    S.searches++;
    // P6, in PCL's order
    const double cos_angle = 0.5 * (double)(((inc[0] + inc[5]) + inc[10]) - 1.f);
    const float tr2 = (inc[3] * inc[3] + inc[7] * inc[7]) + inc[11] * inc[11];
    if (it >= max_iterations)
      S.state = kIcpIterations;
    else if (cos_angle >= 1.0 - eps && (double)tr2 <= eps)
      S.state = kIcpTransform;
    else if (fabs(mse - S.prev_mse) < 1e-12)
      S.state = kIcpAbsMse;
    else
      S.prev_mse = mse;
  }
  __syncthreads();
  // P5: the working cloud moves by the increment (also on the last iteration, as PCL's transformCloud runs before the tests)
  float inc[16];
  for (int e = 0; e < 16; e++) inc[e] = inc_s[e];
  for (int i = tid; i < J.n_src; i += kIcpThreads) {
    work[J.off_src + i] = apply_tf(inc, W[i]);
    K[i] = kIcpNoKey;
  }
}

// P9, first half: the ORIGINAL (guess-transformed) source moved by final, into the working cloud; keys reset
__global__ __launch_bounds__(kIcpThreads) void icp_fitness_prep_kernel(const IcpJobDev *__restrict__ jobs, const IcpState *__restrict__ states,
                                                                       const float4 *__restrict__ orig, float4 *__restrict__ work,
                                                                       unsigned long long *__restrict__ keys) {
  const IcpState &S = states[blockIdx.x];
  if (S.state == kIcpEmpty) return;
  const IcpJobDev &J = jobs[blockIdx.x];
  float F[16];
  for (int e = 0; e < 16; e++) F[e] = S.final_tf[e];
  for (int i = threadIdx.x; i < J.n_src; i += kIcpThreads) {
    work[J.off_src + i] = apply_tf(F, orig[J.off_src + i]);
    keys[J.off_src + i] = kIcpNoKey;
  }
}

// P9, second half: mean of the nearest-neighbour distances of every source point (no distance limit); D4: fixed tree order
__global__ __launch_bounds__(kIcpThreads) void icp_fitness_kernel(const IcpJobDev *__restrict__ jobs, IcpState *__restrict__ states,
                                                                  const unsigned long long *__restrict__ keys) {
  __shared__ double red[kIcpThreads];
  IcpState &S = states[blockIdx.x];
  if (S.state == kIcpEmpty) return;
  const IcpJobDev &J = jobs[blockIdx.x];
  double ds = 0;
  for (int i = threadIdx.x; i < J.n_src; i += kIcpThreads) ds += (double)__uint_as_float((unsigned)(keys[J.off_src + i] >> 32));
  const double sum = block_sum(ds, red);
  if (threadIdx.x == 0) S.fitness = sum / (double)J.n_src;
}

bool finite16(const double *m) {
  for (int e = 0; e < 16; e++)
    if (!std::isfinite(m[e])) return false;
  return true;
}

// what one launch sequence leaves bound in the context's arena: the device-only clouds and keys, and the states (read back by fetch)
struct IcpRun {
  CallArena A;
  long long tot_src = 0, tot_tgt = 0;
  float4 *orig = nullptr, *work = nullptr, *tgt = nullptr;
  unsigned long long *keys = nullptr;
  size_t o_states = 0;
};

// all-or-nothing validation of a call (`who`: "dsm_icp_batch: " ...); outputs: the job's result pointers are required
int icp_validate(const char *who, dsm_context *ctx, int n_jobs, const dsm_icp_job *jobs, int max_iterations, double transformation_epsilon,
                 double max_corr_dist, bool outputs) {
  const std::string w(who);
  if (!ctx || n_jobs < 1 || !jobs || max_iterations < 1 || max_iterations > kIcpIterationsLimit || !std::isfinite(transformation_epsilon) ||
      !std::isfinite(max_corr_dist) || max_corr_dist < 0)
    return invalid((w + "bad argument").c_str());
  for (int j = 0; j < n_jobs; j++) {
    const dsm_icp_job &J = jobs[j];
    if (J.n_src < 0 || J.n_tgt < 0 || J.n_src > DSM_ICP_MAX_POINTS || J.n_tgt > DSM_ICP_MAX_POINTS || (J.n_src && !J.src_xyz) ||
        (J.n_tgt && !J.tgt_xyz) || !J.tfm_target_source || (outputs && (!J.score || !J.ok || !J.iterations || !J.state)))
      return invalid((w + "bad job").c_str());
    if (!finite16(J.tfm_target_source)) return invalid((w + "non-finite guess").c_str());
  }
  return DSM_OK;
}

// The launch sequence of one call, from the block table to the last kernel of `stop_stage` (DSM_ICP_STAGE_*; the searches and steps of
// the iterations are told apart by `stop_iteration`, 0-based).  dsm_icp_batch runs it to its end under the production slice rule
// (force_slices = 0); dsm_diag_icp_stages stops inside it and may force the number of target slices a job is cut into.  Nothing is
// read back here: the caller fetches the states, or copies the device buffers of `run` out, on the context's stream.
int icp_launch(dsm_context *ctx, int n_jobs, const dsm_icp_job *jobs, int max_iterations, double transformation_epsilon, double max_corr_dist,
               int force_slices, int stop_stage, int stop_iteration, IcpRun &run) {
  long long tot_src = 0, tot_tgt = 0;
  for (int j = 0; j < n_jobs; j++) tot_src += jobs[j].n_src, tot_tgt += jobs[j].n_tgt;
  run.tot_src = tot_src, run.tot_tgt = tot_tgt;
  // the call's blocks of the search: as many target slices per job as bring the call to about 2048 workgroups, at least one tile each
  std::vector<IcpJobDev> hj(n_jobs);
  std::vector<IcpNnBlock> blocks;
  long long src_blocks = 0;
  for (int j = 0; j < n_jobs; j++)
    if (jobs[j].n_src && jobs[j].n_tgt) src_blocks += (jobs[j].n_src + kIcpThreads - 1) / kIcpThreads;
  const long long want_slices = force_slices > 0 ? force_slices : src_blocks ? (2048 + src_blocks - 1) / src_blocks : 1;
  long long os = 0, ot = 0;
  for (int j = 0; j < n_jobs; j++) {
    const dsm_icp_job &J = jobs[j];
    IcpJobDev &D = hj[j];
    D.n_src = J.n_src, D.n_tgt = J.n_tgt, D.off_src = os, D.off_tgt = ot;
    memcpy(D.guess, J.tfm_target_source, sizeof D.guess);
    os += J.n_src, ot += J.n_tgt;
    if (!J.n_src || !J.n_tgt) continue;
    const int slices = (int)std::min<long long>(want_slices, (J.n_tgt + kIcpTile - 1) / kIcpTile);
    const int per = (J.n_tgt + slices - 1) / slices;
    for (int s0 = 0; s0 < J.n_src; s0 += kIcpThreads)
      for (int t0 = 0; t0 < J.n_tgt; t0 += per) blocks.push_back(IcpNnBlock{j, s0, t0, std::min(J.n_tgt, t0 + per)});
  }
  // staged [jobs | blocks | source xyz | target xyz], device-only [orig | work | target | keys], read back [states]
  CallArena &A = run.A;
  const size_t o_jobs = A.in.take(sizeof(IcpJobDev) * n_jobs), o_blocks = A.in.take(sizeof(IcpNnBlock) * std::max<size_t>(1, blocks.size()));
  const size_t o_src = A.in.take(sizeof(double) * 3 * (size_t)tot_src), o_tgt = A.in.take(sizeof(double) * 3 * (size_t)tot_tgt);
  const size_t b_f4s = sizeof(float4) * (size_t)std::max(1ll, tot_src), b_f4t = sizeof(float4) * (size_t)std::max(1ll, tot_tgt);
  const size_t o_orig = A.work.take(b_f4s), o_work = A.work.take(b_f4s), o_tgt4 = A.work.take(b_f4t);
  const size_t o_keys = A.work.take(sizeof(unsigned long long) * (size_t)std::max(1ll, tot_src)), o_states = A.out.take(sizeof(IcpState) * n_jobs);
  int rc = A.bind(ctx);
  if (rc) return rc;
  memcpy(A.host_in<IcpJobDev>(o_jobs), hj.data(), sizeof(IcpJobDev) * n_jobs);
  if (!blocks.empty()) memcpy(A.host_in<IcpNnBlock>(o_blocks), blocks.data(), sizeof(IcpNnBlock) * blocks.size());
  for (int j = 0; j < n_jobs; j++) {
    if (jobs[j].n_src) memcpy(A.host_in<double>(o_src) + 3 * hj[j].off_src, jobs[j].src_xyz, sizeof(double) * 3 * jobs[j].n_src);
    if (jobs[j].n_tgt) memcpy(A.host_in<double>(o_tgt) + 3 * hj[j].off_tgt, jobs[j].tgt_xyz, sizeof(double) * 3 * jobs[j].n_tgt);
  }
  const IcpJobDev *dj = A.dev_in<const IcpJobDev>(o_jobs);
  const IcpNnBlock *db = A.dev_in<const IcpNnBlock>(o_blocks);
  const double *d_src = A.dev_in<const double>(o_src), *d_tgt = A.dev_in<const double>(o_tgt);
  float4 *orig = A.dev_work<float4>(o_orig), *work = A.dev_work<float4>(o_work), *tgt = A.dev_work<float4>(o_tgt4);
  unsigned long long *keys = A.dev_work<unsigned long long>(o_keys);
  IcpState *d_states = A.dev_out<IcpState>(o_states);
  run.orig = orig, run.work = work, run.tgt = tgt, run.keys = keys, run.o_states = o_states;
  hipStream_t st = ctx->stream;
  if ((rc = A.upload())) return rc;
  const int nb = (int)blocks.size();
  const double max_dist2 = max_corr_dist * max_corr_dist;
  const auto stops = [&](int stage, int it) { return stop_stage == stage && (it < 0 || it == stop_iteration); };
  hipLaunchKernelGGL(icp_prep_kernel, dim3(n_jobs), dim3(kIcpThreads), 0, st, dj, d_src, d_tgt, orig, work, tgt, keys, d_states);
  bool stopped = stops(DSM_ICP_STAGE_PREP, -1);
  for (int it = 0; it < max_iterations && nb && !stopped; it++) {
    hipLaunchKernelGGL(icp_nn_kernel, dim3(nb), dim3(kIcpThreads), 0, st, db, dj, (const IcpState *)d_states, (const float4 *)work,
                       (const float4 *)tgt, keys, 0);
    if ((stopped = stops(DSM_ICP_STAGE_SEARCH, it))) break;
    hipLaunchKernelGGL(icp_step_kernel, dim3(n_jobs), dim3(kIcpThreads), 0, st, dj, d_states, work, (const float4 *)tgt, keys,
                       max_iterations, transformation_epsilon, max_dist2);
    stopped = stops(DSM_ICP_STAGE_STEP, it);
  }
  if (nb && !stopped) {
    hipLaunchKernelGGL(icp_fitness_prep_kernel, dim3(n_jobs), dim3(kIcpThreads), 0, st, dj, (const IcpState *)d_states, (const float4 *)orig,
                       work, keys);
    stopped = stops(DSM_ICP_STAGE_FITNESS_PREP, -1);
  }
  if (nb && !stopped) {
    hipLaunchKernelGGL(icp_nn_kernel, dim3(nb), dim3(kIcpThreads), 0, st, db, dj, (const IcpState *)d_states, (const float4 *)work,
                       (const float4 *)tgt, keys, 1);
    stopped = stops(DSM_ICP_STAGE_FITNESS_SEARCH, -1);
  }
  if (nb && !stopped)
    hipLaunchKernelGGL(icp_fitness_kernel, dim3(n_jobs), dim3(kIcpThreads), 0, st, dj, d_states, (const unsigned long long *)keys);
  DSM_HIP(hipGetLastError());
  return DSM_OK;
}

// the public mirror of the per-job state is the state itself
static_assert(sizeof(dsm_icp_state) == sizeof(IcpState) && offsetof(dsm_icp_state, prev_mse) == offsetof(IcpState, prev_mse) &&
                  offsetof(dsm_icp_state, fitness) == offsetof(IcpState, fitness) && offsetof(dsm_icp_state, state) == offsetof(IcpState, state) &&
                  offsetof(dsm_icp_state, searches) == offsetof(IcpState, searches) && offsetof(dsm_icp_state, corr) == offsetof(IcpState, corr),
              "dsm_icp_state (include/dsm_hotpath.h) mirrors IcpState");

} // namespace

extern "C" {

// replaces icp() (src/loop_closure/pose_estimation/icp.h:44-71) for a batch of independent matches
int dsm_icp_batch(dsm_context *ctx, int n_jobs, dsm_icp_job *jobs, int max_iterations, double transformation_epsilon, double max_corr_dist,
                  double score_thres) {
  if (std::isnan(score_thres)) return invalid("dsm_icp_batch: bad argument");
  int rc = icp_validate("dsm_icp_batch: ", ctx, n_jobs, jobs, max_iterations, transformation_epsilon, max_corr_dist, true);
  if (rc) return rc;
  IcpRun run;
  if ((rc = icp_launch(ctx, n_jobs, jobs, max_iterations, transformation_epsilon, max_corr_dist, 0, DSM_ICP_STAGE_FITNESS, 0, run))) return rc;
  if ((rc = run.A.fetch(sizeof(IcpState) * n_jobs))) return rc;
  const IcpState *h_states = run.A.host_out<IcpState>(run.o_states);
  for (int j = 0; j < n_jobs; j++) {
    dsm_icp_job &J = jobs[j];
    const IcpState &S = h_states[j];
    if (J.corr_counts)
      for (int k = 0; k < max_iterations; k++) J.corr_counts[k] = S.state == kIcpEmpty ? -1 : S.corr[k];
    *J.iterations = S.state == kIcpEmpty ? 0 : S.iterations;
    *J.state = S.state;
    if (S.state == kIcpEmpty) { // D3
      *J.score = INFINITY;
      *J.ok = 0;
      continue;
    }
    // P8: tfm_target_source = double(final) * tfm_target_source, k = 0 .. 3 left to right
    double G[16], F[16];
    memcpy(G, J.tfm_target_source, sizeof G);
    for (int e = 0; e < 16; e++) F[e] = (double)S.final_tf[e];
    for (int r = 0; r < 4; r++)
      for (int c = 0; c < 4; c++)
        J.tfm_target_source[r * 4 + c] = ((F[r * 4] * G[c] + F[r * 4 + 1] * G[4 + c]) + F[r * 4 + 2] * G[8 + c]) + F[r * 4 + 3] * G[12 + c];
    *J.score = (float)S.fitness; // P9
    *J.ok = (double)*J.score < score_thres ? 1 : 0;
  }
  return DSM_OK;
}


// test aid: the same launch sequence stopped after a stage, the device's buffers copied out (include/dsm_hotpath.h)
int dsm_diag_icp_stages(dsm_context *ctx, int n_jobs, const dsm_icp_job *jobs, int max_iterations, double transformation_epsilon,
                        double max_corr_dist, int want_slices, int stop_stage, int stop_iteration, float *orig_xyzw, float *work_xyzw,
                        float *target_xyzw, unsigned long long *keys, dsm_icp_state *states) {
  int rc = icp_validate("dsm_diag_icp_stages: ", ctx, n_jobs, jobs, max_iterations, transformation_epsilon, max_corr_dist, false);
  if (rc) return rc;
  const bool per_iteration = stop_stage == DSM_ICP_STAGE_SEARCH || stop_stage == DSM_ICP_STAGE_STEP;
  if (want_slices < 0 || stop_stage < DSM_ICP_STAGE_PREP || stop_stage > DSM_ICP_STAGE_FITNESS ||
      (per_iteration && (stop_iteration < 0 || stop_iteration >= max_iterations)))
    return invalid("dsm_diag_icp_stages: bad want_slices, stage or iteration");
  IcpRun run;
  if ((rc = icp_launch(ctx, n_jobs, jobs, max_iterations, transformation_epsilon, max_corr_dist, want_slices, stop_stage, stop_iteration, run)))
    return rc;
  hipStream_t st = ctx->stream;
  const size_t b_src = sizeof(float4) * (size_t)run.tot_src, b_tgt = sizeof(float4) * (size_t)run.tot_tgt;
  if (orig_xyzw && b_src) DSM_HIP(hipMemcpyAsync(orig_xyzw, run.orig, b_src, hipMemcpyDeviceToHost, st));
  if (work_xyzw && b_src) DSM_HIP(hipMemcpyAsync(work_xyzw, run.work, b_src, hipMemcpyDeviceToHost, st));
  if (target_xyzw && b_tgt) DSM_HIP(hipMemcpyAsync(target_xyzw, run.tgt, b_tgt, hipMemcpyDeviceToHost, st));
  if (keys && run.tot_src) DSM_HIP(hipMemcpyAsync(keys, run.keys, sizeof(unsigned long long) * (size_t)run.tot_src, hipMemcpyDeviceToHost, st));
  if ((rc = run.A.fetch(sizeof(IcpState) * n_jobs))) return rc; // drains the stream: the copies above have landed
  if (states) memcpy(states, run.A.host_out<IcpState>(run.o_states), sizeof(IcpState) * n_jobs);
  return DSM_OK;
}

} // extern "C"
