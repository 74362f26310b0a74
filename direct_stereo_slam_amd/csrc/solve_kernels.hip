// solve_kernels.hip -- the rest of EnergyFunctional::solveSystemF and resubstituteF_MT of FrontEnd::optimize
// (dso_helpers/FrontEndOptimize.cpp:332-486) on the device, for the windows of many sequences in one call.  Semantics: T1d, F1-F8,
// R1-R3, V of DESIGN.md section 18.
//
// One dsm_window_solve_batch = one staged copy, the FIVE launches of dsm_window_hessian_batch (hessian_launch.hpp), THREE more on the
// same stream and arena, one read-back (as pieces in solve_launch.hpp, which dsm_window_step_batch runs too):
//   sol_stitch_kernel  one 64-lane workgroup per (job, 8 x 8 block of the upper block triangle), one per (job, frame) for the C rows
//                      and the right-hand sides of the frame's block, one per job for the 4 x 4 corner (T1d).  Lane (a, b) holds the
//                      block's entry and walks the contributing pairs in T1's order; the Mh / Mt intermediate of a product goes
//                      through LDS.  Every entry of the upper half is written once, with its mirror: no matrix is cleared first.
//   sol_solve_kernel   one workgroup per job.  F1-F5 element-parallel; the pivot order from the scaled diagonal alone (ranks; ties and
//                      NaNs take the literal selection loop in one lane); the permuted lower triangle in LDS, column-major, ONE ROW PER
//                      LANE: at step k the d_j A[k][j] products are formed once and broadcast through LDS, every lane forms the dot
//                      product over its own row, the column is divided by the pivot with one division per lane and step.  Then the
//                      substitutions (the back substitution's products in parallel, its chain in the row's lane), F7 and bit 0 of R3.
//   sol_step_kernel    one lane per point: every workgroup forms xAd of all pairs in LDS (R1, one lane per (pair, c)), then R2 over the
//                      point's residual list in ascending residual index, and bit 1 of R3.
// Every result is ONE sequential chain in one lane, in the stated order: it does not depend on the launch geometry or on the other
// jobs of the call.  No kernel waits for another workgroup; barriers are workgroup-local.  No MFMA, no scratch.
#include <algorithm>
#include <cstddef>
#include <cstring>
#include <string>
#include <vector>

#include "solve_launch.hpp"

#include "solve_math.hpp"

using namespace dsm;

namespace {

constexpr int kSolveBlock = 256; // sol_solve_kernel: rows in the first N lanes, every lane fills
constexpr int kStepBlock = 256;  // sol_step_kernel: points per workgroup

struct SolJob {
  HesView V;
  int N, n_null;
  double lambda;
  // doubles into the staged doubles; the optional ones -1 for zeros
  long long d_adh, d_adt, d_HL, d_bL, d_HM, d_bM, d_dx, d_basis, d_pinv;
  // 4-byte words from the start of the arena's device-only part, every one at a multiple of eight bytes; o_lastH, o_lastb -1: not asked for
  long long o_HA, o_bA, o_HS, o_bS, o_x, o_step, o_flags, o_lastH, o_lastb;
};

__device__ __forceinline__ double *dbl(float *base, long long word) { return reinterpret_cast<double *>(base + word); }
__device__ __forceinline__ void put_sym(double *H, int N, int i, int j, double v) { H[(long long)i * N + j] = v, H[(long long)j * N + i] = v; }

__global__ __launch_bounds__(64) void sol_stitch_kernel(const SolJob *jobs, const double *sd, float *base) {
  const SolJob &J = jobs[blockIdx.y];
  const int nf = J.V.n_frames, N = J.N, tid = threadIdx.x, a = tid >> 3, b = tid & 7;
  const int nb = nf * (nf + 1) / 2, blk = blockIdx.x;
  if (blk > nb + nf) return; // uniform over the workgroup
  __shared__ double M[64];
  const double *top = dbl(base, J.V.o_top), *D = dbl(base, J.V.o_D), *E = dbl(base, J.V.o_E), *EB = dbl(base, J.V.o_EB);
  const double *adh = sd + J.d_adh, *adt = sd + J.d_adt;
  double *HA = dbl(base, J.o_HA), *bA = dbl(base, J.o_bA), *HS = dbl(base, J.o_HS), *bS = dbl(base, J.o_bS);
  if (blk < nb) { // block (I, K), I <= K, of the frames' part
    int I = 0, r = blk;
    while (r >= nf - I) r -= nf - I, I++;
    const int K = I + r, row = 4 + 8 * I + a, col = 4 + 8 * K + b;
    const bool mine = I < K || a <= b;
    double acc = 0.0;
    for (int h = 0; h < nf; h++) // H_A: the pairs in (h, t) order
      for (int t = 0; t < nf; t++) {
        if (t == h || !((I == h || I == t) && (K == h || K == t))) continue;
        const long long pr = h * nf + t;
        const double *left = (I == h ? adh : adt) + pr * 64, *right = (K == h ? adh : adt) + pr * 64;
        __syncthreads(); // the product before has read M
        M[tid] = sol::dot8(left + 8 * a, 1, top + pr * 169 + 4 * 13 + 4 + b, 13);
        __syncthreads();
        acc += sol::dot8(M + 8 * a, 1, right + 8 * b, 1);
      }
    if (mine) put_sym(HA, N, row, col, acc);
    acc = 0.0;
    for (int h = 0; h < nf; h++) // H_sc: (h, t1, t2) order
      for (int t1 = 0; t1 < nf; t1++) {
        if (t1 == h || !(I == h || I == t1)) continue;
        for (int t2 = 0; t2 < nf; t2++) {
          if (t2 == h || !(K == h || K == t2)) continue;
          const long long p1 = h * nf + t1, p2 = h * nf + t2;
          const double *left = (I == h ? adh : adt) + p1 * 64, *right = (K == h ? adh : adt) + p2 * 64;
          __syncthreads();
          M[tid] = sol::dot8(left + 8 * a, 1, D + (p1 * nf + t2) * 64 + b, 8);
          __syncthreads();
          acc += sol::dot8(M + 8 * a, 1, right + 8 * b, 1);
        }
      }
    if (mine) put_sym(HS, N, row, col, acc);
    return;
  }
  if (blk < nb + nf) { // the C rows over frame f's columns (lanes 0-31: row a < 4, column b) and the frame's right-hand sides (32-39)
    const int f = blk - nb;
    if (tid >= 40) return;
    const bool rhs = tid >= 32;
    double acc = 0.0, acc_s = 0.0;
    for (int h = 0; h < nf; h++)
      for (int t = 0; t < nf; t++) {
        if (t == h || (h != f && t != f)) continue;
        const long long pr = h * nf + t;
        const double *ad = (h == f ? adh : adt) + pr * 64, *A = top + pr * 169;
        if (rhs) {
          acc += sol::dot8(ad + 8 * b, 1, A + 4 * 13 + 12, 13);
          acc_s += sol::dot8(ad + 8 * b, 1, EB + pr * 8, 1);
        } else {
          acc += sol::dot8(A + a * 13 + 4, 1, ad + 8 * b, 1);
          acc_s += sol::dot8(ad + 8 * b, 1, E + pr * 32 + a, 4);
        }
      }
    if (rhs) bA[4 + 8 * f + b] = acc, bS[4 + 8 * f + b] = acc_s;
    else put_sym(HA, N, a, 4 + 8 * f + b, acc), put_sym(HS, N, a, 4 + 8 * f + b, acc_s);
    return;
  }
  if (tid < 16) { // the corner
    const int c = tid >> 2, d = tid & 3;
    double acc = 0.0;
    for (int h = 0; h < nf; h++)
      for (int t = 0; t < nf; t++)
        if (t != h) acc += top[(long long)(h * nf + t) * 169 + c * 13 + d];
    if (c <= d) put_sym(HA, N, c, d, acc), put_sym(HS, N, c, d, dbl(base, J.V.o_Hcc)[4 * c + d]);
  } else if (tid < 20) {
    const int c = tid - 16;
    double acc = 0.0;
    for (int h = 0; h < nf; h++)
      for (int t = 0; t < nf; t++)
        if (t != h) acc += top[(long long)(h * nf + t) * 169 + c * 13 + 12];
    bA[c] = acc, bS[c] = dbl(base, J.V.o_bc)[c];
  }
}

__device__ __forceinline__ bool not_finite(double x) { return !(fabs(x) <= 1.7976931348623157e308); }

__global__ __launch_bounds__(kSolveBlock) void sol_solve_kernel(const SolJob *jobs, const double *sd, float *base) {
  extern __shared__ double lds[];
  const SolJob &J = jobs[blockIdx.x];
  const int N = J.N, tid = threadIdx.x, nt = blockDim.x;
  // Lm: the permuted lower triangle, entry (i, j) at j N + i, so that the lanes of a step read consecutive words
  double *Lm = lds, *v = Lm + N * N, *bF = v + N, *dg = bF + N, *tmp = dg + N, *yv = tmp + N, *av = yv + N, *xs = av + N;
  int *perm = reinterpret_cast<int *>(xs + N), *odd = perm + N, *bad = odd + 1;
  const double *HL = sd + J.d_HL, *bL = sd + J.d_bL, *HM = J.d_HM >= 0 ? sd + J.d_HM : nullptr, *bM = J.d_bM >= 0 ? sd + J.d_bM : nullptr;
  const double *dx = J.d_dx >= 0 ? sd + J.d_dx : nullptr;
  const double *HA = dbl(base, J.o_HA), *bA = dbl(base, J.o_bA), *HS = dbl(base, J.o_HS), *bS = dbl(base, J.o_bS);
  const double lam1 = 1.0 + J.lambda, s = 1.0 / lam1;
  const bool row = tid < N;
  auto undamped = [&](int i, int j) { // F2
    const long long e = (long long)i * N + j;
    return sol::hf_entry(HL[e], HM ? HM[e] : 0.0, HA[e]);
  };
  auto entry = [&](int i, int j) { return sol::damped(undamped(i, j), HS[(long long)i * N + j], i == j, lam1, s); }; // F4
  if (row) { // F1, F2 for b, F5's scale, the scaled diagonal
    const double d = entry(tid, tid), vi = sol::scale_of(d);
    v[tid] = vi, av[tid] = fabs(sol::scaled(vi, d, vi));
    const double b = sol::bf_entry(bL[tid], sol::prior_top(HM ? HM + (long long)tid * N : nullptr, bM, dx, tid, N), bA[tid], bS[tid]);
    bF[tid] = b;
    if (J.o_lastb >= 0) dbl(base, J.o_lastb)[tid] = b; // F3
  }
  if (tid == 0) *odd = 0, *bad = 0;
  if (J.o_lastH >= 0)
    for (int e = tid; e < N * N; e += nt) dbl(base, J.o_lastH)[e] = undamped(e / N, e % N) - HS[e];
  __syncthreads();
  if (row) { // F6: the pivot order, from the diagonal alone
    const double mine = av[tid];
    int rank = 0;
    bool tie = mine != mine;
    for (int j = 0; j < N; j++) {
      const double o = av[j];
      rank += o > mine;
      tie = tie || (j != tid && o == mine);
    }
    if (tie) *odd = 1;
    else perm[rank] = tid;
  }
  __syncthreads();
  if (*odd) { // uniform: exact ties or a NaN, where the swaps of the selection loop decide
    if (tid == 0) sol::pivot_order(av, perm, N);
    __syncthreads();
  }
  for (int e = tid; e < N * N; e += nt) { // F5 on the permuted lower triangle, read from the lower triangle of the system
    const int j = e / N, i = e - j * N;
    if (i < j) continue;
    const int pi = perm[i], pj = perm[j], hi = pi > pj ? pi : pj, lo = pi > pj ? pj : pi;
    Lm[e] = sol::scaled(v[hi], entry(hi, lo), v[lo]);
  }
  double y = row ? v[perm[tid]] * bF[perm[tid]] : 0.0;
  __syncthreads();
  bool all_zero = false;
  for (int k = 0; k < N; k++) { // left-looking; no pivoting left to do
    if (k > 0) {
      if (tid < k) tmp[tid] = dg[tid] * Lm[tid * N + k];
      __syncthreads();
      if (row && tid >= k) {
        double acc = 0.0;
        for (int j = 0; j < k; j++) acc += Lm[j * N + tid] * tmp[j];
        Lm[k * N + tid] -= acc;
      }
      __syncthreads();
    }
    const double akk = Lm[k * N + k];
    const bool valid = fabs(akk) > 0.0;
    if (k == 0 && !valid) {
      all_zero = true;
      break;
    }
    if (row && tid > k && valid) Lm[k * N + tid] /= akk; // (lane k's own entry, the pivot, stays as every lane reads it)
    if (tid == k) dg[k] = akk;
    __syncthreads();
  }
  if (all_zero) {
    y = 0.0;
  } else {
    for (int j = 0; j + 1 < N; j++) { // L^-1
      if (tid == j) yv[j] = y;
      __syncthreads();
      if (row && tid > j) y -= Lm[j * N + tid] * yv[j];
    }
    if (row) y = sol::d_inverse(y, dg[tid]);
    for (int i = N - 1; i >= 0; i--) { // L^-T: the products of column i in parallel, the chain of y[i] in lane i
      double *buf = (i & 1) ? tmp : yv;
      if (row && tid > i) buf[tid] = Lm[i * N + tid] * y;
      __syncthreads();
      if (tid == i)
        for (int j = i + 1; j < N; j++) y -= buf[j];
    }
  }
  if (row) xs[perm[tid]] = y;
  __syncthreads();
  double x = row ? v[tid] * xs[tid] : 0.0;
  if (J.n_null > 0) { // F7
    if (row) av[tid] = x;
    __syncthreads();
    if (tid < J.n_null) {
      const double *pinv = sd + J.d_pinv + (long long)tid * N;
      double t = 0.0;
      for (int i = 0; i < N; i++) t += pinv[i] * av[i];
      dg[tid] = t;
    }
    __syncthreads();
    if (row) {
      const double *basis = sd + J.d_basis + (long long)tid * J.n_null;
      double t = 0.0;
      for (int k = 0; k < J.n_null; k++) t += basis[k] * dg[k];
      x = x - t;
    }
  }
  if (row) {
    dbl(base, J.o_x)[tid] = x;
    if (not_finite(x)) *bad = 1;
  }
  __syncthreads();
  if (tid == 0) reinterpret_cast<int *>(base)[J.o_flags] = *bad ? DSM_SOLVE_X_NOT_FINITE : 0; // R3, bit 0
}

__global__ __launch_bounds__(kStepBlock) void sol_step_kernel(const SolJob *jobs, const double *sd, const float *stage, float *base) {
  const SolJob &J = jobs[blockIdx.y];
  const int nf = J.V.n_frames, tid = threadIdx.x;
  if (blockIdx.x * kStepBlock >= J.V.n_pts) return; // uniform over the workgroup
  __shared__ float xad[DSM_WINDOW_MAX_FRAMES * DSM_WINDOW_MAX_FRAMES * 8];
  const double *x = dbl(base, J.o_x);
  for (int idx = tid; idx < nf * nf * 8; idx += kStepBlock) { // R1
    const int pr = idx >> 3, h = pr / nf, t = pr - h * nf;
    xad[idx] = h == t ? 0.0f : sol::x_ad(x, h, t, sd + J.d_adh + (long long)pr * 64, sd + J.d_adt + (long long)pr * 64, idx & 7);
  }
  __syncthreads();
  const int p = blockIdx.x * kStepBlock + tid;
  if (p >= J.V.n_pts) return;
  const int *stage_i = reinterpret_cast<const int *>(stage);
  const float *prec = base + J.V.o_prec + (long long)hes::P_FLOATS * p;
  float st = 0.0f;
  if (__float_as_int(prec[hes::P_NACT])) { // R2
    float b = sol::step_begin(prec[hes::P_BDSUM], x, prec + hes::P_HCDSUM);
    const int h = stage_i[J.V.off_host + p];
    for (int k = stage_i[J.V.off_pt_start + p]; k < stage_i[J.V.off_pt_start + p + 1]; k++) { // ascending residual index
      const int r = stage_i[J.V.off_pt_list + k];
      const float *rec = base + J.V.o_rec + (long long)hes::R_FLOATS * r;
      if (!reinterpret_cast<const int *>(rec)[hes::R_ACTIVE]) continue;
      b = sol::step_residual(b, xad + (h * nf + stage_i[J.V.off_target + r]) * 8, rec + hes::R_JP);
    }
    st = sol::step_end(b, prec[hes::P_HDI]);
  }
  base[J.o_step + p] = st;
  if (!(fabsf(st) <= 3.402823466e38f)) atomicOr(reinterpret_cast<int *>(base) + J.o_flags, DSM_SOLVE_STEP_NOT_FINITE); // R3, bit 1
}

size_t solve_lds_bytes(int N) { return 8 * ((size_t)N * N + 7 * (size_t)N) + 4 * ((size_t)N + 2); }

} // namespace

extern "C" int dsm_window_solve_batch(dsm_context *ctx, int n_jobs, const dsm_solve_job *jobs, const dsm_linearize_params *params) {
  auto bad = [](const char *msg) { return invalid((std::string("dsm_window_solve_batch: ") + msg).c_str()); };
  size_t res = 0;
  std::vector<const dsm_linearize_job *> lin;
  for (int j = 0; jobs && j < n_jobs; j++) lin.push_back(&jobs[j].hes.lin);
  int rc = linearize_check_jobs("dsm_window_solve_batch", ctx, n_jobs, jobs ? lin.data() : nullptr, params, &res);
  if (rc) return rc;
  for (int j = 0; j < n_jobs; j++) {
    if (const char *e = hessian_job_error(jobs[j].hes, false)) return bad(e);
    if (const char *e = solve_job_error(jobs[j])) return bad(e);
  }
  CallArena A;
  SolPlan P;
  for (int j = 0; j < n_jobs; j++) P.jobs.push_back(&jobs[j]);
  solve_layout(P, A);
  if ((rc = A.bind(ctx))) return rc;
  solve_stage(P, A);
  if ((rc = A.upload())) return rc;
  if ((rc = solve_launch(ctx, P, A, *params))) return rc;
  if ((rc = A.fetch(A.out.used))) return rc;
  solve_unpack(P, A, *params);
  return DSM_OK;
}

namespace dsm {

// on top of the Hessian call's parts: staged [job table | doubles: ad_host, ad_target, H_L, b_L and the optional inputs], device only
// or read back (a job that asks for one of them) [H_A, b_A, H_sc, b_sc], read back [x, steps, flags, as asked for: last_HS, last_bS].
// A stitch_only plan (dsm_window_marginalize_batch) has jobs without H_L / b_L (counted only where given; every other caller's
// validation refuses a NULL one) and takes no room for x, the steps and the flags: only sol_stitch_kernel runs on it.
void solve_layout(SolPlan &P, CallArena &A) {
  const int n_jobs = (int)P.jobs.size();
  P.hes.lean = true;
  for (int j = 0; j < n_jobs; j++) P.hes.jobs.push_back(&P.jobs[j]->hes);
  hessian_layout(P.hes, A);
  P.at.assign(n_jobs, SolWhere());
  size_t doubles = 0;
  for (int j = 0; j < n_jobs; j++) {
    const dsm_solve_job &S = *P.jobs[j];
    const size_t nf = S.hes.lin.n_frames, N = 4 + 8 * nf;
    SolWhere &w = P.at[j];
    doubles += 2 * nf * nf * 64 + (S.H_L ? N * N : 0) + (S.b_L ? N : 0) + (S.H_M ? N * N : 0) + (S.b_M ? N : 0) + (S.delta_x ? N : 0) +
               2 * N * (size_t)S.n_null;
    const bool out = S.hes.H_A || S.hes.b_A || S.hes.H_sc || S.hes.b_sc;
    auto take = [&A, out](size_t bytes) {
      HesSpot s;
      s.out = out, s.at = (out ? A.out : A.work).take(bytes);
      return s;
    };
    w.HA = take(8 * N * N), w.bA = take(8 * N), w.HS = take(8 * N * N), w.bS = take(8 * N);
    if (!P.stitch_only) w.x = A.out.take(8 * N), w.step = A.out.take(4 * (size_t)S.hes.lin.n_pts), w.flags = A.out.take(4);
    if (S.last_HS) w.lastH = (long long)A.out.take(8 * N * N);
    if (S.last_bS) w.lastb = (long long)A.out.take(8 * N);
    P.max_N = std::max(P.max_N, (int)N);
  }
  P.o_sol = A.in.take(sizeof(SolJob) * n_jobs), P.o_sd = A.in.take(8 * doubles);
  P.sol_stride = sizeof(SolJob), P.sol_lambda = offsetof(SolJob, lambda);
}

void solve_stage(SolPlan &P, CallArena &A) {
  const int n_jobs = (int)P.jobs.size();
  hessian_stage(P.hes, A);
  SolJob *hs = A.host_in<SolJob>(P.o_sol);
  double *hd = A.host_in<double>(P.o_sd);
  size_t used = 0;
  auto put = [&](const double *a, size_t n) {
    if (!a) return -1ll;
    memcpy(hd + used, a, 8 * n);
    used += n;
    return (long long)(used - n);
  };
  const long long out0 = P.hes.out0;
  P.view.assign(n_jobs, SolView());
  for (int j = 0; j < n_jobs; j++) {
    const dsm_solve_job &S = *P.jobs[j];
    const size_t nf = S.hes.lin.n_frames, N = 4 + 8 * nf;
    const SolWhere &w = P.at[j];
    SolJob &G = hs[j];
    memset(&G, 0, sizeof G);
    G.V = P.hes.view[j], G.N = (int)N, G.n_null = S.n_null, G.lambda = S.lambda;
    G.d_adh = put(S.hes.ad_host, nf * nf * 64), G.d_adt = put(S.hes.ad_target, nf * nf * 64);
    G.d_HL = put(S.H_L, N * N), G.d_bL = put(S.b_L, N), G.d_HM = put(S.H_M, N * N), G.d_bM = put(S.b_M, N), G.d_dx = put(S.delta_x, N);
    G.d_basis = put(S.n_null ? S.null_basis : nullptr, N * S.n_null), G.d_pinv = put(S.n_null ? S.null_pinv : nullptr, N * S.n_null);
    G.o_HA = w.HA.word(out0), G.o_bA = w.bA.word(out0), G.o_HS = w.HS.word(out0), G.o_bS = w.bS.word(out0);
    G.o_x = out0 + (long long)(w.x / 4), G.o_step = out0 + (long long)(w.step / 4), G.o_flags = out0 + (long long)(w.flags / 4);
    if (P.stitch_only) G.o_x = G.o_step = G.o_flags = -1; // no room was taken: sol_solve_kernel and sol_step_kernel do not run
    G.o_lastH = w.lastH < 0 ? -1 : out0 + w.lastH / 4, G.o_lastb = w.lastb < 0 ? -1 : out0 + w.lastb / 4;
    P.view[j] = SolView{(int)N, G.d_HL, G.d_bL, G.d_HM, G.d_bM, G.d_dx};
  }
}

int solve_launch_stitch(dsm_context *ctx, SolPlan &P, CallArena &A) {
  const int n_jobs = (int)P.jobs.size(), nf = P.hes.max_nf;
  hipLaunchKernelGGL(sol_stitch_kernel, dim3(nf * (nf + 1) / 2 + nf + 1, n_jobs), dim3(64), 0, ctx->stream, A.dev_in<const SolJob>(P.o_sol),
                     A.dev_in<const double>(P.o_sd), P.hes.dev_base);
  return DSM_OK;
}

int solve_launch(dsm_context *ctx, SolPlan &P, CallArena &A, const dsm_linearize_params &params) {
  const int n_jobs = (int)P.jobs.size();
  if (int rc = hessian_launch(ctx, P.hes, A, params)) return rc;
  const SolJob *ds = A.dev_in<const SolJob>(P.o_sol);
  const double *dd = A.dev_in<const double>(P.o_sd);
  const size_t lds = solve_lds_bytes(P.max_N);
  if (lds > 64 * 1024) DSM_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(sol_solve_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  if (int rc = solve_launch_stitch(ctx, P, A)) return rc;
  hipLaunchKernelGGL(sol_solve_kernel, dim3(n_jobs), dim3(kSolveBlock), lds, ctx->stream, ds, dd, P.hes.dev_base);
  if (P.hes.max_pts)
    hipLaunchKernelGGL(sol_step_kernel, dim3((P.hes.max_pts + kStepBlock - 1) / kStepBlock, n_jobs), dim3(kStepBlock), 0, ctx->stream, ds, dd,
                       P.hes.dev_stage, P.hes.dev_base);
  DSM_HIP(hipGetLastError());
  return DSM_OK;
}

void solve_unpack(const SolPlan &P, const CallArena &A, const dsm_linearize_params &params) {
  const int n_jobs = (int)P.jobs.size();
  hessian_unpack(P.hes, A, params);
  const unsigned char *ho = A.host_out<unsigned char>(0);
  for (int j = 0; j < n_jobs; j++) {
    const dsm_solve_job &S = *P.jobs[j];
    const size_t N = 4 + 8 * (size_t)S.hes.lin.n_frames;
    const SolWhere &w = P.at[j];
    if (S.hes.H_A) memcpy(S.hes.H_A, ho + w.HA.at, 8 * N * N);
    if (S.hes.b_A) memcpy(S.hes.b_A, ho + w.bA.at, 8 * N);
    if (S.hes.H_sc) memcpy(S.hes.H_sc, ho + w.HS.at, 8 * N * N);
    if (S.hes.b_sc) memcpy(S.hes.b_sc, ho + w.bS.at, 8 * N);
    if (P.stitch_only) continue;
    memcpy(S.x, ho + w.x, 8 * N);
    if (S.hes.lin.n_pts) memcpy(S.step, ho + w.step, 4 * (size_t)S.hes.lin.n_pts);
    memcpy(S.flags, ho + w.flags, 4);
    if (S.last_HS) memcpy(S.last_HS, ho + w.lastH, 8 * N * N);
    if (S.last_bS) memcpy(S.last_bS, ho + w.lastb, 8 * N);
  }
}

} // namespace dsm
