// marginalize_kernels.hip -- what FrontEnd::makeKeyFrame does right after optimize (FrontEnd.cpp:816-839) on the device, for the
// windows of many sequences in one call: the verdicts of flagPointsForRemoval, marginalizePointsF and marginalizeFrame.  Semantics:
// C, M1, X1, A1', M2, G1-G7, Z, V of DESIGN.md section 21.
//
// One dsm_window_marginalize_batch = the verdicts (C) on the host while staging, ONE staged copy of the sub-window of M1 (the points
// of verdict 1 with all their residuals, a Hessian job of its own), NINE launches on the context's stream, one read-back:
//   linearize_kernel    (linearize_kernels.hip, unchanged) over the sub-window; the rows stay in the device-only part of the arena
//   mrg_fix_kernel      one lane per residual of the sub-window: X1 on an active row, res_toZeroF written WHERE THE ROW'S resF STANDS,
//                       so that the unchanged accumulation forms A1'; also into the read-back when the job asks for res_to_zero
//   hes_residual_kernel, hes_point_kernel, hes_pair_kernel, hes_schur_kernel (hessian_kernels.hip, unchanged)
//   sol_stitch_kernel   (solve_kernels.hip, unchanged): T1d
//   mrg_fold_kernel     one lane per entry of the N x N prior and of its right-hand side: M2
//   mrg_frame_kernel    one workgroup per job: G1-G7 for the job's marginalised frames, one after the other.  The system sits in LDS
//                       (dynamic; above 64 KB the launch raises the kernel's limit as sol_solve_kernel's does: N = 132 takes 150 KB).
//                       G1 is the load (the frame's rows and columns move to the end), G3, G4, G6 and G7 are element-parallel with one
//                       chain per entry, G5 (the 8 x 8 inverse) runs in lane 0 on LDS operands.  A frame's result goes to the job's
//                       output in global memory with its own stride and is the next frame's input: every lane has loaded its part
//                       before a workgroup barrier lets any lane overwrite it.  A job without a marginalised frame returns at once.
// Every result is ONE sequential chain in one lane, in the stated order: it does not depend on the launch geometry or on the other
// jobs of the call.  No kernel waits for another workgroup; barriers are workgroup-local.  No MFMA, no scratch.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "solve_launch.hpp"

#include "marginalize_internal.hpp"
#include "marginalize_math.hpp"

using namespace dsm;

namespace {

constexpr int kFixBlock = 256;   // mrg_fix_kernel: residuals per workgroup
constexpr int kFoldBlock = 256;  // mrg_fold_kernel: entries per workgroup
constexpr int kFrameBlock = 256; // mrg_frame_kernel: one workgroup per job

struct MrgJob {
  int N, n_marg;
  float weight;
  // 4-byte words into the call's staged floats; off_frames: n_marg ints
  int off_dp, off_cd, off_delta, off_frames;
  // doubles into the call's staged doubles; d_HM, d_bM -1 for zeros
  long long d_HM, d_bM, d_prior, d_dprior;
  // 4-byte words from the start of the arena's device-only part, every one at a multiple of eight bytes; o_rtz -1: not asked for,
  // o_Ho, o_bo -1: no frame leaves
  long long o_HA, o_bA, o_HS, o_bS, o_Hp, o_bp, o_Ho, o_bo, o_rtz;
};

__device__ __forceinline__ double *dbl(float *base, long long word) { return reinterpret_cast<double *>(base + word); }

__global__ __launch_bounds__(kFixBlock) void mrg_fix_kernel(const LinJob *lin_jobs, const MrgJob *jobs, const float *lin_stage, const float *stage,
                                                            float *base) {
  const LinJob &L = lin_jobs[blockIdx.y];
  const MrgJob &J = jobs[blockIdx.y];
  const int r = blockIdx.x * kFixBlock + threadIdx.x;
  if (r >= L.n_res) return;
  if ((__float_as_int(base[L.o_head + (long long)kLinHeadWords * r]) & 0xff) != lin::RES_IN) return; // A0: every residual entered IN
  const int *stage_i = reinterpret_cast<const int *>(lin_stage);
  const int p = stage_i[L.off_point + r], h = stage_i[L.off_host + p], t = stage_i[L.off_target + r];
  float *row = base + L.o_J + (long long)lin::J_FLOATS * r;
  mrg::res_to_zero(row, stage + J.off_dp + 8 * (h * L.n_frames + t), stage + J.off_cd, stage[J.off_delta + p], row + lin::J_RESF); // X1
  if (J.o_rtz >= 0) {
    float *out = base + J.o_rtz + 8ll * r;
#pragma unroll
    for (int i = 0; i < 8; i++) out[i] = row[lin::J_RESF + i];
  }
}

__global__ __launch_bounds__(kFoldBlock) void mrg_fold_kernel(const MrgJob *jobs, const double *sd, float *base) {
  const MrgJob &J = jobs[blockIdx.y];
  const int N = J.N, e = blockIdx.x * kFoldBlock + threadIdx.x;
  const double w = (double)J.weight;
  if (e < N * N) {
    dbl(base, J.o_Hp)[e] = mrg::fold(J.d_HM >= 0 ? sd[J.d_HM + e] : 0.0, w, dbl(base, J.o_HA)[e], dbl(base, J.o_HS)[e]);
  } else if (e < N * N + N) {
    const int i = e - N * N;
    dbl(base, J.o_bp)[i] = mrg::fold(J.d_bM >= 0 ? sd[J.d_bM + i] : 0.0, w, dbl(base, J.o_bA)[i], dbl(base, J.o_bS)[i]);
  }
}

__global__ __launch_bounds__(kFrameBlock) void mrg_frame_kernel(const MrgJob *jobs, const double *sd, const float *stage, float *base) {
  extern __shared__ double lds[];
  const MrgJob &J = jobs[blockIdx.x];
  if (J.n_marg == 0) return; // uniform over the workgroup
  const int N0 = J.N, tid = threadIdx.x, nt = blockDim.x;
  double *Hs = lds, *bs = Hs + N0 * N0, *S = bs + N0, *SI = S + N0, *bli = SI + N0, *a = bli + 8 * (N0 - 8), *P = a + 64, *y = P + 64;
  int *piv = reinterpret_cast<int *>(y + 8);
  const int *frames = reinterpret_cast<const int *>(stage) + J.off_frames;
  double *Ho = dbl(base, J.o_Ho), *bo = dbl(base, J.o_bo);
  const double *srcH = dbl(base, J.o_Hp), *srcb = dbl(base, J.o_bp);
  int n = N0;
  for (int m = 0; m < J.n_marg; m++) {
    const int f = frames[m] - m, nd = n - 8; // the frames before it have left
    for (int e = tid; e < n * n; e += nt) { // G1
      const int i = e / n, j = e - i * n;
      Hs[e] = srcH[(long long)mrg::source_index(i, f, n) * n + mrg::source_index(j, f, n)];
    }
    for (int i = tid; i < n; i += nt) bs[i] = srcb[mrg::source_index(i, f, n)];
    __syncthreads();
    if (tid < 8) { // G2
      const double pr = sd[J.d_prior + 8 * m + tid];
      Hs[(nd + tid) * n + nd + tid] += pr;
      bs[nd + tid] += pr * sd[J.d_dprior + 8 * m + tid];
    }
    __syncthreads();
    for (int i = tid; i < n; i += nt) { // G3
      const double s = mrg::scale_of(Hs[i * n + i]);
      S[i] = s, SI[i] = mrg::scale_inverse(s);
    }
    __syncthreads();
    for (int e = tid; e < n * n; e += nt) { // G4
      const int i = e / n, j = e - i * n;
      Hs[e] = mrg::scaled(SI[i], Hs[e], SI[j]);
    }
    for (int i = tid; i < n; i += nt) bs[i] = SI[i] * bs[i];
    __syncthreads();
    if (tid < 64) a[tid] = Hs[(nd + (tid >> 3)) * n + nd + (tid & 7)];
    __syncthreads();
    if (tid == 0) mrg::lu_inverse8(a, P, piv, y); // G5
    __syncthreads();
    const double *bottom = Hs + nd * n;
    for (int q = tid; q < nd * 8; q += nt) bli[q] = mrg::bli_entry(bottom + (q >> 3), n, P + (q & 7)); // G6
    __syncthreads();
    for (int e = tid; e < nd * nd; e += nt) {
      const int i = e / nd, j = e - i * nd;
      Hs[i * n + j] = mrg::schur_entry(Hs[i * n + j], bli + 8 * i, bottom + j, n);
    }
    for (int i = tid; i < nd; i += nt) bs[i] = mrg::schur_entry(bs[i], bli + 8 * i, bs + nd, 1);
    __syncthreads();
    for (int e = tid; e < nd * nd; e += nt) { // G7
      const int i = e / nd, j = e - i * nd;
      Ho[e] = mrg::symmetrised(mrg::scaled(S[i], Hs[i * n + j], S[j]), mrg::scaled(S[j], Hs[j * n + i], S[i]));
    }
    for (int i = tid; i < nd; i += nt) bo[i] = S[i] * bs[i];
    __threadfence_block();
    __syncthreads(); // the next frame's load reads what every lane wrote
    srcH = Ho, srcb = bo, n = nd;
  }
}

size_t frame_lds_bytes(int N) { return 8 * ((size_t)N * N + 3 * (size_t)N + 8 * (size_t)(N - 8) + 64 + 64 + 8) + 4 * 8; }

struct MrgWhere {
  HesSpot Hp, bp;
  long long Ho = -1, bo = -1, rtz = -1; // bytes into out; -1: none
};

} // namespace

extern "C" int dsm_window_marginalize_batch(dsm_context *ctx, int n_jobs, const dsm_marginalize_job *jobs, const dsm_linearize_params *lin_params,
                                            const dsm_marginalize_params *marg_params) {
  auto bad = [](const char *msg) { return invalid((std::string("dsm_window_marginalize_batch: ") + msg).c_str()); };
  size_t res = 0;
  std::vector<const dsm_linearize_job *> lin;
  for (int j = 0; jobs && j < n_jobs; j++) lin.push_back(&jobs[j].hes.lin);
  int rc = linearize_check_jobs("dsm_window_marginalize_batch", ctx, n_jobs, jobs ? lin.data() : nullptr, lin_params, &res);
  if (rc) return rc;
  if (const char *e = marginalize_params_error(marg_params)) return bad(e);
  std::vector<std::vector<unsigned char>> verdict(n_jobs);
  for (int j = 0; j < n_jobs; j++) {
    if (const char *e = hessian_job_error(jobs[j].hes, false)) return bad(e);
    if (const char *e = marginalize_job_error(jobs[j], *marg_params, verdict[j])) return bad(e); // C
  }
  std::vector<MrgSub> subs(n_jobs); // M1; they point into themselves and stay where they are
  CallArena A;
  SolPlan P;
  P.stitch_only = true;
  for (int j = 0; j < n_jobs; j++) {
    marginalize_sub(jobs[j], *marg_params, verdict[j].data(), subs[j]);
    P.jobs.push_back(&subs[j].job);
  }
  // on top of the solve call's parts: staged [job table | floats: ad_ht_delta, c_delta, the sub-window's delta, marg_frames |
  // doubles: H_M, b_M, frame_prior, frame_delta_prior], device only or read back (a job that asks for it, or of which no frame
  // leaves) [the prior after the points], read back [the prior after the frames, as asked for: res_to_zero]
  solve_layout(P, A);
  std::vector<MrgWhere> at(n_jobs);
  size_t words = 0, doubles = 0;
  int max_N = 12, max_marg = 0;
  for (int j = 0; j < n_jobs; j++) {
    const dsm_marginalize_job &M = jobs[j];
    const size_t nf = M.hes.lin.n_frames, N = 4 + 8 * nf, nm = M.n_marg_frames;
    words += nf * nf * 8 + 4 + subs[j].pts.size() + nm;
    doubles += (M.H_M ? N * N : 0) + (M.b_M ? N : 0) + 16 * nm;
    MrgWhere &w = at[j];
    const bool out = M.H_M_points || M.b_M_points || nm == 0;
    w.Hp.out = w.bp.out = out;
    w.Hp.at = (out ? A.out : A.work).take(8 * N * N), w.bp.at = (out ? A.out : A.work).take(8 * N);
    if (nm) w.Ho = (long long)A.out.take(8 * (N - 8) * (N - 8)), w.bo = (long long)A.out.take(8 * (N - 8));
    if (M.res_to_zero && !subs[j].res.empty()) w.rtz = (long long)A.out.take(4 * 8 * subs[j].res.size());
    max_N = std::max(max_N, (int)N), max_marg = std::max(max_marg, (int)nm);
  }
  const size_t o_mrg = A.in.take(sizeof(MrgJob) * n_jobs), o_words = A.in.take(4 * words), o_doubles = A.in.take(8 * doubles);
  if ((rc = A.bind(ctx))) return rc;
  solve_stage(P, A);
  {
    const long long out0 = P.hes.out0;
    MrgJob *hm = A.host_in<MrgJob>(o_mrg);
    WordPacker W{A.host_in<float>(o_words)};
    double *hd = A.host_in<double>(o_doubles);
    size_t used = 0;
    auto put = [&](const double *a, size_t n) {
      if (!a) return -1ll;
      memcpy(hd + used, a, 8 * n);
      used += n;
      return (long long)(used - n);
    };
    for (int j = 0; j < n_jobs; j++) {
      const dsm_marginalize_job &M = jobs[j];
      const size_t nf = M.hes.lin.n_frames, N = 4 + 8 * nf, nm = M.n_marg_frames;
      const MrgWhere &w = at[j];
      const SolWhere &s = P.at[j];
      MrgJob &G = hm[j];
      memset(&G, 0, sizeof G);
      G.N = (int)N, G.n_marg = (int)nm, G.weight = marg_params->marg_weight_fac;
      W.put(&G.off_dp, M.ad_ht_delta, nf * nf * 8), W.put(&G.off_cd, M.c_delta, 4);
      W.put(&G.off_delta, subs[j].delta.data(), subs[j].delta.size()), W.put(&G.off_frames, M.marg_frames, nm);
      G.d_HM = put(M.H_M, N * N), G.d_bM = put(M.b_M, N);
      G.d_prior = put(nm ? M.frame_prior : nullptr, 8 * nm), G.d_dprior = put(nm ? M.frame_delta_prior : nullptr, 8 * nm);
      G.o_HA = s.HA.word(out0), G.o_bA = s.bA.word(out0), G.o_HS = s.HS.word(out0), G.o_bS = s.bS.word(out0);
      G.o_Hp = w.Hp.word(out0), G.o_bp = w.bp.word(out0);
      G.o_Ho = w.Ho < 0 ? -1 : out0 + w.Ho / 4, G.o_bo = w.bo < 0 ? -1 : out0 + w.bo / 4, G.o_rtz = w.rtz < 0 ? -1 : out0 + w.rtz / 4;
    }
  }
  if ((rc = A.upload())) return rc;
  const MrgJob *dm = A.dev_in<const MrgJob>(o_mrg);
  const float *dw = A.dev_in<const float>(o_words);
  const double *dd = A.dev_in<const double>(o_doubles);
  float *base = P.hes.dev_base;
  if ((rc = hessian_launch_linearize(ctx, P.hes, A, *lin_params))) return rc;
  if (P.hes.max_res)
    hipLaunchKernelGGL(mrg_fix_kernel, dim3((P.hes.max_res + kFixBlock - 1) / kFixBlock, n_jobs), dim3(kFixBlock), 0, ctx->stream,
                       A.dev_in<const LinJob>(P.hes.o_lin), dm, P.hes.dev_stage, dw, base);
  if ((rc = hessian_launch_accumulate(ctx, P.hes, A))) return rc;
  if ((rc = solve_launch_stitch(ctx, P, A))) return rc;
  hipLaunchKernelGGL(mrg_fold_kernel, dim3((max_N * max_N + max_N + kFoldBlock - 1) / kFoldBlock, n_jobs), dim3(kFoldBlock), 0, ctx->stream, dm, dd, base);
  if (max_marg) {
    const size_t lds = frame_lds_bytes(max_N);
    if (lds > 64 * 1024)
      DSM_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(mrg_frame_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(mrg_frame_kernel, dim3(n_jobs), dim3(kFrameBlock), lds, ctx->stream, dm, dd, dw, base);
  }
  DSM_HIP(hipGetLastError());
  if ((rc = A.fetch(A.out.used))) return rc;
  solve_unpack(P, A, *lin_params);
  const unsigned char *ho = A.host_out<unsigned char>(0);
  for (int j = 0; j < n_jobs; j++) {
    const dsm_marginalize_job &M = jobs[j];
    const size_t N = 4 + 8 * (size_t)M.hes.lin.n_frames, Nn = N - 8 * (size_t)M.n_marg_frames;
    const MrgWhere &w = at[j];
    marginalize_scatter(M, verdict[j].data(), subs[j]); // Z
    if (w.rtz >= 0)
      for (size_t i = 0; i < subs[j].res.size(); i++)
        if (subs[j].active[i]) memcpy(M.res_to_zero + 8 * (size_t)subs[j].res[i], ho + w.rtz + 32 * i, 32);
    if (M.H_M_points) memcpy(M.H_M_points, ho + w.Hp.at, 8 * N * N);
    if (M.b_M_points) memcpy(M.b_M_points, ho + w.bp.at, 8 * N);
    memcpy(M.H_M_out, ho + (M.n_marg_frames ? (size_t)w.Ho : w.Hp.at), 8 * Nn * Nn);
    memcpy(M.b_M_out, ho + (M.n_marg_frames ? (size_t)w.bo : w.bp.at), 8 * Nn);
  }
  return DSM_OK;
}
