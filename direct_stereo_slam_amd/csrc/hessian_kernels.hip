// hessian_kernels.hip -- accumulateAF_MT / accumulateSCF_MT of FrontEnd::optimize (dso_helpers/FrontEndOptimize.cpp:332-486) on the
// device, for the windows of many sequences in one call.  Semantics: A0-A3, P1, S1-S3, T1, V of DESIGN.md section 17.
//
// One dsm_window_hessian_batch = one staged copy, FIVE launches on the context's stream, one read-back:
//   linearize_kernel     (linearize_kernels.hip, unchanged) with a row for every residual; the rows go to the device-only part of the
//                        call arena unless the job's lin.J_out asks for them
//   hes_residual_kernel  one lane per residual: A0, and for an active residual its record (A1, A2 and the operands of A3 in the order
//                        the later kernels pick them by address)
//   hes_point_kernel     one lane per point: S1 over its residual list in ascending residual index, S2, and the point's row of the
//                        slot table (target -> active residual, -1: none)
//   hes_pair_kernel      one workgroup per [host][target] pair, one lane per entry of the upper half of the 13 x 13 accumulator (P1):
//                        the pair's residual list is walked in chunks of kPairChunk records staged in LDS, every lane adds the float
//                        term of its entry to a double, in list order
//   hes_schur_kernel     one workgroup per (host, t1) and one more per job (S3): the host's points are walked in ascending index in
//                        chunks of kSchurChunk staged in LDS (per point its S2 results and the JpJdF of its active residual against
//                        every target); lane 64 t2 + 8 a + b holds acc_D[host][t1][t2][a][b], the 64 lanes of t2 == host (a block that
//                        is always zero: a frame is no target of its own points) hold acc_E[host][t1] and acc_EB[host][t1]; the extra
//                        workgroup walks all points in chunks of kHccChunk for acc_Hcc and acc_bc
// Every accumulator entry is ONE sequential chain in one lane, in the stated order: the result does not depend on the launch
// geometry or on the other jobs of the call.  The parallelism is across entries, pairs, hosts and jobs.  No kernel waits for another
// workgroup; barriers are workgroup-local (LDS staging).  No MFMA.  Operands are picked by address from LDS (hessian_math.hpp).
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "hessian_launch.hpp"

#include "hessian_math.hpp"

using namespace dsm;

namespace {

constexpr int kResBlock = 256;  // hes_residual_kernel: residuals per workgroup
constexpr int kPtBlock = 64;    // hes_point_kernel: points per workgroup
constexpr int kPairBlock = 128; // hes_pair_kernel: 91 entries, the rest only stage
constexpr int kPairChunk = 16;  // records of one pair in LDS at a time
constexpr int kSchurChunk = 32; // points of one host in LDS at a time
constexpr int kHccChunk = 128;  // points in LDS at a time in the workgroup of acc_Hcc / acc_bc
constexpr int kPairRec = hes::R_TOP_END + 1; // the operands of A3 and the active flag

struct HesJob {
  int n_frames, n_pts, n_res, shift;
  // 4-byte words into the staged inputs; the optional per-point inputs -1 for zeros
  int off_pair_start, off_pair_list, off_pt_start, off_pt_list, off_host_start, off_host_pts;
  int off_prior, off_delta, off_hdd_lin, off_bd_lin, off_hcd_lin;
  // 4-byte words from the start of the arena's device-only part
  long long o_rows, o_rec, o_prec, o_slot, o_jp, o_top, o_D, o_E, o_EB, o_Hcc, o_bc; // o_jp -1: JpJdF is not asked for
};

__global__ __launch_bounds__(kResBlock) void hes_residual_kernel(const LinJob *lin_jobs, const HesJob *jobs, const float *stage, float *base) {
  const LinJob &L = lin_jobs[blockIdx.y];
  const HesJob &J = jobs[blockIdx.y];
  const int r = blockIdx.x * kResBlock + threadIdx.x;
  if (r >= J.n_res) return;
  const int state_in = reinterpret_cast<const int *>(stage)[L.off_flags + r] & 0xff;
  const int new_state = __float_as_int(base[L.o_head + (long long)kLinHeadWords * r]) & 0xff;
  const int active = state_in != lin::RES_OOB && new_state == lin::RES_IN; // A0
  float *rec = base + J.o_rec + (long long)hes::R_FLOATS * r;
  reinterpret_cast<int *>(rec)[hes::R_ACTIVE] = active;
  if (!active) return;
  hes::residual_record(base + J.o_rows + (long long)lin::J_FLOATS * r, rec); // A1, A2
  if (J.o_jp >= 0) {
    float *jp = base + J.o_jp + 8ll * r;
#pragma unroll
    for (int i = 0; i < 8; i++) jp[i] = rec[hes::R_JP + i];
  }
}

__global__ __launch_bounds__(kPtBlock) void hes_point_kernel(const LinJob *lin_jobs, const HesJob *jobs, const float *stage, float *base) {
  const LinJob &L = lin_jobs[blockIdx.y];
  const HesJob &J = jobs[blockIdx.y];
  const int p = blockIdx.x * kPtBlock + threadIdx.x;
  if (p >= J.n_pts) return;
  const int *stage_i = reinterpret_cast<const int *>(stage);
  const int nf = J.n_frames;
  int *slot = reinterpret_cast<int *>(base + J.o_slot) + (long long)p * nf;
  for (int t = 0; t < nf; t++) slot[t] = -1;
  float bd = 0.0f, hdd = 0.0f, h0 = 0.0f, h1 = 0.0f, h2 = 0.0f, h3 = 0.0f;
  int n_active = 0;
  const int s = stage_i[J.off_pt_start + p], e = stage_i[J.off_pt_start + p + 1];
  for (int k = s; k < e; k++) { // S1: ascending residual index
    const int r = stage_i[J.off_pt_list + k];
    const float *rec = base + J.o_rec + (long long)hes::R_FLOATS * r;
    if (!reinterpret_cast<const int *>(rec)[hes::R_ACTIVE]) continue;
    hes::point_add(rec, bd, hdd, h0, h1, h2, h3);
    slot[stage_i[L.off_target + r]] = r;
    n_active++;
  }
  float *prec = base + J.o_prec + (long long)hes::P_FLOATS * p;
  prec[hes::P_HDD] = hdd, prec[hes::P_BD] = bd;
  prec[hes::P_HCD] = h0, prec[hes::P_HCD + 1] = h1, prec[hes::P_HCD + 2] = h2, prec[hes::P_HCD + 3] = h3;
  hes::point_finish(prec, n_active, J.off_prior >= 0 ? stage[J.off_prior + p] : 0.0f, J.off_delta >= 0 ? stage[J.off_delta + p] : 0.0f,
                    J.off_hdd_lin >= 0 ? stage[J.off_hdd_lin + p] : 0.0f, J.off_bd_lin >= 0 ? stage[J.off_bd_lin + p] : 0.0f,
                    J.off_hcd_lin >= 0 ? stage + J.off_hcd_lin + 4 * p : nullptr, J.shift != 0); // S2
}

__global__ __launch_bounds__(kPairBlock) void hes_pair_kernel(const HesJob *jobs, const float *stage, float *base) {
  const HesJob &J = jobs[blockIdx.y];
  const int pair = blockIdx.x, tid = threadIdx.x;
  if (pair >= J.n_frames * J.n_frames) return; // uniform over the workgroup
  __shared__ float rec[kPairChunk][kPairRec];
  const int *stage_i = reinterpret_cast<const int *>(stage);
  const int s = stage_i[J.off_pair_start + pair], e = stage_i[J.off_pair_start + pair + 1];
  int a = 0, b = 0;
  if (tid < hes::kTopEntries) hes::top_entry(tid, a, b);
  double acc = 0.0;
  for (int c = s; c < e; c += kPairChunk) {
    const int n = min(kPairChunk, e - c);
    for (int idx = tid; idx < n * kPairRec; idx += kPairBlock) {
      const int i = idx / kPairRec, f = idx - i * kPairRec;
      const int r = stage_i[J.off_pair_list + c + i];
      rec[i][f] = base[J.o_rec + (long long)hes::R_FLOATS * r + (f < hes::R_TOP_END ? f : hes::R_ACTIVE)];
    }
    __syncthreads();
    if (tid < hes::kTopEntries)
      for (int i = 0; i < n; i++) // P1: ascending residual index
        if (__float_as_int(rec[i][hes::R_TOP_END])) acc += (double)hes::top_term(rec[i], a, b);
    __syncthreads();
  }
  if (tid < hes::kTopEntries) {
    double *top = reinterpret_cast<double *>(base + J.o_top) + (long long)pair * (hes::kTop * hes::kTop);
    top[a * hes::kTop + b] = acc, top[b * hes::kTop + a] = acc;
  }
}

__global__ __launch_bounds__(1024) void hes_schur_kernel(const HesJob *jobs, const float *stage, float *base) {
  const HesJob &J = jobs[blockIdx.y];
  const int nf = J.n_frames, blk = blockIdx.x, tid = threadIdx.x;
  if (blk > nf * nf) return; // uniform over the workgroup
  __shared__ float jp[kSchurChunk][DSM_WINDOW_MAX_FRAMES][8]; // JpJdF of the point's active residual against each target
  __shared__ int act[kSchurChunk][DSM_WINDOW_MAX_FRAMES];
  __shared__ float pt[kHccChunk][hes::P_FLOATS]; // the first kSchurChunk rows in the (host, t1) workgroups
  const int *stage_i = reinterpret_cast<const int *>(stage);
  const float *prec = base + J.o_prec;
  double acc = 0.0;
  if (blk == nf * nf) { // acc_Hcc (lanes 0-15) and acc_bc (16-19): all points in ascending index
    for (int c0 = 0; c0 < J.n_pts; c0 += kHccChunk) {
      const int n = min(kHccChunk, J.n_pts - c0);
      for (int idx = tid; idx < n * hes::P_FLOATS; idx += blockDim.x) (&pt[0][0])[idx] = prec[(long long)hes::P_FLOATS * c0 + idx];
      __syncthreads();
      if (tid < 20)
        for (int i = 0; i < n; i++)
          if (__float_as_int(pt[i][hes::P_NACT])) acc += (double)(tid < 16 ? hes::term_Hcc(pt[i], tid >> 2, tid & 3) : hes::term_bc(pt[i], tid - 16));
      __syncthreads();
    }
    if (tid < 16) reinterpret_cast<double *>(base + J.o_Hcc)[tid] = acc;
    else if (tid < 20) reinterpret_cast<double *>(base + J.o_bc)[tid - 16] = acc;
    return;
  }
  const int h = blk / nf, t1 = blk - h * nf;
  const int t2 = tid >> 6, k = tid & 63;
  const int hs = stage_i[J.off_host_start + h], he = t1 == h ? hs : stage_i[J.off_host_start + h + 1]; // no residual has its host as target
  const int *slot = reinterpret_cast<const int *>(base + J.o_slot);
  // role: 0 idle, 1 acc_D[h][t1][t2][k >> 3][k & 7], 2 acc_E[h][t1][k >> 2][k & 3], 3 acc_EB[h][t1][k - 32]
  const int role = t2 >= nf ? 0 : t2 != h ? 1 : k < 32 ? 2 : k < 40 ? 3 : 0;
  for (int c0 = hs; c0 < he; c0 += kSchurChunk) {
    const int n = min(kSchurChunk, he - c0);
    for (int idx = tid; idx < n * nf * 8; idx += blockDim.x) {
      const int e = idx & 7, q = idx >> 3, i = q / nf, t = q - i * nf;
      const int r = slot[(long long)stage_i[J.off_host_pts + c0 + i] * nf + t];
      if (e == 0) act[i][t] = r >= 0;
      jp[i][t][e] = r >= 0 ? base[J.o_rec + (long long)hes::R_FLOATS * r + hes::R_JP + e] : 0.0f;
    }
    for (int idx = tid; idx < n * hes::P_FLOATS; idx += blockDim.x) {
      const int i = idx / hes::P_FLOATS, f = idx - i * hes::P_FLOATS;
      pt[i][f] = prec[(long long)hes::P_FLOATS * stage_i[J.off_host_pts + c0 + i] + f];
    }
    __syncthreads();
    if (role)
      for (int i = 0; i < n; i++) { // S3: ascending point index; a point has at most one residual against a target
        if (!act[i][t1]) continue;
        if (role == 1) {
          if (act[i][t2]) acc += (double)hes::term_D(pt[i], jp[i][t1], jp[i][t2], k >> 3, k & 7);
        } else if (role == 2) {
          acc += (double)hes::term_E(pt[i], jp[i][t1], k >> 2, k & 3);
        } else {
          acc += (double)hes::term_EB(pt[i], jp[i][t1], k - 32);
        }
      }
    __syncthreads();
  }
  if (t2 < nf) reinterpret_cast<double *>(base + J.o_D)[((long long)blk * nf + t2) * 64 + k] = role == 1 ? acc : 0.0;
  if (role == 2) reinterpret_cast<double *>(base + J.o_E)[(long long)blk * 32 + k] = acc;
  if (role == 3) reinterpret_cast<double *>(base + J.o_EB)[(long long)blk * 8 + k - 32] = acc;
}

} // namespace

extern "C" int dsm_window_hessian_batch(dsm_context *ctx, int n_jobs, const dsm_hessian_job *jobs, const dsm_linearize_params *params) {
  auto bad = [](const char *msg) { return invalid((std::string("dsm_window_hessian_batch: ") + msg).c_str()); };
  size_t res = 0;
  std::vector<const dsm_linearize_job *> lin;
  for (int j = 0; jobs && j < n_jobs; j++) lin.push_back(&jobs[j].lin);
  int rc = linearize_check_jobs("dsm_window_hessian_batch", ctx, n_jobs, jobs ? lin.data() : nullptr, params, &res);
  if (rc) return rc;
  for (int j = 0; j < n_jobs; j++)
    if (const char *e = hessian_job_error(jobs[j])) return bad(e);
  CallArena A;
  HesPlan P;
  for (int j = 0; j < n_jobs; j++) P.jobs.push_back(&jobs[j]);
  hessian_layout(P, A);
  if ((rc = A.bind(ctx))) return rc;
  hessian_stage(P, A);
  if ((rc = A.upload())) return rc;
  if ((rc = hessian_launch(ctx, P, A, *params))) return rc;
  DSM_HIP(hipGetLastError());
  if ((rc = A.fetch(A.out.used))) return rc;
  hessian_unpack(P, A, *params);
  return DSM_OK;
}

namespace dsm {

// staged [linearize job table | job table | per job: the linearisation's inputs, the index lists, the optional per-point inputs],
// device only [per job: rows (unless lin.J_out), records, slot table], read back [heads | per job: point results, accumulators |
// per job, as asked for: JpJdF, centre, projections, rows]; a lean plan keeps the point results and the accumulators of a job that
// asks for none of them in the device-only part
void hessian_layout(HesPlan &P, CallArena &A) {
  const int n_jobs = (int)P.jobs.size();
  auto job = [&P](int j) -> const dsm_hessian_job & { return *P.jobs[j]; };
  size_t words = 0;
  for (int j = 0; j < n_jobs; j++) {
    const dsm_hessian_job &H = job(j);
    const size_t nf = H.lin.n_frames, np = H.lin.n_pts, nr = H.lin.n_res;
    words += linearize_stage_words(H.lin) + (nf * nf + 1) + nr + (np + 1) + nr + (nf + 1) + np;
    words += np * ((H.prior != nullptr) + (H.delta != nullptr) + (H.hdd_lin != nullptr) + (H.bd_lin != nullptr) + 4 * (H.hcd_lin != nullptr));
  }
  P.o_lin = A.in.take(sizeof(LinJob) * n_jobs), P.o_hes = A.in.take(sizeof(HesJob) * n_jobs), P.o_stage = A.in.take(4 * words);
  std::vector<HesWhere> &at = P.at;
  at.assign(n_jobs, HesWhere());
  for (int j = 0; j < n_jobs; j++) {
    const size_t nf = job(j).lin.n_frames, np = job(j).lin.n_pts, nr = job(j).lin.n_res;
    HesWhere &w = at[j];
    w.rows_out = job(j).lin.J_out && nr;
    if (!w.rows_out) w.rows = A.work.take(4 * lin::J_FLOATS * nr);
    w.rec = A.work.take(4 * hes::R_FLOATS * nr), w.slot = A.work.take(4 * np * nf);
  }
  for (int j = 0; j < n_jobs; j++) at[j].head = A.out.take(4 * kLinHeadWords * (size_t)job(j).lin.n_res);
  for (int j = 0; j < n_jobs; j++) {
    const dsm_hessian_job &H = job(j);
    const size_t nf = H.lin.n_frames, n2 = nf * nf;
    HesWhere &w = at[j];
    const bool prec_out = !P.lean || H.hdd_acc || H.bd_acc || H.hcd_acc || H.hdi || H.bd_sum || H.idepth_hessian;
    const bool raw_out = !P.lean || H.acc_top || H.acc_D || H.acc_E || H.acc_EB || H.acc_Hcc || H.acc_bc;
    auto take = [&A](bool out, size_t bytes) {
      HesSpot s;
      s.out = out, s.at = (out ? A.out : A.work).take(bytes);
      return s;
    };
    w.prec = take(prec_out, 4 * hes::P_FLOATS * (size_t)H.lin.n_pts);
    w.top = take(raw_out, 8 * n2 * 169), w.D = take(raw_out, 8 * n2 * nf * 64), w.E = take(raw_out, 8 * n2 * 32), w.EB = take(raw_out, 8 * n2 * 8);
    w.Hcc = take(raw_out, 8 * 16), w.bc = take(raw_out, 8 * 4);
  }
  for (int j = 0; j < n_jobs; j++) {
    const dsm_linearize_job &L = job(j).lin;
    const size_t n = L.n_res;
    HesWhere &w = at[j];
    if (job(j).JpJdF && n) w.jp = (long long)A.out.take(4 * 8 * n);
    if (L.center_projected_to && n) w.cpt = (long long)A.out.take(4 * 3 * n);
    if (L.projected_to && n) w.proj = (long long)A.out.take(4 * 16 * n);
    if (w.rows_out) w.J = (long long)A.out.take(4 * lin::J_FLOATS * n);
  }
}

void hessian_stage(HesPlan &P, CallArena &A) {
  const int n_jobs = (int)P.jobs.size();
  // the kernels count 4-byte words from the start of the device-only part; the read-back part follows it
  const long long out0 = P.out0 = (long long)(A.work.used / 4);
  auto from_out = [out0](long long bytes) { return bytes < 0 ? -1ll : out0 + bytes / 4; };
  LinJob *hl = A.host_in<LinJob>(P.o_lin);
  HesJob *hh = A.host_in<HesJob>(P.o_hes);
  WordPacker W{A.host_in<float>(P.o_stage)};
  int max_res = 0, max_pts = 0, max_nf = 1;
  P.view.assign(n_jobs, HesView());
  for (int j = 0; j < n_jobs; j++) {
    const dsm_hessian_job &H = *P.jobs[j];
    const dsm_linearize_job &L = H.lin;
    const int nf = L.n_frames, np = L.n_pts, nr = L.n_res;
    const HesWhere &w = P.at[j];
    LinJob &D = hl[j];
    memset(&D, 0, sizeof D);
    D.o_head = from_out((long long)w.head), D.o_cpt = from_out(w.cpt), D.o_proj = from_out(w.proj);
    D.o_J = w.rows_out ? from_out(w.J) : (long long)(w.rows / 4);
    linearize_stage(L, D, W);
    HesJob &G = hh[j];
    memset(&G, 0, sizeof G);
    G.n_frames = nf, G.n_pts = np, G.n_res = nr, G.shift = H.shift_prior_to_zero != 0;
    G.o_rows = D.o_J, G.o_rec = (long long)(w.rec / 4), G.o_slot = (long long)(w.slot / 4);
    G.o_prec = w.prec.word(out0), G.o_jp = from_out(w.jp), G.o_top = w.top.word(out0), G.o_D = w.D.word(out0);
    G.o_E = w.E.word(out0), G.o_EB = w.EB.word(out0), G.o_Hcc = w.Hcc.word(out0), G.o_bc = w.bc.word(out0);
    // the two index lists, one counting pass each: the residuals of every [host][target] pair and of every point in ascending index,
    // the points grouped by host in ascending index
    int *pair_start = (int *)W.reserve(&G.off_pair_start, (size_t)nf * nf + 1), *pair_list = (int *)W.reserve(&G.off_pair_list, nr);
    int *pt_start = (int *)W.reserve(&G.off_pt_start, (size_t)np + 1), *pt_list = (int *)W.reserve(&G.off_pt_list, nr);
    int *host_start = (int *)W.reserve(&G.off_host_start, (size_t)nf + 1), *host_pts = (int *)W.reserve(&G.off_host_pts, np);
    std::fill(pair_start, pair_start + nf * nf + 1, 0), std::fill(pt_start, pt_start + np + 1, 0), std::fill(host_start, host_start + nf + 1, 0);
    for (int r = 0; r < nr; r++) pair_start[L.host[L.point[r]] * nf + L.target[r] + 1]++, pt_start[L.point[r] + 1]++;
    for (int p = 0; p < np; p++) host_start[L.host[p] + 1]++;
    for (int i = 0; i < nf * nf; i++) pair_start[i + 1] += pair_start[i];
    for (int p = 0; p < np; p++) pt_start[p + 1] += pt_start[p];
    for (int f = 0; f < nf; f++) host_start[f + 1] += host_start[f];
    {
      std::vector<int> pa(pair_start, pair_start + nf * nf), pp(pt_start, pt_start + np), ph(host_start, host_start + nf);
      for (int r = 0; r < nr; r++) pair_list[pa[L.host[L.point[r]] * nf + L.target[r]]++] = r, pt_list[pp[L.point[r]]++] = r;
      for (int p = 0; p < np; p++) host_pts[ph[L.host[p]]++] = p;
    }
    G.off_prior = G.off_delta = G.off_hdd_lin = G.off_bd_lin = G.off_hcd_lin = -1;
    if (H.prior) W.put(&G.off_prior, H.prior, np);
    if (H.delta) W.put(&G.off_delta, H.delta, np);
    if (H.hdd_lin) W.put(&G.off_hdd_lin, H.hdd_lin, np);
    if (H.bd_lin) W.put(&G.off_bd_lin, H.bd_lin, np);
    if (H.hcd_lin) W.put(&G.off_hcd_lin, H.hcd_lin, 4 * (size_t)np);
    max_res = std::max(max_res, nr), max_pts = std::max(max_pts, np), max_nf = std::max(max_nf, nf);
    HesView &V = P.view[j];
    V.n_frames = nf, V.n_pts = np, V.n_res = nr;
    V.off_pt_start = G.off_pt_start, V.off_pt_list = G.off_pt_list, V.off_target = D.off_target, V.off_host = D.off_host;
    V.o_rec = G.o_rec, V.o_prec = G.o_prec, V.o_top = G.o_top, V.o_D = G.o_D, V.o_E = G.o_E, V.o_EB = G.o_EB, V.o_Hcc = G.o_Hcc, V.o_bc = G.o_bc;
  }
  P.max_res = max_res, P.max_pts = max_pts, P.max_nf = max_nf;
  P.dev_stage = A.dev_in<const float>(P.o_stage), P.dev_base = A.dev_work<float>(0);
}

int hessian_launch(dsm_context *ctx, HesPlan &P, CallArena &A, const dsm_linearize_params &params) {
  if (int rc = hessian_launch_linearize(ctx, P, A, params)) return rc;
  return hessian_launch_accumulate(ctx, P, A);
}

int hessian_launch_linearize(dsm_context *ctx, HesPlan &P, CallArena &A, const dsm_linearize_params &params) {
  if (!P.max_res) return DSM_OK;
  const dsm_window *win = P.jobs[0]->lin.window;
  return linearize_launch(ctx, (int)P.jobs.size(), P.max_res, A.dev_in<const LinJob>(P.o_lin), P.dev_stage, P.dev_base, win->w, win->h, params);
}

int hessian_launch_accumulate(dsm_context *ctx, HesPlan &P, CallArena &A) {
  const int n_jobs = (int)P.jobs.size(), max_res = P.max_res, max_pts = P.max_pts, max_nf = P.max_nf;
  const LinJob *dl = A.dev_in<const LinJob>(P.o_lin);
  const HesJob *dh = A.dev_in<const HesJob>(P.o_hes);
  const float *ds = P.dev_stage;
  float *base = P.dev_base;
  if (max_res) {
    hipLaunchKernelGGL(hes_residual_kernel, dim3((max_res + kResBlock - 1) / kResBlock, n_jobs), dim3(kResBlock), 0, ctx->stream, dl, dh, ds, base);
  }
  if (max_pts)
    hipLaunchKernelGGL(hes_point_kernel, dim3((max_pts + kPtBlock - 1) / kPtBlock, n_jobs), dim3(kPtBlock), 0, ctx->stream, dl, dh, ds, base);
  hipLaunchKernelGGL(hes_pair_kernel, dim3(max_nf * max_nf, n_jobs), dim3(kPairBlock), 0, ctx->stream, dh, ds, base);
  hipLaunchKernelGGL(hes_schur_kernel, dim3(max_nf * max_nf + 1, n_jobs), dim3(64 * max_nf), 0, ctx->stream, dh, ds, base);
  return DSM_OK;
}

void hessian_unpack(const HesPlan &P, const CallArena &A, const dsm_linearize_params &params) {
  const int n_jobs = (int)P.jobs.size();
  const unsigned char *ho = A.host_out<unsigned char>(0);
  for (int j = 0; j < n_jobs; j++) {
    const dsm_hessian_job &H = *P.jobs[j];
    const dsm_linearize_job &L = H.lin;
    const HesWhere &w = P.at[j];
    const float *hf = reinterpret_cast<const float *>(ho);
    linearize_unpack(L, hf, (long long)(w.head / 4), w.cpt < 0 ? -1 : w.cpt / 4, w.proj < 0 ? -1 : w.proj / 4, w.J < 0 ? -1 : w.J / 4);
    for (int r = 0; r < L.n_res; r++) {
      const bool active = L.state_in[r] != DSM_RES_OOB && L.new_state[r] == DSM_RES_IN; // A0
      if (H.active) H.active[r] = active;
      if (active && w.jp >= 0) memcpy(H.JpJdF + (size_t)8 * r, ho + w.jp + (size_t)32 * r, 32);
    }
    const float *prec = reinterpret_cast<const float *>(ho + w.prec.at);
    for (int p = 0; w.prec.out && p < L.n_pts; p++) {
      const float *P = prec + (size_t)hes::P_FLOATS * p;
      if (H.hdd_acc) H.hdd_acc[p] = P[hes::P_HDD];
      if (H.bd_acc) H.bd_acc[p] = P[hes::P_BD];
      if (H.hcd_acc) memcpy(H.hcd_acc + 4 * p, P + hes::P_HCD, 16);
      if (H.hdi) H.hdi[p] = P[hes::P_HDI];
      if (H.bd_sum) H.bd_sum[p] = P[hes::P_BDSUM];
      if (H.idepth_hessian) H.idepth_hessian[p] = P[hes::P_IDH];
    }
    auto raw = [ho](const HesSpot &s) { return reinterpret_cast<const double *>(ho + s.at); };
    if (!P.lean) hessian_stitch(H, raw(w.top), raw(w.D), raw(w.E), raw(w.EB), raw(w.Hcc), raw(w.bc));
    else if (w.top.out) hessian_copy_raw(H, raw(w.top), raw(w.D), raw(w.E), raw(w.EB), raw(w.Hcc), raw(w.bc));
    linearize_job_summary(L, params); // B1, B2
  }
}

} // namespace dsm
