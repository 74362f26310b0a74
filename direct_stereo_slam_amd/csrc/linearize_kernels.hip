// linearize_kernels.hip -- FrontEnd::linearizeAll (dso_helpers/FrontEndOptimize.cpp:121-179) on the device: PointFrameResidual::linearize
// for every active residual of the windows of many sequences in one call.  Semantics: L1-L8, B1-B4 of DESIGN.md section 16.
//
// One dsm_linearize_residuals_batch = one staged copy, ONE launch, one read-back:
//   linearize_kernel  one lane per (residual, pattern pixel): lane = 8 * k + pixel, eight residuals per wave, four waves per workgroup,
//                     blockIdx.y = job.  The twelve texels of all 64 pixels of a wave are in flight at once.  The centre projection and
//                     the geometric Jacobians (L2, L3) are computed by all eight lanes of a residual: the lanes are there anyway, and
//                     every lane then holds the 22 floats it takes its share of the row from.
// Bit parity with the reference's sequential float sums: a lane computes its pixel's twelve TERMS (lin::pixel, shared with the host
// form); each sum is then a chain through the eight lanes of the residual in pattern order -- seven row_shr:1 steps, at step s only
// lane s of the group adds its left neighbour's prefix -- which begins with +0.0f + x0 as the reference's accumulator does.  One
// ballot gives the failing pixels; a residual is OOB iff its byte of the ballot is non-zero, and nothing of an OOB residual but its
// state and energy leaves the kernel.
// A row (74 floats) is written by the eight lanes of its residual, lane i the floats 8 j + i: every store instruction of the wave
// writes eight runs of 32 bytes, and the per-residual floats are picked from registers by compares, not indexed (no scratch).
// The kernel waits for no other workgroup, has no barrier and uses no LDS; the energy sum and the order statistic of B2 are formed on the
// host from the read-back (linearize_job_summary), so that no cross-workgroup reduction has an order to pin.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "linearize_launch.hpp"

using namespace dsm;

namespace {

constexpr int kWavesPerBlock = 4;
constexpr int kResPerBlock = 8 * kWavesPerBlock;
constexpr int kHeadWords = kLinHeadWords;
constexpr size_t kMaxResiduals = 1u << 24;

template <int CTRL>
__device__ __forceinline__ float dpp(float v) { // lanes without a source get 0; they never use it
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}

// the sum of x over the eight lanes of a group as the sequential ((((+0 + x0) + x1) + ...) + x7), in every lane of the group
__device__ __forceinline__ float chain8(float x, int idx, int last_lane) {
  float p = 0.0f + x;
#pragma unroll
  for (int s = 1; s < 8; s++) {
    const float left = dpp<0x111>(p); // row_shr:1 -- a group of eight never crosses a row of sixteen
    if (idx == s) p = left + x;
  }
  return __shfl(p, last_lane);
}

// a_i for i in [0, 8), by compares.  The values come as scalars: picked from an array, the compiler turns the compares back into an
// index, and the array into memory.
__device__ __forceinline__ float pick8(int i, float a0, float a1, float a2, float a3, float a4, float a5, float a6, float a7) {
  const float lo = i & 2 ? (i & 1 ? a3 : a2) : (i & 1 ? a1 : a0), hi = i & 2 ? (i & 1 ? a7 : a6) : (i & 1 ? a5 : a4);
  return i & 4 ? hi : lo;
}

__global__ __launch_bounds__(64 * kWavesPerBlock) void linearize_kernel(const LinJob *jobs, const float *stage, float *out, int w, int h,
                                                                        lin::Settings S, int zero_a, int zero_b) {
  const LinJob &J = jobs[blockIdx.y];
  const int lane = threadIdx.x & 63, idx = lane & 7;
  const int r = blockIdx.x * kResPerBlock + (int)(threadIdx.x >> 6) * 8 + (lane >> 3);
  if (r - (lane >> 3) >= J.n_res) return; // wave-uniform; the kernel has no barrier
  const bool act = r < J.n_res;
  const int rr = act ? r : J.n_res - 1; // the lanes past the end read the last residual's inputs and write nothing
  const int *stage_i = reinterpret_cast<const int *>(stage);
  const int p = stage_i[J.off_point + rr], tgt = stage_i[J.off_target + rr], flags = stage_i[J.off_flags + rr];
  const int hst = stage_i[J.off_host + p], pair = hst * J.n_frames + tgt;
  const int state_in = flags & 0xff;
  const lin::Cam C{J.fx, J.fy, J.cx, J.cy, J.fxi, J.fyi, w, h};
  float R0[9], t0[3], M[9], Kt[3], aff[2];
#pragma unroll
  for (int k = 0; k < 9; k++) R0[k] = stage[J.off_R0 + 9 * pair + k], M[k] = stage[J.off_M + 9 * pair + k];
#pragma unroll
  for (int k = 0; k < 3; k++) t0[k] = stage[J.off_t0 + 3 * pair + k], Kt[k] = stage[J.off_Kt + 3 * pair + k];
  aff[0] = stage[J.off_aff + 2 * pair], aff[1] = stage[J.off_aff + 2 * pair + 1];
  const float b0 = stage[J.off_b0 + pair];
  const float u = stage[J.off_u + p], v = stage[J.off_v + p], id = stage[J.off_id + p], idz = stage[J.off_idz + p];
  const float color = stage[J.off_color + 8 * p + idx], wt = stage[J.off_wt + 8 * p + idx];
  // pt::pattern(idx) without its tables, which an index that is not a constant would put into memory: dx + 2, dy + 2 as nibbles
  const int dx = (int)((0x21420312u >> (4 * idx)) & 15u) - 2, dy = (int)((0x43222110u >> (4 * idx)) & 15u) - 2;

  lin::Centre c;
  const bool live = act && state_in != lin::RES_OOB && lin::centre(C, R0, t0, u, v, idz, c); // L1, L2: equal in the eight lanes of a residual
  lin::Pixel P;
  bool ok = false;
  if (live) ok = lin::pixel(C, J.plane[tgt], M, Kt, aff, b0, u, v, dx, dy, id, color, wt, S, P); // L4, L5
  const unsigned long long failed = __ballot(live && !ok);
  const bool oob = !live || ((failed >> (lane & 56)) & 0xffull) != 0;
  float sum[lin::N_SUMS];
#pragma unroll
  for (int k = 0; k < lin::N_SUMS; k++) sum[k] = chain8(ok ? P.T[k] : 0.0f, idx, lane | 7); // L6
  int state = lin::RES_OOB;
  float E = stage[J.off_ein + rr], with_outlier = -1.0f;
  if (!oob) {
    with_outlier = E = sum[lin::S_E];
    state = lin::verdict(E, sum[lin::S_WJI2], stage[J.off_eth + hst], stage[J.off_eth + tgt]); // L7
  }
  if (!act) return;
  if (idx == 0) {
    const bool keep = J.fix && state_in != lin::RES_OOB && state == lin::RES_IN; // B3
    const float rel = keep && (flags >> 8) ? lin::rel_baseline(M, Kt, u, v, id) : 0.0f;
    float4 head;
    head.x = __int_as_float(state | (keep ? 256 : 0)), head.y = E, head.z = with_outlier, head.w = rel;
    *reinterpret_cast<float4 *>(out + J.o_head + (long long)kHeadWords * r) = head;
  }
  if (oob) return; // L8: nothing else of an OOB residual is written
  if (J.o_cpt >= 0 && idx < 3) {
    out[J.o_cpt + 3ll * r + idx] = idx == 0 ? c.Ku : idx == 1 ? c.Kv : c.new_idepth;
  }
  if (J.o_proj >= 0) *reinterpret_cast<float2 *>(out + J.o_proj + 16ll * r + 2 * idx) = make_float2(P.Ku, P.Kv);
  if (J.o_J >= 0) {
    float G[lin::kGeoFloats];
    lin::geometric(C, R0, t0, c, S, G); // L3
    const float sxy = sum[lin::S_XY], sab = sum[lin::S_AB];
    float *row = out + J.o_J + (long long)lin::J_FLOATS * r + idx;
    row[lin::J_RESF] = P.resF;
    row[lin::J_PDXI] = pick8(idx, G[0], G[1], G[2], G[3], G[4], G[5], G[6], G[7]);
    row[lin::J_PDXI + 8] = pick8(idx, G[8], G[9], G[10], G[11], G[12], G[13], G[14], G[15]);
    if (idx < 6) row[lin::J_PDXI + 16] = pick8(idx, G[16], G[17], G[18], G[19], G[20], G[21], 0.0f, 0.0f);
    row[lin::J_IDX] = P.gx;
    row[lin::J_IDX + 8] = P.gy;
    row[lin::J_ABF] = zero_a ? 0.0f : P.ja;
    row[lin::J_ABF + 8] = zero_b ? 0.0f : P.jb;
    row[lin::J_IDX2] = pick8(idx, sum[lin::S_XX], sxy, sxy, sum[lin::S_YY], sum[lin::S_AX], sum[lin::S_AY], sum[lin::S_BX], sum[lin::S_BY]);
    if (idx < 4) row[lin::J_IDX2 + 8] = pick8(idx, sum[lin::S_AA], sab, sab, sum[lin::S_BB], 0.0f, 0.0f, 0.0f, 0.0f);
  }
}

} // namespace

namespace dsm {

int linearize_check_jobs(const char *call, dsm_context *ctx, int n_jobs, const dsm_linearize_job *const *jobs, const dsm_linearize_params *params,
                         size_t *res_out) {
  auto bad = [call](const char *msg) { return invalid((std::string(call) + ": " + msg).c_str()); };
  if (!ctx || n_jobs < 1 || !jobs) return bad("bad argument");
  if (const char *e = linearize_params_error(params)) return bad(e);
  size_t res = 0;
  for (int j = 0; j < n_jobs; j++) {
    const dsm_linearize_job &J = *jobs[j];
    if (!J.window || J.window->ctx != ctx) return bad("no window, or a window of another context");
    if (J.window->w != jobs[0]->window->w || J.window->h != jobs[0]->window->h) return bad("one geometry per call");
    if (const char *e = linearize_job_error(J)) return bad(e);
    for (int f = 0; f < J.n_frames; f++)
      if (J.window->find(J.frame_ids[f]) < 0) return bad("a frame id that is not in the window");
    res += (size_t)J.n_res;
  }
  if (res > kMaxResiduals) return bad("too many residuals in one call");
  *res_out = res;
  return DSM_OK;
}

// the six precalc tables, frame_energy_th, the point arrays and the residual arrays
size_t linearize_stage_words(const dsm_linearize_job &J) {
  const size_t nf = J.n_frames;
  return 27 * nf * nf + nf + 21 * (size_t)J.n_pts + 4 * (size_t)J.n_res;
}

void linearize_stage(const dsm_linearize_job &J, LinJob &D, WordPacker &W) {
  const size_t nf = J.n_frames, n = J.n_pts, nr = J.n_res;
  for (size_t f = 0; f < nf; f++) D.plane[f] = J.window->plane(J.window->find(J.frame_ids[f]));
  D.fx = J.cam[0], D.fy = J.cam[1], D.cx = J.cam[2], D.cy = J.cam[3], D.fxi = J.cam_inv[0], D.fyi = J.cam_inv[1];
  D.n_frames = J.n_frames, D.n_res = J.n_res, D.fix = J.fix_linearization != 0;
  W.put(&D.off_R0, J.pre_RTll_0, 9 * nf * nf);
  W.put(&D.off_t0, J.pre_tTll_0, 3 * nf * nf);
  W.put(&D.off_M, J.pre_KRKiTll, 9 * nf * nf);
  W.put(&D.off_Kt, J.pre_KtTll, 3 * nf * nf);
  W.put(&D.off_aff, J.pre_aff_mode, 2 * nf * nf);
  W.put(&D.off_b0, J.pre_b0_mode, nf * nf);
  W.put(&D.off_eth, J.frame_energy_th, nf);
  W.put(&D.off_host, J.host, n);
  W.put(&D.off_u, J.u, n);
  W.put(&D.off_v, J.v, n);
  W.put(&D.off_id, J.idepth_scaled, n);
  W.put(&D.off_idz, J.idepth_zero_scaled, n);
  W.put(&D.off_color, J.color, 8 * n);
  W.put(&D.off_wt, J.weights, 8 * n);
  W.put(&D.off_point, J.point, nr);
  W.put(&D.off_target, J.target, nr);
  W.put(&D.off_ein, J.energy_in, nr);
  int *flags = (int *)W.reserve(&D.off_flags, nr);
  for (size_t r = 0; r < nr; r++) flags[r] = J.state_in[r] | (J.fix_linearization && J.is_new[r] ? 256 : 0);
}

int linearize_launch(dsm_context *ctx, int n_jobs, int max_res, const LinJob *dev_jobs, const float *dev_stage, float *out, int w, int h,
                     const dsm_linearize_params &params) {
  const lin::Settings S{params.huber_th, params.outlier_th_sum_component, params.scale_idepth, params.scale_f, params.scale_c};
  hipLaunchKernelGGL(linearize_kernel, dim3((max_res + kResPerBlock - 1) / kResPerBlock, n_jobs), dim3(64 * kWavesPerBlock), 0, ctx->stream,
                     dev_jobs, dev_stage, out, w, h, S, params.zero_jab_a != 0, params.zero_jab_b != 0);
  DSM_HIP(hipGetLastError());
  return DSM_OK;
}

void linearize_unpack(const dsm_linearize_job &J, const float *ho, long long o_head, long long o_cpt, long long o_proj, long long o_J) {
  for (int r = 0; r < J.n_res; r++) {
    const float *q = ho + o_head + (size_t)kHeadWords * r;
    unsigned word;
    memcpy(&word, q, 4);
    const int state = word & 0xff;
    J.new_state[r] = (unsigned char)state, J.new_energy[r] = q[1], J.new_energy_with_outlier[r] = q[2];
    if (J.fix_linearization) {
      if (J.keep) J.keep[r] = (unsigned char)(word >> 8);
      if (J.rel_bs) J.rel_bs[r] = q[3];
    }
    if (state == lin::RES_OOB) continue; // L8
    if (o_cpt >= 0) memcpy(J.center_projected_to + (size_t)3 * r, ho + o_cpt + (size_t)3 * r, 12);
    if (o_proj >= 0) memcpy(J.projected_to + (size_t)16 * r, ho + o_proj + (size_t)16 * r, 64);
    if (o_J >= 0) memcpy(J.J_out + (size_t)lin::J_FLOATS * r, ho + o_J + (size_t)lin::J_FLOATS * r, 4 * lin::J_FLOATS);
  }
}

} // namespace dsm

extern "C" int dsm_linearize_residuals_batch(dsm_context *ctx, int n_jobs, const dsm_linearize_job *jobs, const dsm_linearize_params *params) {
  size_t res = 0;
  std::vector<const dsm_linearize_job *> list;
  for (int j = 0; jobs && j < n_jobs; j++) list.push_back(jobs + j);
  int rc = linearize_check_jobs("dsm_linearize_residuals_batch", ctx, n_jobs, jobs ? list.data() : nullptr, params, &res);
  if (rc) return rc;
  if (res) {
    // staged [job table | the six precalc tables, frame_energy_th, the point arrays and the residual arrays of every job], read back
    // [head of every job | per job, as asked for: centre, projections, rows]
    size_t words = 0;
    for (int j = 0; j < n_jobs; j++) words += linearize_stage_words(jobs[j]);
    CallArena A;
    const size_t o_jobs = A.in.take(sizeof(LinJob) * n_jobs), o_stage = A.in.take(4 * words);
    std::vector<long long> o_head(n_jobs), o_cpt(n_jobs, -1), o_proj(n_jobs, -1), o_J(n_jobs, -1);
    for (int j = 0; j < n_jobs; j++) o_head[j] = (long long)(A.out.take(4 * kHeadWords * (size_t)jobs[j].n_res) / 4);
    for (int j = 0; j < n_jobs; j++) {
      const size_t n = jobs[j].n_res;
      if (jobs[j].center_projected_to && n) o_cpt[j] = (long long)(A.out.take(4 * 3 * n) / 4);
      if (jobs[j].projected_to && n) o_proj[j] = (long long)(A.out.take(4 * 16 * n) / 4);
      if (jobs[j].J_out && n) o_J[j] = (long long)(A.out.take(4 * lin::J_FLOATS * n) / 4);
    }
    if ((rc = A.bind(ctx))) return rc;
    LinJob *hj = A.host_in<LinJob>(o_jobs);
    WordPacker W{A.host_in<float>(o_stage)};
    int max_res = 0;
    for (int j = 0; j < n_jobs; j++) {
      LinJob &D = hj[j];
      memset(&D, 0, sizeof D);
      D.o_head = o_head[j], D.o_cpt = o_cpt[j], D.o_proj = o_proj[j], D.o_J = o_J[j];
      linearize_stage(jobs[j], D, W);
      max_res = std::max(max_res, jobs[j].n_res);
    }
    if ((rc = A.upload())) return rc;
    if ((rc = linearize_launch(ctx, n_jobs, max_res, A.dev_in<const LinJob>(o_jobs), A.dev_in<const float>(o_stage), A.dev_out<float>(0),
                               jobs[0].window->w, jobs[0].window->h, *params)))
      return rc;
    if ((rc = A.fetch(A.out.used))) return rc;
    const float *ho = A.host_out<float>(0);
    for (int j = 0; j < n_jobs; j++) linearize_unpack(jobs[j], ho, o_head[j], o_cpt[j], o_proj[j], o_J[j]);
  }
  for (int j = 0; j < n_jobs; j++) linearize_job_summary(jobs[j], *params); // B1, B2
  return DSM_OK;
}
