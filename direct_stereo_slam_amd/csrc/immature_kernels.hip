// immature_kernels.hip -- the second half of FrontEnd::activatePointsMT (FrontEnd.cpp:458-468) on the device:
// FrontEnd::optimizeImmaturePoint (dso_helpers/FrontEndOptPoint.cpp:35-138) for the selected points of the windows of many sequences
// in one call, and dsm_window, the level-0 intensity planes of a window's keyframes.  Semantics: M1-M8, U1-U9 of DESIGN.md section 13.
//
// One dsm_optimize_immature_points_batch = one staged copy, ONE launch, one read-back:
//   immature_kernel  one wave per point (four points per workgroup, blockIdx.y = job), one lane per (residual, pattern pixel):
//                    lane = 8 * residual + pixel, so the 8 residuals of a 9-frame window fill the wave and the twelve texels of every
//                    pixel of an evaluation are in flight at once.  The first linearisation and the up to gn_iterations trial
//                    evaluations are a loop inside the wave; its control flow is wave-uniform.
// Bit parity with the reference's sequential float sums: a lane computes its pixel's three TERMS (imm::tap, shared with the host form);
// the wave then finds the first failing pixel of every residual (one ballot) and adds the terms that count in the reference's order --
// Hdd and bd as one chain over the lanes of the surviving pixels (residual by residual, pixel by pixel; the terms in front of a failing
// pixel count, U5), the energy as one chain of eight per residual and one chain over the residuals.  The operands come from
// v_readlane (the lane is wave-uniform), so every lane holds the same sums.
// The kernel waits for no other workgroup and uses no LDS; its loops are bounded by 64, 8, n_frames and gn_iterations.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "call_arena.hpp"
#include "immature_math.hpp"

using namespace dsm;

namespace {

constexpr int kWavesPerBlock = 4;
constexpr int kOutWords = 8; // per point: idepth, Hdd, bd, energy, status | iterations << 8, three words of residual states
constexpr size_t kMaxPoints = 1u << 24;

struct ImJob {
  const float *plane[DSM_IMMATURE_MAX_FRAMES]; // level-0 planes in frame_ids order
  float fx, fy, cx, cy, fxi, fyi;
  int n_frames, n_pts, min_obs;
  int off_R, off_t, off_aff, off_host, off_u, off_v, off_idmin, off_idmax, off_eth, off_color, off_wt; // 4-byte words into the staged inputs
  int out_off;                                                                                          // first point of the job in the output
};

__device__ __forceinline__ float lane_value(float x, int lane) { // x of a wave-uniform lane
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), __builtin_amdgcn_readfirstlane(lane)));
}
__device__ __forceinline__ int lane_value(int x, int lane) { return __builtin_amdgcn_readlane(x, __builtin_amdgcn_readfirstlane(lane)); }
__device__ __forceinline__ float uniform(float x) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x))); }

// what a lane keeps of its residual (the eight lanes of a residual hold equal copies): ImmaturePointTemporaryResidual
struct LaneRes {
  int state, new_state;
  float energy, new_energy;
};

// what a lane needs for its pattern pixel: the job's camera, its residual's target plane and precalc row, the point
struct PointLane {
  imm::Cam C;
  const float *I; // the target's plane
  float R[9], t[3], aff[2];
  float u, v, color, wt, energy_th, huber;
  int dx, dy, lane, nres;
  bool act; // the lane has a residual
};

// One pass over the residuals (:56-58 / :86-88): every ImmaturePoint::linearizeResidual of the point at `idepth`.  Returns the sum of
// the returned energies; Hdd / bd: the accumulators after the last residual.  All three are equal in every lane.
__device__ __forceinline__ float evaluate(const PointLane &P, LaneRes &res, float slack, float idepth, float &Hdd, float &bd) {
  const bool live = P.act && res.state != imm::RES_OOB; // U1
  float tE = 0.f, tH = 0.f, tb = 0.f;
  bool ok = false;
  if (live) ok = imm::tap(P.C, P.I, P.R, P.t, P.aff, P.u, P.v, P.dx, P.dy, idepth, P.color, P.wt, P.huber, tE, tH, tb);
  const unsigned long long failed = __ballot(live && !ok);
  const unsigned mine = (unsigned)(failed >> (P.lane & 56)) & 0xffu;          // the failing pixels of this lane's residual
  const int first = mine ? __ffs((int)mine) - 1 : 8;                          // U4 / U6: the first of them
  unsigned long long counted = __ballot(live && (P.lane & 7) < first);        // U5: the terms that reach Hdd / bd
  float H = 0.f, b = 0.f;
  while (counted) { // in lane order = residual order, pattern order
    const int l = __ffsll((long long)counted) - 1;
    H += lane_value(tH, l);
    b += lane_value(tb, l);
    counted &= counted - 1;
  }
  float energyLeft = 0.f;
  const int base = P.lane & 56;
#pragma unroll
  for (int k = 0; k < 8; k++) energyLeft += __shfl(tE, base + k);
  float ret;
  if (!live || first < 8) {
    if (P.act) res.new_state = imm::RES_OOB;
    ret = res.energy;
  } else {
    const float lim = P.energy_th * slack; // U9
    if (energyLeft > lim) {
      energyLeft = lim;
      res.new_state = imm::RES_OUTLIER;
    } else {
      res.new_state = imm::RES_IN;
    }
    res.new_energy = energyLeft;
    ret = energyLeft;
  }
  float E = 0.f;
  for (int r = 0; r < P.nres; r++) E += lane_value(ret, 8 * r);
  Hdd = H, bd = b;
  return E;
}

__global__ __launch_bounds__(64 * kWavesPerBlock) void immature_kernel(const ImJob *jobs, const float *stage, unsigned *out, int w, int h,
                                                                       float huber, float min_h, int gn_its) {
  const ImJob &J = jobs[blockIdx.y];
  const int pt = blockIdx.x * kWavesPerBlock + (int)(threadIdx.x >> 6);
  if (pt >= J.n_pts) return; // wave-uniform; the kernel has no barrier
  const int lane = threadIdx.x & 63, nf = J.n_frames;
  const int *stage_i = reinterpret_cast<const int *>(stage);
  const int host = stage_i[J.off_host + pt];
  PointLane P;
  P.C = imm::Cam{J.fx, J.fy, J.cx, J.cy, J.fxi, J.fyi, w, h};
  P.lane = lane, P.nres = nf - 1, P.huber = huber;
  P.act = (lane >> 3) < P.nres;
  const int r = P.act ? (lane >> 3) : 0;
  const int tgt = P.nres > 0 ? r + (r >= host ? 1 : 0) : 0; // the residuals skip the host frame (:38-46)
  const int pair = host * nf + tgt;
  P.I = J.plane[tgt];
#pragma unroll
  for (int k = 0; k < 9; k++) P.R[k] = stage[J.off_R + 9 * pair + k];
#pragma unroll
  for (int k = 0; k < 3; k++) P.t[k] = stage[J.off_t + 3 * pair + k];
  P.aff[0] = stage[J.off_aff + 2 * pair], P.aff[1] = stage[J.off_aff + 2 * pair + 1];
  P.u = stage[J.off_u + pt], P.v = stage[J.off_v + pt], P.energy_th = stage[J.off_eth + pt];
  P.color = stage[J.off_color + 8 * pt + (lane & 7)], P.wt = stage[J.off_wt + 8 * pt + (lane & 7)];
  pt::pattern(lane & 7, P.dx, P.dy);

  LaneRes res{imm::RES_IN, imm::RES_OUTLIER, 0.f, 0.f};
  float Hdd = 0.f, bd = 0.f;
  const float start = uniform(imm::lm_start(stage[J.off_idmin + pt], stage[J.off_idmax + pt])); // M1
  const float energy = uniform(evaluate(P, res, 1000.f, start, Hdd, bd));                       // M2
  res.state = res.new_state, res.energy = res.new_energy;
  imm::LM lm = imm::lm_begin(start, energy, uniform(Hdd), uniform(bd), min_h);
  while (!lm.done && lm.iterations < gn_its) {
    const float newEnergy = uniform(evaluate(P, res, 1.f, imm::lm_propose(lm), Hdd, bd));
    if (imm::lm_trial(lm, newEnergy, uniform(Hdd), uniform(bd), min_h)) res.state = res.new_state, res.energy = res.new_energy;
  }
  imm::lm_finish(lm, __popcll(__ballot(P.act && (lane & 7) == 0 && res.state == imm::RES_IN)), J.min_obs);
  unsigned st[3] = {0u, 0u, 0u};
  for (int f = 0; f < nf; f++) {
    const int rr = f < host ? f : f - 1;
    const unsigned s = f == host ? (unsigned)DSM_RES_HOST : (unsigned)lane_value(res.state, 8 * (rr < 0 ? 0 : rr));
    st[f >> 2] |= s << (8 * (f & 3));
  }
  unsigned word;
  switch (lane) {
  case 0: word = __float_as_uint(lm.idepth); break;
  case 1: word = __float_as_uint(lm.Hdd); break;
  case 2: word = __float_as_uint(lm.bd); break;
  case 3: word = __float_as_uint(lm.energy); break;
  case 4: word = (unsigned)lm.status | ((unsigned)lm.iterations << 8); break;
  case 5: word = st[0]; break;
  case 6: word = st[1]; break;
  default: word = st[2]; break;
  }
  if (lane < kOutWords) out[(size_t)(J.out_off + pt) * kOutWords + lane] = word;
}

// all-or-nothing validation of a batch: nothing is enqueued before every job has passed
int check_jobs(dsm_context *ctx, int n_jobs, const dsm_immature_job *jobs, float huber_th, float min_idepth_h_act, int gn_iterations,
               size_t *pts_out) {
  auto bad = [](const char *msg) { return invalid((std::string("dsm_optimize_immature_points_batch: ") + msg).c_str()); };
  if (!ctx || n_jobs < 1 || !jobs) return bad("bad argument");
  if (const char *e = immature_settings_error(huber_th, min_idepth_h_act, gn_iterations)) return bad(e);
  size_t pts = 0;
  for (int j = 0; j < n_jobs; j++) {
    const dsm_immature_job &J = jobs[j];
    if (!J.window || J.window->ctx != ctx) return bad("no window, or a window of another context");
    if (J.window->w != jobs[0].window->w || J.window->h != jobs[0].window->h) return bad("one geometry per call");
    if (const char *e = immature_job_error(J)) return bad(e);
    for (int f = 0; f < J.n_frames; f++)
      if (J.window->find(J.frame_ids[f]) < 0) return bad("a frame id that is not in the window");
    pts += (size_t)J.n_pts;
  }
  if (pts > kMaxPoints) return bad("too many points in one call");
  *pts_out = pts;
  return DSM_OK;
}

int window_slot_for_put(dsm_window *win, int frame_id, const char *who, int *slot) {
  if (win->find(frame_id) >= 0) return invalid((std::string(who) + ": the frame id is already in the window").c_str());
  for (int i = 0; i < win->capacity; i++)
    if (!win->used[i]) {
      *slot = i;
      return DSM_OK;
    }
  return invalid((std::string(who) + ": the window is full").c_str());
}

} // namespace

extern "C" {

int dsm_window_create(dsm_context *ctx, int w, int h, int capacity, dsm_window **out) {
  if (out) *out = nullptr;
  if (!ctx || !out || w < 8 || h < 8 || (long long)w * h > (1ll << 28) || capacity < 1 || capacity > DSM_WINDOW_MAX_FRAMES)
    return invalid("dsm_window_create: bad argument");
  DSM_HIP(hipSetDevice(ctx->device));
  dsm_window *win = new dsm_window;
  win->ctx = ctx, win->w = w, win->h = h, win->capacity = capacity;
  hipError_t e = hipMalloc(&win->d_planes, sizeof(float) * (size_t)capacity * w * h);
  if (e != hipSuccess) {
    delete win;
    return hip_fail(e, "dsm_window_create", __FILE__, __LINE__);
  }
  *out = win;
  return DSM_OK;
}

int dsm_window_destroy(dsm_window *win) {
  if (!win) return DSM_OK;
  (void)hipSetDevice(win->ctx->device);
  if (win->d_planes) (void)hipFree(win->d_planes);
  delete win;
  return DSM_OK;
}

int dsm_window_put_host(dsm_window *win, int frame_id, const float *I) {
  if (!win || !I) return invalid("dsm_window_put_host: bad argument");
  int slot = -1;
  int rc = window_slot_for_put(win, frame_id, "dsm_window_put_host", &slot);
  if (rc) return rc;
  DSM_HIP(hipSetDevice(win->ctx->device));
  DSM_HIP(hipMemcpyAsync(win->plane(slot), I, sizeof(float) * (size_t)win->w * win->h, hipMemcpyHostToDevice, win->ctx->stream));
  DSM_HIP(hipStreamSynchronize(win->ctx->stream));
  win->ids[slot] = frame_id, win->used[slot] = true;
  return DSM_OK;
}

int dsm_window_put_from_tracker(dsm_window *win, int frame_id, dsm_tracker *owner, int slot_of_owner) {
  if (!win || !owner || slot_of_owner < 0 || slot_of_owner > 1) return invalid("dsm_window_put_from_tracker: bad argument");
  if (owner->ctx != win->ctx) return invalid("dsm_window_put_from_tracker: the tracker belongs to another context");
  if (owner->w != win->w || owner->h != win->h) return invalid("dsm_window_put_from_tracker: the tracker's level 0 has another geometry");
  if (!owner->have_frame[slot_of_owner]) return invalid("dsm_window_put_from_tracker: no frame in this slot");
  int slot = -1;
  int rc = window_slot_for_put(win, frame_id, "dsm_window_put_from_tracker", &slot);
  if (rc) return rc;
  DSM_HIP(hipSetDevice(win->ctx->device));
  // behind the pyramid kernels of the hand-over on the same stream
  DSM_HIP(hipMemcpyAsync(win->plane(slot), owner->d_img[slot_of_owner][0], sizeof(float) * (size_t)win->w * win->h, hipMemcpyDeviceToDevice,
                         win->ctx->stream));
  DSM_HIP(hipStreamSynchronize(win->ctx->stream));
  win->ids[slot] = frame_id, win->used[slot] = true;
  return DSM_OK;
}

int dsm_window_drop(dsm_window *win, int frame_id) {
  if (!win) return invalid("dsm_window_drop: no window");
  const int slot = win->find(frame_id);
  if (slot < 0) return invalid("dsm_window_drop: the frame id is not in the window");
  win->used[slot] = false;
  return DSM_OK;
}

int dsm_window_get(dsm_window *win, int frame_id, float *out) {
  if (!win || !out) return invalid("dsm_window_get: bad argument");
  const int slot = win->find(frame_id);
  if (slot < 0) return invalid("dsm_window_get: the frame id is not in the window");
  DSM_HIP(hipSetDevice(win->ctx->device));
  DSM_HIP(hipMemcpyAsync(out, win->plane(slot), sizeof(float) * (size_t)win->w * win->h, hipMemcpyDeviceToHost, win->ctx->stream));
  DSM_HIP(hipStreamSynchronize(win->ctx->stream));
  return DSM_OK;
}

int dsm_optimize_immature_points_batch(dsm_context *ctx, int n_jobs, const dsm_immature_job *jobs, float huber_th, float min_idepth_h_act,
                                       int gn_iterations) {
  size_t pts = 0;
  int rc = check_jobs(ctx, n_jobs, jobs, huber_th, min_idepth_h_act, gn_iterations, &pts);
  if (rc) return rc;
  if (pts == 0) return DSM_OK;
  // staged [job table | pre_R, pre_t, pre_aff, host, u, v, idepth_min, idepth_max, energy_th, color, weights of every job], read back
  // [kOutWords words per point]
  size_t words = 0;
  for (int j = 0; j < n_jobs; j++) words += 14 * (size_t)jobs[j].n_frames * jobs[j].n_frames + 22 * (size_t)jobs[j].n_pts;
  CallArena A;
  const size_t o_jobs = A.in.take(sizeof(ImJob) * n_jobs), o_stage = A.in.take(4 * words), o_out = A.out.take(4 * kOutWords * pts);
  if ((rc = A.bind(ctx))) return rc;
  ImJob *hj = A.host_in<ImJob>(o_jobs);
  WordPacker W{A.host_in<float>(o_stage)};
  size_t op = 0;
  int max_pts = 0;
  for (int j = 0; j < n_jobs; j++) {
    const dsm_immature_job &J = jobs[j];
    const size_t nf = J.n_frames, n = J.n_pts;
    ImJob &D = hj[j];
    memset(&D, 0, sizeof D);
    for (size_t f = 0; f < nf; f++) D.plane[f] = J.window->plane(J.window->find(J.frame_ids[f]));
    D.fx = J.cam[0], D.fy = J.cam[1], D.cx = J.cam[2], D.cy = J.cam[3], D.fxi = J.cam_inv[0], D.fyi = J.cam_inv[1];
    D.n_frames = J.n_frames, D.n_pts = J.n_pts, D.min_obs = J.min_obs, D.out_off = (int)op;
    W.put(&D.off_R, J.pre_R, 9 * nf * nf);
    W.put(&D.off_t, J.pre_t, 3 * nf * nf);
    W.put(&D.off_aff, J.pre_aff, 2 * nf * nf);
    W.put(&D.off_host, J.host, n);
    W.put(&D.off_u, J.u, n);
    W.put(&D.off_v, J.v, n);
    W.put(&D.off_idmin, J.idepth_min, n);
    W.put(&D.off_idmax, J.idepth_max, n);
    W.put(&D.off_eth, J.energy_th, n);
    W.put(&D.off_color, J.color, 8 * n);
    W.put(&D.off_wt, J.weights, 8 * n);
    op += n;
    max_pts = std::max(max_pts, J.n_pts);
  }
  if ((rc = A.upload())) return rc;
  hipLaunchKernelGGL(immature_kernel, dim3((max_pts + kWavesPerBlock - 1) / kWavesPerBlock, n_jobs), dim3(64 * kWavesPerBlock), 0, ctx->stream,
                     A.dev_in<const ImJob>(o_jobs), A.dev_in<const float>(o_stage), A.dev_out<unsigned>(o_out), jobs[0].window->w,
                     jobs[0].window->h, huber_th, min_idepth_h_act, gn_iterations);
  DSM_HIP(hipGetLastError());
  if ((rc = A.fetch(4 * kOutWords * pts))) return rc;
  const unsigned *ho = A.host_out<unsigned>(o_out);
  for (int j = 0; j < n_jobs; j++) {
    const dsm_immature_job &J = jobs[j];
    const int nf = J.n_frames;
    for (int i = 0; i < J.n_pts; i++) {
      const unsigned *q = ho + (size_t)(hj[j].out_off + i) * kOutWords;
      memcpy(&J.idepth_out[i], &q[0], 4);
      if (J.hdd_out) memcpy(&J.hdd_out[i], &q[1], 4);
      if (J.bd_out) memcpy(&J.bd_out[i], &q[2], 4);
      if (J.energy_out) memcpy(&J.energy_out[i], &q[3], 4);
      J.status[i] = (unsigned char)(q[4] & 0xff);
      if (J.iterations_out) J.iterations_out[i] = (int)(q[4] >> 8);
      memcpy(&J.res_state[(size_t)i * nf], &q[5], nf);
    }
  }
  return DSM_OK;
}

} // extern "C"
