// trace_kernels.hip -- the loop of FrontEnd::traceNewCoarse (FrontEnd.cpp:276-327) on the device: ImmaturePoint::traceOn for every
// immature point of many sequences against each sequence's new frame, in one call.  Semantics: T1-T16 of DESIGN.md section 14.
//
// One dsm_trace_points_batch = one staged copy, ONE launch, one read-back:
//   trace_kernel  eight lanes per point, one lane per pattern pixel, eight points per wave, four waves per workgroup,
//                 blockIdx.y = job.  The geometry (T1-T7) runs redundantly on the eight lanes of a point.  The search (T9) is a loop
//                 over the steps whose trip count is the largest numSteps of the wave, four steps per trip: the positions of the four
//                 come from the chain of float additions before any texel is back, so their sixteen texel loads are in flight
//                 together; lanes of points that are finished or never searched are masked.  The refinement (T11) runs the eight
//                 points of the wave at once.
// Bit parity with the sequential float sums: a lane computes its pixel's term (trace_math.hpp and point_math.hpp, shared with the
// host form) and the eight lanes of a point add the eight terms as one chain in lane order = pattern order (__shfl, width 8), so
// every lane of the point holds the same sum.  errors[] (T10) sits in LDS, 100 floats per point; only lanes of the same wave
// exchange data through it, and no wave waits for another.  Loops are bounded by 99 steps, gn_iterations and 8.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "call_arena.hpp"
#include "trace_math.hpp"

using namespace dsm;

namespace {

constexpr int kWavesPerBlock = 4, kPointsPerWave = 8, kPointsPerBlock = kWavesPerBlock * kPointsPerWave;
constexpr int kStepsPerTrip = 4;
constexpr int kErrStride = 100; // floats per point in LDS: 8 points of a wave start 4 banks apart
constexpr int kInWords = 31;    // staged per point
constexpr int kOutWords = 8;    // per point: status | steps << 8, idepth_min, idepth_max, quality, uv (2), interval, spare
constexpr size_t kMaxPoints = 1u << 24;

struct TrJob {
  const float *plane; // the new frame, level 0
  int n_hosts, n_pts;
  int off_R, off_t, off_aff, off_host, off_u, off_v, off_eth, off_G, off_color, off_wt, off_status, off_idmin, off_idmax, off_quality, off_uv,
      off_interval; // 4-byte words into the staged inputs
  int out_off;      // first point of the job in the output
};

// lanes of one wave only: what the lanes of a point wrote to LDS is read by the other lanes of the same point
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the eight terms of a point, lane by lane, added in pattern order; every lane of the point gets the sum
__device__ __forceinline__ float chain8(float acc, float term) {
#pragma unroll
  for (int k = 0; k < 8; k++) acc += __shfl(term, k, 8);
  return acc;
}

__global__ __launch_bounds__(64 * kWavesPerBlock) void trace_kernel(const TrJob *jobs, const float *stage, unsigned *out, int w, int h,
                                                                    dsm_trace_params S) {
  __shared__ float errs[kWavesPerBlock][kPointsPerWave][kErrStride];
  const TrJob &J = jobs[blockIdx.y];
  const int wave = (int)(threadIdx.x >> 6), lane = threadIdx.x & 63, grp = lane >> 3, k = lane & 7;
  const int pt0 = ((int)blockIdx.x * kWavesPerBlock + wave) * kPointsPerWave;
  if (pt0 >= J.n_pts) return; // wave-uniform; the kernel has no workgroup barrier
  const bool have = pt0 + grp < J.n_pts;
  const int pt = have ? pt0 + grp : J.n_pts - 1; // a group without a point reads the last point's data and does nothing with it
  const int *stage_i = reinterpret_cast<const int *>(stage);
  const float *I = J.plane;
  const int host = stage_i[J.off_host + pt];
  float R[9], t[3], aff[2], G[4];
#pragma unroll
  for (int i = 0; i < 9; i++) R[i] = stage[J.off_R + 9 * host + i];
#pragma unroll
  for (int i = 0; i < 3; i++) t[i] = stage[J.off_t + 3 * host + i];
  aff[0] = stage[J.off_aff + 2 * host], aff[1] = stage[J.off_aff + 2 * host + 1];
#pragma unroll
  for (int i = 0; i < 4; i++) G[i] = stage[J.off_G + 4 * pt + i];
  const float u = stage[J.off_u + pt], v = stage[J.off_v + pt], energy_th = stage[J.off_eth + pt];
  const float color = stage[J.off_color + 8 * pt + k], wt = stage[J.off_wt + 8 * pt + k];
  const int entered = stage_i[J.off_status + pt];
  trc::Point P{have ? entered : DSM_IPS_OOB, stage[J.off_idmin + pt], stage[J.off_idmax + pt], stage[J.off_quality + pt],
               stage[J.off_uv + 2 * pt], stage[J.off_uv + 2 * pt + 1], stage[J.off_interval + pt]};
  trc::Line L{};
  const bool run = trc::geometry(w, h, R, t, u, v, G, S, P, L); // T1-T7, the same in the eight lanes of a point
  const int ns = run ? L.numSteps : 0;
  float rx, ry;
  trc::rotated_pattern(R, k, rx, ry);

  // T9: the search
  float *my_errs = errs[wave][grp];
  float ptx = L.ptx, pty = L.pty, bestU = 0.f, bestV = 0.f, bestEnergy = 1e10f;
  int bestIdx = -1;
  for (int s0 = 0; __ballot(s0 < ns) != 0ull; s0 += kStepsPerTrip) {
    float px[kStepsPerTrip], py[kStepsPerTrip], x[kStepsPerTrip], y[kStepsPerTrip];
    bool ok[kStepsPerTrip];
    pt::Tex4 T[kStepsPerTrip];
#pragma unroll
    for (int j = 0; j < kStepsPerTrip; j++) { // the positions are the chain of additions; all loads of the trip are issued here
      px[j] = ptx, py[j] = pty;
      x[j] = ptx + rx, y[j] = pty + ry;
      ok[j] = s0 + j < ns && trc::guard(x[j], y[j], w, h); // T8: no load leaves the plane
      T[j] = pt::Tex4{0.f, 0.f, 0.f, 0.f};
      if (ok[j]) T[j] = pt::load4(I, w, x[j], y[j]);
      ptx += L.dx;
      pty += L.dy;
    }
#pragma unroll
    for (int j = 0; j < kStepsPerTrip; j++) {
      const float term = trc::search_term(ok[j], pt::interp_I(T[j], x[j], y[j]), aff, color, S.huber_th);
      const float energy = chain8(0.f, term);
      if (s0 + j < ns) {
        if (k == 0) my_errs[s0 + j] = energy;
        if (energy < bestEnergy) bestU = px[j], bestV = py[j], bestEnergy = energy, bestIdx = s0 + j;
      }
    }
  }
  wave_lds_sync();

  // T10: the second best energy outside the radius; a minimum, so its order does not matter (no NaN wins, no -0 occurs)
  float secondBest = 1e10f;
  const int radius = trc::test_radius(S);
  for (int s = k; s < ns; s += 8)
    if (trc::outside_radius(s, bestIdx, radius)) {
      const float e = my_errs[s];
      if (e < secondBest) secondBest = e;
    }
#pragma unroll
  for (int m = 1; m < 8; m <<= 1) {
    const float o = __shfl_xor(secondBest, m, 8);
    if (o < secondBest) secondBest = o;
  }
  if (run) trc::quality_update(P, secondBest, bestEnergy, ns);

  // T11: the refinement, eight points at once
  trc::GN g{bestU, bestV, bestU, bestV, 0.f, bestEnergy};
  if (S.gn_iterations > 0) g.bestEnergy = 1e5f;
  bool live = run;
  for (int it = 0; it < S.gn_iterations && __ballot(live) != 0ull; it++) {
    const float x = g.bestU + rx, y = g.bestV + ry;
    const bool ok = live && trc::guard(x, y, w, h);
    float hI = 0.f, gx = 0.f, gy = 0.f, tH, tb, tE;
    if (ok) pt::interp_Ig(pt::load12(I, w, x, y), x, y, hI, gx, gy);
    const bool fin = trc::gn_terms(ok, hI, gx, gy, aff, color, wt, S.huber_th, L.dx, L.dy, tH, tb, tE);
    const unsigned counted = (unsigned)(__ballot(fin) >> (lane & 56)) & 0xffu; // the pixels of this point that reach H and b
    float H = 1.f, b = 0.f, E = 0.f;
#pragma unroll
    for (int kk = 0; kk < 8; kk++) {
      const float hk = __shfl(tH, kk, 8), bk = __shfl(tb, kk, 8), ek = __shfl(tE, kk, 8);
      if ((counted >> kk) & 1u) H += hk, b += bk;
      E += ek;
    }
    if (live && trc::gn_update(g, H, b, E, L.dx, L.dy, S.gn_threshold)) live = false;
  }
  if (run) trc::finish(P, L, g, t, energy_th, S, entered); // T12-T15

  unsigned word;
  switch (k) {
  case 0: word = (unsigned)P.status | ((unsigned)ns << 8); break; // T16
  case 1: word = __float_as_uint(P.idepth_min); break;
  case 2: word = __float_as_uint(P.idepth_max); break;
  case 3: word = __float_as_uint(P.quality); break;
  case 4: word = __float_as_uint(P.uv0); break;
  case 5: word = __float_as_uint(P.uv1); break;
  case 6: word = __float_as_uint(P.interval); break;
  default: word = 0u; break;
  }
  if (have) out[(size_t)(J.out_off + pt) * kOutWords + k] = word;
}

// the new frame of a job that check_jobs has passed
const float *target_plane(const dsm_trace_job &J) {
  if (J.target_tracker) return J.target_tracker->d_img[J.target_slot][0];
  return J.target_window->plane(J.target_window->find(J.target_frame_id));
}

// all-or-nothing validation of a batch: nothing is enqueued before every job has passed
int check_jobs(dsm_context *ctx, int n_jobs, const dsm_trace_job *jobs, const dsm_trace_params *params, int *w_out, int *h_out, size_t *pts_out,
               size_t *words_out) {
  auto bad = [](const char *msg) { return invalid((std::string("dsm_trace_points_batch: ") + msg).c_str()); };
  if (!ctx || n_jobs < 1 || n_jobs > 65535 || !jobs) return bad("bad argument");
  if (const char *e = trace_params_error(params)) return bad(e);
  size_t pts = 0, words = 0;
  int w = 0, h = 0;
  for (int j = 0; j < n_jobs; j++) {
    const dsm_trace_job &J = jobs[j];
    if (const char *e = trace_job_error(J)) return bad(e);
    if ((J.target_tracker != nullptr) == (J.target_window != nullptr)) return bad("a job names a tracker slot or a window frame, not both and not neither");
    int jw, jh;
    if (J.target_tracker) {
      const dsm_tracker *t = J.target_tracker;
      if (t->ctx != ctx) return bad("the tracker belongs to another context");
      if (J.target_slot < 0 || J.target_slot > 1 || !t->have_frame[J.target_slot]) return bad("no frame in this tracker slot");
      jw = t->w, jh = t->h;
    } else {
      const dsm_window *win = J.target_window;
      if (win->ctx != ctx) return bad("the window belongs to another context");
      if (win->find(J.target_frame_id) < 0) return bad("the frame id is not in the window");
      jw = win->w, jh = win->h;
    }
    if (j == 0) w = jw, h = jh;
    if (jw != w || jh != h) return bad("one geometry per call");
    pts += (size_t)J.n_pts;
    words += 14 * (size_t)J.n_hosts + kInWords * (size_t)J.n_pts;
  }
  if (w < 8 || h < 8) return bad("the target is smaller than 8 x 8");
  if (pts > kMaxPoints) return bad("too many points in one call");
  *w_out = w, *h_out = h, *pts_out = pts, *words_out = words;
  return DSM_OK;
}

} // namespace

extern "C" int dsm_trace_points_batch(dsm_context *ctx, int n_jobs, const dsm_trace_job *jobs, const dsm_trace_params *params) {
  size_t pts = 0, words = 0;
  int w = 0, h = 0;
  int rc = check_jobs(ctx, n_jobs, jobs, params, &w, &h, &pts, &words);
  if (rc) return rc;
  if (pts) {
    // staged [job table | krki, kt, aff, then the point arrays of every job], read back [kOutWords per point]
    CallArena A;
    const size_t o_jobs = A.in.take(sizeof(TrJob) * n_jobs), o_stage = A.in.take(4 * words), o_out = A.out.take(4 * kOutWords * pts);
    if ((rc = A.bind(ctx))) return rc;
    TrJob *hj = A.host_in<TrJob>(o_jobs);
    WordPacker W{A.host_in<float>(o_stage)};
    size_t op = 0;
    int max_pts = 0;
    for (int j = 0; j < n_jobs; j++) {
      const dsm_trace_job &J = jobs[j];
      const size_t nh = J.n_hosts, n = J.n_pts;
      TrJob &D = hj[j];
      memset(&D, 0, sizeof D);
      D.plane = target_plane(J), D.n_hosts = J.n_hosts, D.n_pts = J.n_pts, D.out_off = (int)op;
      W.put(&D.off_R, J.krki, 9 * nh);
      W.put(&D.off_t, J.kt, 3 * nh);
      W.put(&D.off_aff, J.aff, 2 * nh);
      W.put(&D.off_host, J.host, n);
      W.put(&D.off_u, J.u, n);
      W.put(&D.off_v, J.v, n);
      W.put(&D.off_eth, J.energy_th, n);
      W.put(&D.off_G, J.grad_h, 4 * n);
      W.put(&D.off_color, J.color, 8 * n);
      W.put(&D.off_wt, J.weights, 8 * n);
      int *status = (int *)W.reserve(&D.off_status, n);
      for (size_t i = 0; i < n; i++) status[i] = J.status[i];
      W.put(&D.off_idmin, J.idepth_min, n);
      W.put(&D.off_idmax, J.idepth_max, n);
      W.put(&D.off_quality, J.quality, n);
      W.put(&D.off_uv, J.trace_uv, 2 * n);
      W.put(&D.off_interval, J.trace_interval, n);
      op += n;
      max_pts = std::max(max_pts, J.n_pts);
    }
    if ((rc = A.upload())) return rc;
    hipLaunchKernelGGL(trace_kernel, dim3((max_pts + kPointsPerBlock - 1) / kPointsPerBlock, n_jobs), dim3(64 * kWavesPerBlock), 0, ctx->stream,
                       A.dev_in<const TrJob>(o_jobs), A.dev_in<const float>(o_stage), A.dev_out<unsigned>(o_out), w, h, *params);
    DSM_HIP(hipGetLastError());
    if ((rc = A.fetch(4 * kOutWords * pts))) return rc;
    const unsigned *ho = A.host_out<unsigned>(o_out);
    for (int j = 0; j < n_jobs; j++) {
      const dsm_trace_job &J = jobs[j];
      for (int i = 0; i < J.n_pts; i++) {
        const unsigned *q = ho + (size_t)(hj[j].out_off + i) * kOutWords;
        J.status[i] = (unsigned char)(q[0] & 0xff);
        if (J.steps_out) J.steps_out[i] = (int)(q[0] >> 8);
        memcpy(&J.idepth_min[i], &q[1], 4);
        memcpy(&J.idepth_max[i], &q[2], 4);
        memcpy(&J.quality[i], &q[3], 4);
        memcpy(&J.trace_uv[2 * (size_t)i], &q[4], 8);
        memcpy(&J.trace_interval[i], &q[6], 4);
      }
    }
  }
  for (int j = 0; j < n_jobs; j++) { // T16
    const dsm_trace_job &J = jobs[j];
    if (!J.counts_out) continue;
    int counts[6] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < J.n_pts; i++) counts[J.status[i]]++;
    memcpy(J.counts_out, counts, sizeof counts);
  }
  return DSM_OK;
}
