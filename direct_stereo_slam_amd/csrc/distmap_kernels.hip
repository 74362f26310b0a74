// distmap_kernels.hip -- CoarseDistanceMap (TrackerAndScaler.h:139-170, TrackerAndScaler.cpp:1174-1362) and the activation walk of
// FrontEnd::activatePointsMT (FrontEnd.cpp:371-451) on the device, batched over the windows of many sequences.  Semantics: D1-D6 of
// DESIGN.md section 12.  Everything is integer-exact: a map cell holds 0..39 or "far" (1000 in the reference), kept as one byte
// (255 = far), which is exact because every comparison of a cell is against a level k <= 39.
//
// One dsm_activate_points_batch = one staged copy, one launch sequence, one read-back:
//   distmap_fill_kernel     (16 cells per thread, blockIdx.y = job)  D1: every cell far
//   distmap_project_kernel  (one thread per seed or candidate, blockIdx.y = job)  D2 / D6: the projection; a seed writes 0 into
//                           its cell, a candidate leaves its cell index (or -1), the fractional part of ptp[0] and its threshold
//   distmap_dilate_kernel   x 39 (one thread per cell, blockIdx.y = job)  D3 / D4: level k; the launch boundary is the level
//                           synchronisation.  From a fresh map the frontier of level k is exactly the set of non-border cells that
//                           hold k - 1, so a cell above k takes k when it has such a neighbour.  In place: a cell only ever changes
//                           from above k to k within a launch, and neither value is the k - 1 a neighbour looks for.
//   distmap_select_kernel   (one wave per job)  D5 / D6: the greedy walk.  Map values never increase, so a candidate that fails
//                           against the current map has failed for good: the wave evaluates 64 candidates at once, accepts the lowest
//                           passing lane, rejects the lanes before it, adds the accepted cell (growDistBFS with frontier lists in LDS,
//                           stopping when the frontier is empty) and re-evaluates the lanes behind it.  The map is held in LDS when
//                           its bytes fit (616 x 184 does), otherwise the same code works on it in global memory.
// No kernel waits for another workgroup; every loop is bounded by 39, by the cell count or by n_cand.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "call_arena.hpp"
#include "point_math.hpp"

using namespace dsm;

struct dsm_distmap {
  dsm_context *ctx = nullptr;
  int w = 0, h = 0, w1 = 0, h1 = 0;
  unsigned char *d_map = nullptr; // w1 * h1 bytes, allocation rounded up to 16
  size_t bytes16 = 0;
};

namespace {

constexpr int kFar = 255;                // 1000 of the reference
constexpr float kFarValue = 1000.0f;     // TrackerAndScaler.cpp:1203
constexpr int kLevels = 40;              // growDistBFS: k = 1 .. 39 (:1238)
constexpr int kListCap = 6272;           // >= 79 * 79: a cell written by one add lies within 39 steps of it (8-neighbourhood)
constexpr int kLdsMapMax = 135 * 1024;   // map bytes held in LDS by distmap_select_kernel<true> (+ the two lists < 160 KiB)
constexpr int kThreads = 256;
constexpr size_t kMaxItems = 1u << 26;   // seeds + candidates of one call

struct DmJob {
  unsigned char *map;
  int n_seeds, n_cand;
  int off_krki, off_kt, off_host, off_u, off_v, off_id, off_type; // 4-byte words into the staged inputs
  int out_off;                                                    // first candidate of the job in cell / frac / thr / decision
  float min_act;
};

__global__ __launch_bounds__(kThreads) void distmap_fill_kernel(const DmJob *jobs, int bytes16) {
  const int o = (blockIdx.x * kThreads + threadIdx.x) * 16;
  if (o >= bytes16) return;
  *reinterpret_cast<uint4 *>(jobs[blockIdx.y].map + o) = make_uint4(~0u, ~0u, ~0u, ~0u);
}

// D2 / D6: ptp = KRKi (u, v, 1) + Kt idepth (point_math.hpp, shared with the host form)
__global__ __launch_bounds__(kThreads) void distmap_project_kernel(const DmJob *jobs, const float *stage, int *cell, float *frac, float *thr,
                                                                   int w1, int h1, int with_cand) {
  const DmJob J = jobs[blockIdx.y];
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= J.n_seeds + (with_cand ? J.n_cand : 0)) return;
  const int hst = reinterpret_cast<const int *>(stage)[J.off_host + i];
  const float *M = stage + J.off_krki + 9 * hst, *T = stage + J.off_kt + 3 * hst;
  const float u = stage[J.off_u + i], v = stage[J.off_v + i], id = stage[J.off_id + i];
  const pt::Vec3 p = pt::add_translation(pt::rotate_uv1(M, u, v), T, id);
  const float qu = p.x / p.z + 0.5f, qv = p.y / p.z + 0.5f;
  const bool ok = qu >= 1.0f && qv >= 1.0f && qu < (float)w1 && qv < (float)h1; // NaN and +-inf fail
  const int c = ok ? (int)qu + w1 * (int)qv : -1;
  if (i < J.n_seeds) {
    if (ok) J.map[c] = 0; // :1223
  } else {
    const int o = J.out_off + (i - J.n_seeds);
    cell[o] = c;
    frac[o] = p.x - floorf(p.x);                              // FrontEnd.cpp:440: the unnormalised ptp[0]
    thr[o] = J.min_act * stage[J.off_type + (i - J.n_seeds)]; // :442
  }
}

__device__ __forceinline__ bool inner(int x, int y, int w1, int h1) { return x > 0 && y > 0 && x < w1 - 1 && y < h1 - 1; }

// D3 / D4, level k of a map under construction (see the head of the file)
__global__ __launch_bounds__(kThreads) void distmap_dilate_kernel(const DmJob *jobs, int w1, int h1, int k) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= w1 * h1) return;
  unsigned char *m = jobs[blockIdx.y].map;
  if (m[i] <= k) return;
  const int x = i % w1, y = i / w1, src = k - 1;
  bool hit = (inner(x + 1, y, w1, h1) && m[i + 1] == src) || (inner(x - 1, y, w1, h1) && m[i - 1] == src) ||
             (inner(x, y + 1, w1, h1) && m[i + w1] == src) || (inner(x, y - 1, w1, h1) && m[i - w1] == src);
  if (!hit && (k & 1))
    hit = (inner(x + 1, y + 1, w1, h1) && m[i + 1 + w1] == src) || (inner(x - 1, y + 1, w1, h1) && m[i - 1 + w1] == src) ||
          (inner(x - 1, y - 1, w1, h1) && m[i - 1 - w1] == src) || (inner(x + 1, y - 1, w1, h1) && m[i + 1 - w1] == src);
  if (hit) m[i] = (unsigned char)k;
}

// D5 by one wave: the cell (ox, oy) becomes 0, then growDistBFS(1) from it on the map as it stands.  la / lb: the two frontier lists,
// entries relative to (ox, oy), one signed byte per axis.  Within a level the neighbours are visited one direction at a time:
// distinct frontier cells have distinct neighbours in one direction, so no two lanes meet in a cell, and a write of an earlier
// direction is seen by the later ones (the barrier orders the lanes' accesses); a cell therefore enters the next list once.
template <typename M>
__device__ __forceinline__ void grow_from(M m, int w1, int h1, int ox, int oy, unsigned short *la, unsigned short *lb, int lane) {
  if (lane == 0) {
    m[ox + w1 * oy] = 0;
    la[0] = 0;
  }
  __syncthreads();
  int n = 1;
  for (int k = 1; k < kLevels && n > 0; k++) {
    int n2 = 0;
    for (int base = 0; base < n; base += 64) {
      const int i = base + lane;
      bool act = i < n;
      int x = 0, y = 0;
      if (act) {
        const unsigned short e = la[i];
        x = ox + (int)(signed char)(e & 0xff);
        y = oy + (int)(signed char)(e >> 8);
        act = inner(x, y, w1, h1); // D4
      }
#pragma unroll
      for (int d = 0; d < 8; d++) {
        constexpr int DX[8] = {1, -1, 0, 0, 1, -1, -1, 1}, DY[8] = {0, 0, 1, -1, 1, 1, -1, -1};
        if (d >= 4 && !(k & 1)) break; // even k: 4-neighbourhood
        const int nx = x + DX[d], ny = y + DY[d];
        bool wr = false;
        if (act) {
          const int idx = nx + w1 * ny;
          if (m[idx] > k) {
            m[idx] = (unsigned char)k;
            wr = true;
          }
        }
        const unsigned long long mask = __ballot(wr);
        if (wr) {
          const int pos = n2 + __popcll(mask & ((1ull << lane) - 1ull));
          if (pos < kListCap) lb[pos] = (unsigned short)(((nx - ox) & 0xff) | (((ny - oy) & 0xff) << 8));
        }
        n2 += __popcll(mask);
        __syncthreads();
      }
    }
    n = n2 < kListCap ? n2 : kListCap;
    unsigned short *t = la;
    la = lb;
    lb = t;
  }
}

// D6 for one job by one wave (see the head of the file)
template <typename M>
__device__ __forceinline__ int select_walk(M m, const DmJob &J, const int *cell, const float *frac, const float *thr, unsigned char *dec,
                                           int w1, int h1, unsigned short *la, unsigned short *lb, int lane) {
  int n_act = 0;
  for (int base = 0; base < J.n_cand; base += 64) {
    const int i = base + lane;
    const bool valid = i < J.n_cand;
    const int c = valid ? cell[J.out_off + i] : -1;
    const float fr = valid ? frac[J.out_off + i] : 0.f, th = valid ? thr[J.out_off + i] : 0.f;
    int d = (valid && c < 0) ? 2 : 0;
    bool alive = valid && c >= 0;
    for (;;) {
      bool pass = false;
      if (alive) {
        const int b = m[c];
        pass = ((b == kFar ? kFarValue : (float)b) + fr) >= th; // FrontEnd.cpp:439-442
      }
      const unsigned long long mask = __ballot(pass);
      if (!mask) break;
      const int first = __ffsll((long long)mask) - 1;
      if (lane <= first) alive = false; // the lanes before the first passing one have failed for good
      if (lane == first) d = 1;
      const int cf = __shfl(c, first);
      grow_from(m, w1, h1, cf % w1, cf / w1, la, lb, lane); // :443
      n_act++;
    }
    if (valid) dec[J.out_off + i] = (unsigned char)d;
  }
  return n_act;
}

template <bool LDS>
__global__ __launch_bounds__(64) void distmap_select_kernel(const DmJob *jobs, const int *cell, const float *frac, const float *thr,
                                                            unsigned char *dec, int *n_act, int w1, int h1, int bytes16) {
  __shared__ unsigned short s_list[2][kListCap];
  __shared__ __attribute__((aligned(16))) unsigned char s_map[LDS ? kLdsMapMax : 16];
  const DmJob J = jobs[blockIdx.x];
  const int lane = threadIdx.x;
  int n = 0;
  if (J.n_cand > 0) {
    if (LDS) {
      for (int o = lane * 16; o < bytes16; o += 64 * 16) *reinterpret_cast<uint4 *>(s_map + o) = *reinterpret_cast<const uint4 *>(J.map + o);
      __syncthreads();
      n = select_walk(s_map, J, cell, frac, thr, dec, w1, h1, s_list[0], s_list[1], lane);
      __syncthreads();
      for (int o = lane * 16; o < bytes16; o += 64 * 16) *reinterpret_cast<uint4 *>(J.map + o) = *reinterpret_cast<const uint4 *>(s_map + o);
    } else {
      n = select_walk(J.map, J, cell, frac, thr, dec, w1, h1, s_list[0], s_list[1], lane);
    }
  }
  if (lane == 0) n_act[blockIdx.x] = n;
}

// dsm_distmap_add: D5 on the map in global memory
__global__ __launch_bounds__(64) void distmap_add_kernel(unsigned char *map, int w1, int h1, int u, int v) {
  __shared__ unsigned short s_list[2][kListCap];
  grow_from(map, w1, h1, u, v, s_list[0], s_list[1], (int)threadIdx.x);
}

// all-or-nothing validation of a batch: nothing is enqueued before every job has passed
int check_jobs(dsm_context *ctx, int n_jobs, const dsm_activation_job *jobs, bool with_cand, size_t *items_out,
               size_t *cands_out) {
  auto bad = [with_cand](const char *msg) {
    return invalid((std::string(with_cand ? "dsm_activate_points_batch: " : "dsm_distmaps_make: ") + msg).c_str());
  };
  if (!ctx || n_jobs < 1 || !jobs) return bad("bad argument");
  size_t items = 0, cands = 0;
  std::vector<const dsm_distmap *> seen;
  for (int j = 0; j < n_jobs; j++) {
    const dsm_activation_job &J = jobs[j];
    const int nc = with_cand ? J.n_cand : 0;
    if (!J.map || J.map->ctx != ctx) return bad("no map, or a map of another context");
    if (J.map->w != jobs[0].map->w || J.map->h != jobs[0].map->h) return bad("one geometry per call");
    if (std::find(seen.begin(), seen.end(), J.map) != seen.end()) return bad("a map may appear in one job only");
    seen.push_back(J.map);
    if (const char *e = activation_job_error(J, with_cand)) return bad(e);
    items += (size_t)J.n_seeds + nc + 12 * (size_t)J.n_hosts, cands += nc;
  }
  if (items > kMaxItems) return bad("too many points in one call");
  *items_out = items, *cands_out = cands;
  return DSM_OK;
}

int run_batch(dsm_context *ctx, int n_jobs, const dsm_activation_job *jobs, bool with_cand) {
  size_t items = 0, cands = 0;
  int rc = check_jobs(ctx, n_jobs, jobs, with_cand, &items, &cands);
  if (rc) return rc;
  const int w1 = jobs[0].map->w1, h1 = jobs[0].map->h1, bytes16 = (int)jobs[0].map->bytes16;
  // staged [job table | krki, kt, host, u, v, idepth, type of every job], device-only [cell | frac | thr], read back [decision | n_activated]
  size_t words = 0;
  for (int j = 0; j < n_jobs; j++)
    words += 12 * (size_t)jobs[j].n_hosts + 4 * ((size_t)jobs[j].n_seeds + (with_cand ? jobs[j].n_cand : 0)) + (with_cand ? jobs[j].n_cand : 0);
  CallArena A;
  const size_t o_jobs = A.in.take(sizeof(DmJob) * n_jobs), o_stage = A.in.take(4 * words), b_c4 = 4 * std::max<size_t>(1, cands);
  const size_t o_cell = A.work.take(b_c4), o_frac = A.work.take(b_c4), o_thr = A.work.take(b_c4);
  const size_t o_dec = A.out.take(std::max<size_t>(1, cands)), o_nact = A.out.take(sizeof(int) * n_jobs);
  if ((rc = A.bind(ctx))) return rc;
  DmJob *hj = A.host_in<DmJob>(o_jobs);
  WordPacker W{A.host_in<float>(o_stage)};
  size_t oc = 0;
  int max_items = 0;
  for (int j = 0; j < n_jobs; j++) {
    const dsm_activation_job &J = jobs[j];
    const int ns = J.n_seeds, nc = with_cand ? J.n_cand : 0, n = ns + nc;
    DmJob &D = hj[j];
    D.map = J.map->d_map, D.n_seeds = ns, D.n_cand = nc, D.out_off = (int)oc, D.min_act = J.min_act_dist;
    W.put(&D.off_krki, J.krki, 9 * (size_t)J.n_hosts);
    W.put(&D.off_kt, J.kt, 3 * (size_t)J.n_hosts);
    W.put2(&D.off_host, J.seed_host, ns, J.cand_host, nc);
    W.put2(&D.off_u, J.seed_u, ns, J.cand_u, nc);
    W.put2(&D.off_v, J.seed_v, ns, J.cand_v, nc);
    W.put2(&D.off_id, J.seed_idepth, ns, J.cand_idepth, nc);
    W.put(&D.off_type, J.cand_type, nc);
    oc += nc;
    max_items = std::max(max_items, n);
  }
  const DmJob *dj = A.dev_in<const DmJob>(o_jobs);
  int *d_cell = A.dev_work<int>(o_cell);
  float *d_frac = A.dev_work<float>(o_frac), *d_thr = A.dev_work<float>(o_thr);
  unsigned char *d_dec = A.dev_out<unsigned char>(o_dec);
  int *d_nact = A.dev_out<int>(o_nact);
  hipStream_t st = ctx->stream;
  if ((rc = A.upload())) return rc;
  hipLaunchKernelGGL(distmap_fill_kernel, dim3((bytes16 / 16 + kThreads - 1) / kThreads, n_jobs), dim3(kThreads), 0, st, dj, bytes16);
  if (max_items)
    hipLaunchKernelGGL(distmap_project_kernel, dim3((max_items + kThreads - 1) / kThreads, n_jobs), dim3(kThreads), 0, st, dj,
                       A.dev_in<const float>(o_stage), d_cell, d_frac, d_thr, w1, h1, with_cand ? 1 : 0);
  for (int k = 1; k < kLevels; k++)
    hipLaunchKernelGGL(distmap_dilate_kernel, dim3((w1 * h1 + kThreads - 1) / kThreads, n_jobs), dim3(kThreads), 0, st, dj, w1, h1, k);
  if (with_cand) {
    if (bytes16 <= kLdsMapMax)
      hipLaunchKernelGGL(distmap_select_kernel<true>, dim3(n_jobs), dim3(64), 0, st, dj, (const int *)d_cell, (const float *)d_frac,
                         (const float *)d_thr, d_dec, d_nact, w1, h1, bytes16);
    else
      hipLaunchKernelGGL(distmap_select_kernel<false>, dim3(n_jobs), dim3(64), 0, st, dj, (const int *)d_cell, (const float *)d_frac,
                         (const float *)d_thr, d_dec, d_nact, w1, h1, bytes16);
  }
  DSM_HIP(hipGetLastError());
  if ((rc = A.fetch(with_cand ? A.out.used : 0))) return rc; // (no candidates: the maps are made, nothing comes back)
  if (with_cand) {
    const unsigned char *h_dec = A.host_out<unsigned char>(o_dec);
    const int *h_nact = A.host_out<int>(o_nact);
    for (int j = 0; j < n_jobs; j++) {
      if (jobs[j].n_cand) memcpy(jobs[j].decision_out, h_dec + hj[j].out_off, jobs[j].n_cand);
      if (jobs[j].n_activated_out) *jobs[j].n_activated_out = h_nact[j];
    }
  }
  return DSM_OK;
}

} // namespace

extern "C" {

int dsm_distmap_create(dsm_context *ctx, int w, int h, dsm_distmap **out) {
  if (out) *out = nullptr;
  if (!ctx || !out || w < 2 || h < 2 || (long long)(w >> 1) * (h >> 1) > (1ll << 28)) return invalid("dsm_distmap_create: bad argument");
  DSM_HIP(hipSetDevice(ctx->device));
  dsm_distmap *m = new dsm_distmap;
  m->ctx = ctx, m->w = w, m->h = h, m->w1 = w >> 1, m->h1 = h >> 1; // makeK, TrackerAndScaler.cpp:1349-1350
  m->bytes16 = ((size_t)m->w1 * m->h1 + 15) & ~(size_t)15;
  hipError_t e = hipMalloc(&m->d_map, m->bytes16);
  if (e == hipSuccess) e = hipMemsetAsync(m->d_map, kFar, m->bytes16, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) {
    if (m->d_map) (void)hipFree(m->d_map);
    delete m;
    return hip_fail(e, "dsm_distmap_create", __FILE__, __LINE__);
  }
  *out = m;
  return DSM_OK;
}

int dsm_distmap_destroy(dsm_distmap *map) {
  if (!map) return DSM_OK;
  (void)hipSetDevice(map->ctx->device);
  if (map->d_map) (void)hipFree(map->d_map);
  delete map;
  return DSM_OK;
}

int dsm_distmap_get(dsm_distmap *map, float *out) {
  if (!map || !out) return invalid("dsm_distmap_get: bad argument");
  const size_t n = (size_t)map->w1 * map->h1;
  std::vector<unsigned char> b(n);
  DSM_HIP(hipSetDevice(map->ctx->device));
  DSM_HIP(hipMemcpyAsync(b.data(), map->d_map, n, hipMemcpyDeviceToHost, map->ctx->stream));
  DSM_HIP(hipStreamSynchronize(map->ctx->stream));
  for (size_t i = 0; i < n; i++) out[i] = b[i] == kFar ? kFarValue : (float)b[i];
  return DSM_OK;
}

int dsm_distmap_add(dsm_distmap *map, int u, int v) {
  if (!map) return invalid("dsm_distmap_add: no map");
  if (u < 0 || v < 0 || u >= map->w1 || v >= map->h1) return invalid("dsm_distmap_add: (u, v) outside the level-1 map");
  DSM_HIP(hipSetDevice(map->ctx->device));
  hipLaunchKernelGGL(distmap_add_kernel, dim3(1), dim3(64), 0, map->ctx->stream, map->d_map, map->w1, map->h1, u, v);
  DSM_HIP(hipGetLastError());
  DSM_HIP(hipStreamSynchronize(map->ctx->stream));
  return DSM_OK;
}

int dsm_distmaps_make(dsm_context *ctx, int n_jobs, const dsm_activation_job *jobs) { return run_batch(ctx, n_jobs, jobs, false); }

int dsm_activate_points_batch(dsm_context *ctx, int n_jobs, const dsm_activation_job *jobs) { return run_batch(ctx, n_jobs, jobs, true); }

} // extern "C"
