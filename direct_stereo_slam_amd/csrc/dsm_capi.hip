// dsm_capi.hip -- C ABI (include/dsm_hotpath.h) of the tracker / scale-optimiser hot path.
// Host side only orchestrates: uploads, launch sequencing of the LM state machine, read-back.
// All arithmetic of the path runs in the HIP kernels of tracker_kernels.hip.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "call_arena.hpp"
#include "dsm_internal.hpp"
#include <algorithm>
#include <utility>

namespace dsm {

static thread_local std::string g_err;
void set_error(const std::string &msg) { g_err = msg; }
int hip_fail(hipError_t e, const char *what, const char *file, int line) {
  char buf[512];
  snprintf(buf, sizeof buf, "HIP error %d (%s) at %s:%d: %s", (int)e, hipGetErrorString(e), file, line, what);
  g_err = buf;
  return DSM_ERR_HIP;
}

int invalid(const char *msg) {
  set_error(msg);
  return DSM_ERR_INVALID;
}

// One intensity plane of a w x h level.  Lanes whose point is not usable fetch their twelve taps around texel (2, 2)
// instead (rows 1-4, columns 1-4), always inside the image (dsm_tracker_create wants a coarsest level of at least 8 x 8);
// the four rows and few texels of slack are belt and braces.
static size_t plane_bytes(int w, int h) { return sizeof(float) * ((size_t)w * h + 4 * (size_t)w + 16); }

int ensure_stage(dsm_context *ctx, size_t floats) {
  if (floats <= ctx->stage_floats) return DSM_OK;
  ctx->stage_floats = 0;
  const int rc = realloc_dev(&ctx->d_stage, floats);
  if (rc) return rc;
  ctx->stage_floats = floats;
  return DSM_OK;
}

const void *pinned_device_pointer(const void *p) {
  hipPointerAttribute_t a{};
  if (hipPointerGetAttributes(&a, p) == hipSuccess && a.type == hipMemoryTypeHost && a.devicePointer) return a.devicePointer;
  (void)hipGetLastError(); // (pageable memory is reported as an error by some runtimes)
  return nullptr;
}

int ensure_batch_capacity(dsm_context *ctx, int nprob, int partial_stride) {
  if (nprob <= ctx->cap_prob && partial_stride <= ctx->partial_stride) return DSM_OK;
  const int cap = nprob > ctx->cap_prob ? nprob : ctx->cap_prob;
  const int ps = partial_stride > ctx->partial_stride ? partial_stride : ctx->partial_stride;
  int rc;
  if ((rc = realloc_dev(&ctx->d_tracker_ptrs, cap))) return rc;
  if ((rc = realloc_pinned(&ctx->h_tracker_ptrs, cap))) return rc;
  if ((rc = realloc_dev(&ctx->d_states, cap))) return rc;
  if ((rc = realloc_pinned(&ctx->h_states, cap))) return rc;
  if ((rc = realloc_dev(&ctx->d_partials, (size_t)cap * ps))) return rc;
  if ((rc = realloc_dev(&ctx->d_start, cap))) return rc;
  if ((rc = realloc_pinned(&ctx->h_start, cap))) return rc;
  if ((rc = realloc_dev(&ctx->d_single, cap))) return rc;
  if ((rc = realloc_pinned(&ctx->h_single, cap))) return rc;
  if ((rc = realloc_dev(&ctx->d_status, 2 * (size_t)cap))) return rc;
  if ((rc = realloc_pinned(&ctx->h_status, 2 * (size_t)cap))) return rc;
  if ((rc = realloc_dev(&ctx->d_rowmap, cap))) return rc;
  if ((rc = realloc_pinned(&ctx->h_rowmap, cap))) return rc;
  if ((rc = realloc_dev(&ctx->d_tickets, cap))) return rc;
  DSM_HIP(hipMemsetAsync(ctx->d_tickets, 0, sizeof(int) * cap, ctx->stream));
  DSM_HIP(hipMemsetAsync(ctx->d_states, 0, sizeof(LMState) * cap, ctx->stream));
  ctx->cap_prob = cap;
  ctx->partial_stride = ps;
  return DSM_OK;
}

int sync_desc(dsm_tracker *t) {
  if (!t->desc_dirty) return DSM_OK;
  DSM_HIP(hipMemcpyAsync(t->d_desc, &t->desc, sizeof(TrackerDev), hipMemcpyHostToDevice, t->ctx->stream));
  // the host copy may change again before the copy engine reads it
  DSM_HIP(hipStreamSynchronize(t->ctx->stream));
  t->desc_dirty = false;
  return DSM_OK;
}

// the same for a batch: all changed descriptors through one pinned staging buffer, one copy and one scatter launch
int sync_descs(dsm_context *ctx, dsm_tracker *const *ts, int n) {
  int dirty = 0;
  for (int i = 0; i < n; i++) dirty += ts[i]->desc_dirty ? 1 : 0;
  if (dirty <= 2) {
    for (int i = 0; i < n; i++) {
      int rc = sync_desc(ts[i]);
      if (rc) return rc;
    }
    return DSM_OK;
  }
  const size_t per = sizeof(TrackerDev) + sizeof(TrackerDev *);
  if (dirty > ctx->desc_stage_cap) {
    if (ctx->desc_stage_busy) DSM_HIP(hipEventSynchronize(ctx->desc_event));
    ctx->desc_stage_busy = false;
    int rc = realloc_dev(&ctx->d_desc_stage, per * dirty);
    if (rc) return rc;
    rc = realloc_pinned(&ctx->h_desc_stage, per * dirty);
    if (rc) return rc;
    ctx->desc_stage_cap = dirty;
  }
  if (!ctx->desc_event) DSM_HIP(hipEventCreateWithFlags(&ctx->desc_event, hipEventDisableTiming));
  if (ctx->desc_stage_busy) DSM_HIP(hipEventSynchronize(ctx->desc_event)); // the previous copy still reads the buffer
  TrackerDev *hd = (TrackerDev *)ctx->h_desc_stage;
  TrackerDev **hp = (TrackerDev **)(ctx->h_desc_stage + sizeof(TrackerDev) * dirty);
  int k = 0;
  for (int i = 0; i < n; i++) {
    if (!ts[i]->desc_dirty) continue;
    bool seen = false; // the same tracker twice in a batch (hypotheses)
    for (int j = 0; j < k && !seen; j++) seen = hp[j] == ts[i]->d_desc;
    if (seen) continue;
    hd[k] = ts[i]->desc;
    hp[k] = ts[i]->d_desc;
    k++;
  }
  DSM_HIP(hipMemcpyAsync(ctx->d_desc_stage, ctx->h_desc_stage, per * dirty, hipMemcpyHostToDevice, ctx->stream));
  launch_desc_scatter(ctx->stream, k, (const TrackerDev *)ctx->d_desc_stage,
                      (TrackerDev *const *)(ctx->d_desc_stage + sizeof(TrackerDev) * dirty));
  DSM_HIP(hipGetLastError());
  DSM_HIP(hipEventRecord(ctx->desc_event, ctx->stream));
  ctx->desc_stage_busy = true;
  for (int i = 0; i < n; i++) ts[i]->desc_dirty = false;
  return DSM_OK;
}

// ---- small host math (float, contraction off): makeK, TrackerAndScaler.cpp:117-141 ----
static float cof3(const float *m, int i, int j) {
  const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
  return m[i1 * 3 + j1] * m[i2 * 3 + j2] - m[i1 * 3 + j2] * m[i2 * 3 + j1];
}
static void mat3f_inverse(const float *m, float *r) { // Eigen Matrix3f::inverse(), cofactor form
  const float c0 = cof3(m, 0, 0), c1 = cof3(m, 1, 0), c2 = cof3(m, 2, 0);
  const float det = (c0 * m[0] + c1 * m[3]) + c2 * m[6];
  const float invdet = 1.0f / det;
  r[0] = c0 * invdet;
  r[1] = c1 * invdet;
  r[2] = c2 * invdet;
  r[3] = cof3(m, 0, 1) * invdet;
  r[4] = cof3(m, 1, 1) * invdet;
  r[5] = cof3(m, 2, 1) * invdet;
  r[6] = cof3(m, 0, 2) * invdet;
  r[7] = cof3(m, 1, 2) * invdet;
  r[8] = cof3(m, 2, 2) * invdet;
}

// SE3(Matrix4d) of Sophus/Eigen for tfm_f1_f0_ (TrackerAndScaler.cpp:82-86)
static void se3_from_matrix(const double T[16], double pose[7]) {
  const double M[3][3] = {{T[0], T[1], T[2]}, {T[4], T[5], T[6]}, {T[8], T[9], T[10]}};
  double q[4];
  double t = M[0][0] + M[1][1] + M[2][2];
  if (t > 0.0) {
    t = std::sqrt(t + 1.0);
    q[3] = 0.5 * t;
    t = 0.5 / t;
    q[0] = (M[2][1] - M[1][2]) * t;
    q[1] = (M[0][2] - M[2][0]) * t;
    q[2] = (M[1][0] - M[0][1]) * t;
  } else {
    int i = 0;
    if (M[1][1] > M[0][0]) i = 1;
    if (M[2][2] > M[i][i]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    t = std::sqrt(M[i][i] - M[j][j] - M[k][k] + 1.0);
    q[i] = 0.5 * t;
    t = 0.5 / t;
    q[3] = (M[k][j] - M[j][k]) * t;
    q[j] = (M[j][i] + M[i][j]) * t;
    q[k] = (M[k][i] + M[i][k]) * t;
  }
  const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  for (int i = 0; i < 4; i++) pose[i] = q[i] / n;
  pose[4] = T[3];
  pose[5] = T[7];
  pose[6] = T[11];
}

// ---- the device descriptor of a tracker, piece by piece (dsm_tracker_*; dsm_pose_estimate_batch builds its jobs' descriptors from the same pieces) ----
static void desc_init(TrackerDev &D, int nlevels, const dsm_params &P) {
  memset(&D, 0, sizeof D);
  D.nlevels = nlevels;
  D.p.huber_th = P.huber_th;
  D.p.coarse_cutoff_th = P.coarse_cutoff_th;
  D.p.scale_xi_rot = P.scale_xi_rot;
  D.p.scale_xi_trans = P.scale_xi_trans;
  D.p.scale_a = P.scale_a;
  D.p.scale_b = P.scale_b;
  D.p.affine_opt_mode_a = P.affine_opt_mode_a;
  D.p.affine_opt_mode_b = P.affine_opt_mode_b;
  D.p.lambda_extrapolation_limit = P.lambda_extrapolation_limit;
  for (int l = 0; l < DSM_MAX_LEVELS; l++) D.p.max_iterations[l] = P.max_iterations[l];
  D.p.fixed_schedule = P.fixed_schedule;
  D.p.geometry = P.chunk_geometry;
}
// camera 1 pyramid, TrackerAndScaler.cpp:89-98
static void desc_cam1(TrackerDev &D, int nlevels, const float K1[4]) {
  D.lv[0].fx1 = K1[0];
  D.lv[0].fy1 = K1[1];
  D.lv[0].cx1 = K1[2];
  D.lv[0].cy1 = K1[3];
  for (int l = 1; l < nlevels; l++) {
    D.lv[l].fx1 = D.lv[l - 1].fx1 * 0.5;
    D.lv[l].fy1 = D.lv[l - 1].fy1 * 0.5;
    D.lv[l].cx1 = (D.lv[0].cx1 + 0.5) / ((int)1 << l) - 0.5;
    D.lv[l].cy1 = (D.lv[0].cy1 + 0.5) / ((int)1 << l) - 0.5;
  }
}
// makeK, TrackerAndScaler.cpp:117-141
static void desc_make_k(TrackerDev &D, int nlevels, float fx, float fy, float cx, float cy) {
  D.lv[0].fx = fx;
  D.lv[0].fy = fy;
  D.lv[0].cx = cx;
  D.lv[0].cy = cy;
  for (int l = 1; l < nlevels; l++) { // :126-133
    D.lv[l].fx = D.lv[l - 1].fx * 0.5;
    D.lv[l].fy = D.lv[l - 1].fy * 0.5;
    D.lv[l].cx = (D.lv[0].cx + 0.5) / ((int)1 << l) - 0.5;
    D.lv[l].cy = (D.lv[0].cy + 0.5) / ((int)1 << l) - 0.5;
  }
  for (int l = 0; l < nlevels; l++) { // :135-140
    const float K[9] = {D.lv[l].fx, 0.0f, D.lv[l].cx, 0.0f, D.lv[l].fy, D.lv[l].cy, 0.0f, 0.0f, 1.0f};
    mat3f_inverse(K, D.lv[l].Ki);
  }
}

static int round8(int x) { return (x + 7) & ~7; }

// record an event pair around a launch when timing is on
struct EvSlot {
  hipEvent_t a, b;
  int lvl;
};

} // namespace dsm

using namespace dsm;

extern "C" {

const char *dsm_last_error(void) { return g_err.c_str(); }
int dsm_abi_version(void) { return DSM_ABI_VERSION; }

int dsm_params_default_sized(dsm_params *p, size_t caller_size) {
  if (!p || caller_size < sizeof(size_t)) return invalid("dsm_params_default_sized: null struct or a size below its first member");
  dsm_params d;
  dsm_params_default(&d);
  memcpy(p, &d, caller_size < sizeof d ? caller_size : sizeof d); // never past the end of the caller's struct
  p->struct_size = caller_size;
  if (caller_size != sizeof d) {
    set_error("dsm_params: the caller was built against another version of dsm_hotpath.h (sizeof(dsm_params) differs)");
    return DSM_ERR_INVALID;
  }
  return DSM_OK;
}

void dsm_params_default(dsm_params *p) {
  memset(p, 0, sizeof *p);
  p->struct_size = sizeof(dsm_params);
  p->huber_th = 9.0f;
  p->coarse_cutoff_th = 20.0f;
  p->scale_xi_rot = 1.0f;
  p->scale_xi_trans = 0.5f;
  p->scale_a = 10.0f;
  p->scale_b = 1000.0f;
  p->affine_opt_mode_a = 0.0f;
  p->affine_opt_mode_b = 0.0f;
  p->lambda_extrapolation_limit = 0.001f;
  const int it[DSM_MAX_LEVELS] = {10, 20, 50, 50, 50, 50};
  memcpy(p->max_iterations, it, sizeof it);
  p->adaptive_schedule = 1;
  p->persistent_coarse = 0;
  p->fuse_lm = 1;
  p->work_queue = 1;
  p->speculate = 1;
  p->compact_tail = 1;
  p->fixed_schedule = 0;
  p->chunk_geometry = 0;
  p->frame_check = 1;
  p->frame_grad_tol = 0.0f;
}

int dsm_context_create(int device_ordinal, dsm_context **out) {
  if (!out) return invalid("dsm_context_create: out is NULL");
  *out = nullptr;
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0) {
    set_error("no HIP device available: this library has no CPU fallback");
    return DSM_ERR_NO_DEVICE;
  }
  if (device_ordinal < 0 || device_ordinal >= ndev) return invalid("dsm_context_create: bad device ordinal");
  DSM_HIP(hipSetDevice(device_ordinal));
  dsm_context *ctx = new dsm_context();
  ctx->device = device_ordinal;
  hipError_t ce = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
  if (ce == hipSuccess) ce = hipEventCreate(&ctx->ev_total[0]);
  if (ce == hipSuccess) ce = hipEventCreate(&ctx->ev_total[1]);
  if (ce == hipSuccess) ce = hipEventCreateWithFlags(&ctx->fork_event, hipEventDisableTiming);
  if (ce == hipSuccess) ce = hipEventCreateWithFlags(&ctx->copy_event, hipEventDisableTiming);
  if (ce != hipSuccess) { // give back what was created
    dsm_context_destroy(ctx);
    DSM_HIP(ce);
  }
  *out = ctx;
  return DSM_OK;
}

int dsm_context_destroy(dsm_context *ctx) {
  if (!ctx) return DSM_OK;
  hipSetDevice(ctx->device);
  if (ctx->stream) hipStreamSynchronize(ctx->stream);
  hipFree(ctx->d_tracker_ptrs);
  hipHostFree(ctx->h_tracker_ptrs);
  hipFree(ctx->d_states);
  hipHostFree(ctx->h_states);
  hipFree(ctx->d_partials);
  hipFree(ctx->d_start);
  hipHostFree(ctx->h_start);
  hipFree(ctx->d_single);
  hipHostFree(ctx->h_single);
  hipFree(ctx->d_status);
  hipFree(ctx->d_rowmap);
  if (ctx->h_rowmap) hipHostFree(ctx->h_rowmap);
  hipFree(ctx->d_tickets);
  hipFree(ctx->d_queue);
  hipFree(ctx->d_qitems);
  hipHostFree(ctx->h_queue);
  hipHostFree(ctx->h_status);
  hipFree(ctx->d_stage);
  if (ctx->h_tpl_stage) hipHostFree(ctx->h_tpl_stage);
  CallArena::release(ctx);
  if (ctx->h_tpl_counts) hipHostFree(ctx->h_tpl_counts);
  for (hipEvent_t ev : ctx->ev_pool) hipEventDestroy(ev);
  for (hipEvent_t ev : ctx->join_events) hipEventDestroy(ev);
  if (ctx->companion_stream) hipStreamDestroy(ctx->companion_stream);
  if (ctx->companion_event) hipEventDestroy(ctx->companion_event);
  for (hipStream_t st : ctx->extra_streams) hipStreamDestroy(st);
  if (ctx->fork_event) hipEventDestroy(ctx->fork_event);
  if (ctx->copy_event) hipEventDestroy(ctx->copy_event);
  for (hipEvent_t ev : ctx->upload_events) hipEventDestroy(ev);
  if (ctx->desc_event) hipEventDestroy(ctx->desc_event);
  hipFree(ctx->d_desc_stage);
  hipHostFree(ctx->h_desc_stage);
  if (ctx->copy_stream) hipStreamDestroy(ctx->copy_stream);
  if (ctx->upload_stream) {
    hipStreamSynchronize(ctx->upload_stream);
    hipStreamDestroy(ctx->upload_stream);
    hipEventDestroy(ctx->upload_copies_event);
    hipEventDestroy(ctx->upload_done_event);
  }
  hipFree(ctx->d_pyr_jobs);
  hipHostFree(ctx->h_pyr_jobs);
  for (hipEvent_t ev : ctx->ev_total)
    if (ev) hipEventDestroy(ev);
  if (ctx->stream) hipStreamDestroy(ctx->stream);
  delete ctx;
  return DSM_OK;
}

int dsm_context_sync(dsm_context *ctx) {
  if (!ctx) return invalid("null context");
  DSM_HIP(hipStreamSynchronize(ctx->stream));
  return DSM_OK;
}
int dsm_context_set_timing(dsm_context *ctx, int enable) {
  if (!ctx) return invalid("null context");
  ctx->timing = enable != 0;
  return DSM_OK;
}
int dsm_context_set_streams(dsm_context *ctx, int n_streams) {
  if (!ctx || n_streams < 1 || n_streams > 16) return invalid("dsm_context_set_streams: 1..16");
  ctx->n_streams = n_streams;
  return DSM_OK;
}
int dsm_context_get_stats(dsm_context *ctx, dsm_stats *out) {
  if (!ctx || !out) return invalid("null argument");
  *out = ctx->stats;
  return DSM_OK;
}
void *dsm_context_stream(dsm_context *ctx) { return ctx ? (void *)ctx->stream : nullptr; }
int dsm_context_stream_queues(dsm_context *ctx, int *streams_out, int *sharing_out) {
  if (!ctx) return invalid("dsm_context_stream_queues: null context");
  if (streams_out) *streams_out = 1 + (int)ctx->extra_streams.size() + (ctx->companion_stream ? 1 : 0);
  if (sharing_out) *sharing_out = ctx->streams_sharing_a_queue;
  return DSM_OK;
}

// ---- tracker ------------------------------------------------------------------------------
static int tracker_create_fill(dsm_tracker *t, dsm_context *ctx, int w, int h, int nlevels, const double T_f1_f0[16],
                               const float K1[4], const dsm_params *params);

int dsm_tracker_create(dsm_context *ctx, int w, int h, int nlevels, const double T_f1_f0[16],
                       const float K1[4], const dsm_params *params, dsm_tracker **out) {
  if (!ctx || !out || !T_f1_f0 || !K1) return invalid("dsm_tracker_create: null argument");
  if (nlevels < 1 || nlevels > DSM_MAX_LEVELS) return invalid("dsm_tracker_create: nlevels out of range");
  if ((w >> (nlevels - 1)) < 8 || (h >> (nlevels - 1)) < 8) return invalid("dsm_tracker_create: image too small for nlevels");
  // the eval kernels address texels with 32-bit byte offsets (16 bytes per texel at most)
  if ((long long)w * h * 16 >= (1ll << 32)) return invalid("dsm_tracker_create: image too large");
  DSM_HIP(hipSetDevice(ctx->device));
  dsm_tracker *t = new dsm_tracker();
  const int rc = tracker_create_fill(t, ctx, w, h, nlevels, T_f1_f0, K1, params);
  if (rc != DSM_OK) { // e.g. out of device memory half way: give back what was allocated (hipFree(nullptr) is a no-op)
    const std::string keep = g_err;
    dsm_tracker_destroy(t);
    g_err = keep;
    return rc;
  }
  *out = t;
  return DSM_OK;
}

// the caller's parameters, checked, or the defaults
static int take_params(const dsm_params *params, dsm_params *out) {
  if (params) {
    if (params->struct_size != sizeof(dsm_params))
      return invalid("dsm_params.struct_size does not match this library's dsm_params: the caller was built against another "
                     "version of dsm_hotpath.h (use dsm_params_default, compare dsm_abi_version() with DSM_ABI_VERSION)");
    if (params->chunk_geometry < 0 || params->chunk_geometry > 2)
      return invalid("dsm_params.chunk_geometry: 0 (throughput table), 1 (latency table) or 2 (latency table, one chunk up to 4096 points)");
    *out = *params;
  } else {
    dsm_params_default(out);
  }
  return DSM_OK;
}

static int tracker_create_fill(dsm_tracker *t, dsm_context *ctx, int w, int h, int nlevels, const double T_f1_f0[16],
                               const float K1[4], const dsm_params *params) {
  t->ctx = ctx;
  t->w = w;
  t->h = h;
  t->nlevels = nlevels;
  const int prc = take_params(params, &t->params);
  if (prc) return prc;
  TrackerDev &D = t->desc;
  desc_init(D, nlevels, t->params);
  se3_from_matrix(T_f1_f0, D.T10);
  for (int l = 0; l < nlevels; l++) { // TrackerAndScaler.cpp:52-64
    const int wl = w >> l, hl = h >> l;
    D.lv[l].w = wl;
    D.lv[l].h = hl;
    DSM_HIP(hipMalloc(&t->d_pts[l], sizeof(float4) * ((size_t)wl * hl + kTemplatePad)));
    DSM_HIP(hipMemsetAsync(t->d_pts[l], 0, sizeof(float4) * ((size_t)wl * hl + kTemplatePad), ctx->stream)); // (not the null stream: streams_overlap)
    t->pts_cap[l] = wl * hl;
    for (int s = 0; s < 2; s++) {
      DSM_HIP(hipMalloc(&t->d_img[s][l], plane_bytes(wl, hl)));
      DSM_HIP(hipMemsetAsync(t->d_img[s][l], 0, plane_bytes(wl, hl), ctx->stream));
      D.lv[l].img[s] = t->d_img[s][l];
    }
    D.lv[l].pts = t->d_pts[l];
    D.lv[l].n = 0;
  }
  desc_cam1(D, nlevels, K1);
  DSM_HIP(hipMalloc(&t->d_desc, sizeof(TrackerDev)));
  t->desc_dirty = true;
  DSM_HIP(hipStreamSynchronize(ctx->stream)); // the zero fills are through before any other stream may write these buffers
  return DSM_OK;
}

int dsm_tracker_destroy(dsm_tracker *t) {
  if (!t) return DSM_OK;
  hipSetDevice(t->ctx->device);
  hipStreamSynchronize(t->ctx->stream);
  if (t->ctx->upload_stream) hipStreamSynchronize(t->ctx->upload_stream); // an asynchronous hand-over may still write its buffers
  if (t->ctx->copy_stream) hipStreamSynchronize(t->ctx->copy_stream);
  for (int l = 0; l < t->nlevels; l++) {
    hipFree(t->d_pts[l]);
    hipFree(t->d_img[0][l]);
    hipFree(t->d_img[1][l]);
  }
  hipFree(t->d_raw[0]);
  hipFree(t->d_raw[1]);
  for (int s = 0; s < 2; s++) {
    hipFree(t->d_raw_back[s]);
    for (int l = 0; l < DSM_MAX_LEVELS; l++) hipFree(t->d_img_back[s][l]);
  }
  hipFree(t->d_desc);
  delete t;
  return DSM_OK;
}

int dsm_tracker_make_k(dsm_tracker *t, float fx, float fy, float cx, float cy) {
  if (!t) return invalid("null tracker");
  desc_make_k(t->desc, t->nlevels, fx, fy, cx, cy);
  t->have_k = true;
  t->desc_dirty = true;
  return DSM_OK;
}

int dsm_tracker_set_ref(dsm_tracker *t, int ref_frame_id, double ref_aff_a, double ref_aff_b,
                        float ref_exposure, const int *n, const float *const *pc_u,
                        const float *const *pc_v, const float *const *pc_idepth,
                        const float *const *pc_color) {
  if (!t || !n || !pc_u || !pc_v || !pc_idepth || !pc_color) return invalid("dsm_tracker_set_ref: null argument");
  dsm_context *ctx = t->ctx;
  DSM_HIP(hipSetDevice(ctx->device));
  for (int l = 0; l < t->nlevels; l++)
    if (n[l] < 0 || n[l] > t->pts_cap[l]) return invalid("dsm_tracker_set_ref: n[lvl] out of range");
  int rc = ensure_stage(ctx, 4 * (size_t)t->w * t->h);
  if (rc) return rc;
  for (int l = 0; l < t->nlevels; l++) {
    const size_t nl = n[l];
    float *su = ctx->d_stage, *sv = su + nl, *si = sv + nl, *sc = si + nl;
    if (nl) {
      DSM_HIP(hipMemcpyAsync(su, pc_u[l], nl * 4, hipMemcpyHostToDevice, ctx->stream));
      DSM_HIP(hipMemcpyAsync(sv, pc_v[l], nl * 4, hipMemcpyHostToDevice, ctx->stream));
      DSM_HIP(hipMemcpyAsync(si, pc_idepth[l], nl * 4, hipMemcpyHostToDevice, ctx->stream));
      DSM_HIP(hipMemcpyAsync(sc, pc_color[l], nl * 4, hipMemcpyHostToDevice, ctx->stream));
      launch_interleave_template(ctx->stream, (int)nl, su, sv, si, sc, t->d_pts[l]);
    }
    DSM_HIP(hipStreamSynchronize(ctx->stream)); // staging buffer is reused by the next level
    t->desc.lv[l].n = (int)nl;
  }
  t->desc.ref_a = ref_aff_a; // :323-324
  t->desc.ref_b = ref_aff_b;
  t->desc.ref_exposure = ref_exposure;
  t->ref_frame_id = ref_frame_id;
  t->have_ref = true;
  t->desc_dirty = true;
  return DSM_OK;
}

int dsm_set_refs_from_points(dsm_context *ctx, int n_jobs, const dsm_ref_job *jobs) {
  if (!ctx || n_jobs < 0 || (n_jobs && !jobs)) return invalid("dsm_set_refs_from_points: bad argument");
  if (!n_jobs) return DSM_OK;
  DSM_HIP(hipSetDevice(ctx->device));
  std::vector<size_t> off((size_t)n_jobs + 1, 0);
  for (int j = 0; j < n_jobs; j++) {
    const dsm_ref_job &J = jobs[j];
    dsm_tracker *t = J.t, *fo = J.frame_owner;
    if (!t || !fo || J.slot < 0 || J.slot > 1 || J.npts < 0 || (J.npts > 0 && (!J.pu || !J.pv || !J.pidepth || !J.pweight)))
      return invalid("dsm_tracker_set_ref_from_points: bad argument");
    if (t->ctx != ctx || fo->ctx != ctx || fo->w != t->w || fo->h != t->h || fo->nlevels != t->nlevels)
      return invalid("dsm_tracker_set_ref_from_points: the frame owner must share context, size and levels");
    if (!fo->have_frame[J.slot]) {
      set_error("dsm_tracker_set_ref_from_points: the keyframe's pyramid has not been uploaded to that slot");
      return DSM_ERR_STATE;
    }
    for (int l = 0; l < t->nlevels; l++)
      if ((long long)((t->w >> l) - 4) * ((t->h >> l) - 4) > t->pts_cap[l]) return invalid("template capacity too small");
    for (int k = 0; k < j; k++)
      if (jobs[k].t == t) return invalid("dsm_set_refs_from_points: a tracker takes one reference per call");
    const size_t floats = make_coarse_depth_workspace_floats(t->w, t->h, t->nlevels, J.npts);
    off[j + 1] = off[j] + ((floats + 63) & ~(size_t)63);
  }
  // ONE launch sequence for all jobs (template_kernels.hip: blockIdx.y = job), ONE host->device copy for their points and the job table
  // (staged in page-locked memory), ONE copy back for their counts.  Device layout of the staging area: [workspaces | points | counts |
  // job table]; the pinned mirror holds [points | job table] and, separately, the counts.
  dsm_tracker *t0 = jobs[0].t;
  for (int j = 1; j < n_jobs; j++)
    if (jobs[j].t->w != t0->w || jobs[j].t->h != t0->h || jobs[j].t->nlevels != t0->nlevels)
      return invalid("dsm_set_refs_from_points: trackers of different geometry in one call");
  std::vector<size_t> poff((size_t)n_jobs + 1, 0);
  int max_npts = 0;
  for (int j = 0; j < n_jobs; j++) {
    poff[j + 1] = poff[j] + ((4 * (size_t)jobs[j].npts + 3) & ~(size_t)3);
    if (jobs[j].npts > max_npts) max_npts = jobs[j].npts;
  }
  const size_t ws_floats = off[n_jobs], pt_floats = poff[n_jobs], cnt_floats = ((size_t)n_jobs * (DSM_MAX_LEVELS + 2) + 3) & ~(size_t)3;
  const size_t tab_floats = (sizeof(TplJob) * (size_t)n_jobs + 3) / 4;
  int rc = ensure_stage(ctx, ws_floats + pt_floats + cnt_floats + tab_floats + 16);
  if (rc) return rc;
  const size_t host_floats = pt_floats + tab_floats + 16;
  if (host_floats > ctx->tpl_stage_floats) {
    if (ctx->h_tpl_stage) DSM_HIP(hipHostFree(ctx->h_tpl_stage));
    ctx->h_tpl_stage = nullptr, ctx->tpl_stage_floats = 0;
    DSM_HIP(hipHostMalloc(&ctx->h_tpl_stage, sizeof(float) * host_floats * 2, hipHostMallocDefault));
    ctx->tpl_stage_floats = host_floats * 2;
  }
  if ((size_t)n_jobs * (DSM_MAX_LEVELS + 2) > ctx->tpl_counts_cap) {
    if (ctx->h_tpl_counts) DSM_HIP(hipHostFree(ctx->h_tpl_counts));
    ctx->h_tpl_counts = nullptr, ctx->tpl_counts_cap = 0;
    DSM_HIP(hipHostMalloc(&ctx->h_tpl_counts, sizeof(int) * (size_t)n_jobs * (DSM_MAX_LEVELS + 2) * 2, hipHostMallocDefault));
    ctx->tpl_counts_cap = (size_t)n_jobs * (DSM_MAX_LEVELS + 2) * 2;
  }
  float *d_ws = ctx->d_stage, *d_pt = d_ws + ws_floats;
  int *d_cnt = (int *)(d_pt + pt_floats);
  TplJob *d_tab = (TplJob *)((float *)d_cnt + cnt_floats);
  float *h_pt = ctx->h_tpl_stage;
  TplJob *h_tab = (TplJob *)(h_pt + pt_floats);
  for (int j = 0; j < n_jobs; j++) {
    const dsm_ref_job &J = jobs[j];
    dsm_tracker *t = J.t;
    t->have_ref = false; // (until its counts are back)
    const size_t np_ = (size_t)J.npts;
    float *hp = h_pt + poff[j];
    if (np_) {
      memcpy(hp, J.pu, sizeof(float) * np_);
      memcpy(hp + np_, J.pv, sizeof(float) * np_);
      memcpy(hp + 2 * np_, J.pidepth, sizeof(float) * np_);
      memcpy(hp + 3 * np_, J.pweight, sizeof(float) * np_);
    }
    TplJob &T = h_tab[j];
    memset(&T, 0, sizeof T);
    T.npts = J.npts;
    T.pt = d_pt + poff[j];
    T.ws = d_ws + off[j];
    T.d_n = d_cnt + (size_t)j * (DSM_MAX_LEVELS + 2);
    for (int l = 0; l < t->nlevels; l++) T.ref[l] = J.frame_owner->d_img[J.slot][l], T.pts[l] = t->d_pts[l];
  }
  // (points and job table are contiguous in the pinned mirror and on the device up to the counts in between: two copies)
  if (pt_floats) DSM_HIP(hipMemcpyAsync(d_pt, h_pt, sizeof(float) * pt_floats, hipMemcpyHostToDevice, ctx->stream));
  DSM_HIP(hipMemcpyAsync(d_tab, h_tab, sizeof(TplJob) * (size_t)n_jobs, hipMemcpyHostToDevice, ctx->stream));
  launch_make_coarse_depth(ctx->stream, t0->w, t0->h, t0->nlevels, d_tab, n_jobs, max_npts, kTexel);
  DSM_HIP(hipGetLastError());
  int *h_cnt = ctx->h_tpl_counts;
  DSM_HIP(hipMemcpyAsync(h_cnt, d_cnt, sizeof(int) * (size_t)n_jobs * (DSM_MAX_LEVELS + 2), hipMemcpyDeviceToHost, ctx->stream));
  DSM_HIP(hipStreamSynchronize(ctx->stream));
  std::vector<int> h_n((size_t)n_jobs * (DSM_MAX_LEVELS + 1), 0);
  for (int j = 0; j < n_jobs; j++)
    for (int l = 0; l <= jobs[j].t->nlevels; l++) h_n[(size_t)j * (DSM_MAX_LEVELS + 1) + l] = h_cnt[(size_t)j * (DSM_MAX_LEVELS + 2) + l];
  for (int j = 0; j < n_jobs; j++)
    if (h_n[(size_t)j * (DSM_MAX_LEVELS + 1) + jobs[j].t->nlevels]) // a point projected outside the image: the reference would corrupt memory (:160)
      return invalid("dsm_tracker_set_ref_from_points: point outside the level-0 image");
  for (int j = 0; j < n_jobs; j++) {
    const dsm_ref_job &J = jobs[j];
    dsm_tracker *t = J.t;
    const int *hn = h_n.data() + (size_t)j * (DSM_MAX_LEVELS + 1);
    for (int l = 0; l < t->nlevels; l++) {
      t->desc.lv[l].n = hn[l];
      if (J.n_out) J.n_out[l] = hn[l];
    }
    t->desc.ref_a = J.ref_aff_a; // :323-324
    t->desc.ref_b = J.ref_aff_b;
    t->desc.ref_exposure = J.ref_exposure;
    t->ref_frame_id = J.ref_frame_id;
    t->have_ref = true;
    t->desc_dirty = true;
  }
  return DSM_OK;
}

int dsm_tracker_set_ref_from_points(dsm_tracker *t, dsm_tracker *frame_owner, int slot, int ref_frame_id, double ref_aff_a,
                                    double ref_aff_b, float ref_exposure, int npts, const float *pu, const float *pv,
                                    const float *pidepth, const float *pweight, int *n_out) {
  if (!t) return invalid("dsm_tracker_set_ref_from_points: bad argument");
  dsm_ref_job J;
  J.t = t, J.frame_owner = frame_owner, J.slot = slot, J.ref_frame_id = ref_frame_id, J.ref_aff_a = ref_aff_a, J.ref_aff_b = ref_aff_b;
  J.ref_exposure = ref_exposure, J.npts = npts, J.pu = pu, J.pv = pv, J.pidepth = pidepth, J.pweight = pweight, J.n_out = n_out;
  return dsm_set_refs_from_points(t->ctx, 1, &J);
}

int dsm_tracker_scale_depth(dsm_tracker *t, float scale) {
  if (!t) return invalid("null tracker");
  if (!t->have_ref) {
    set_error("dsm_tracker_scale_depth before set_ref");
    return DSM_ERR_STATE;
  }
  DSM_HIP(hipSetDevice(t->ctx->device));
  // one launch over all levels, enqueued on the context's stream and NOT waited for: everything that reads the template afterwards --
  // evaluations, the streaming form's advances (their stream groups fork from this stream), dsm_tracker_get_template -- is ordered
  // behind it there (eight keyframes' calls were 0.24 of the 1.9 ms between two advances of 128 concurrent sequences)
  ScaleDepthArgs a;
  a.nlevels = t->nlevels;
  int max_n = 0;
  for (int l = 0; l < t->nlevels; l++) {
    a.n[l] = t->desc.lv[l].n, a.pts[l] = t->d_pts[l];
    if (a.n[l] > max_n) max_n = a.n[l];
  }
  launch_scale_depth_levels(t->ctx->stream, a, max_n, scale);
  DSM_HIP(hipGetLastError());
  return DSM_OK;
}

int dsm_tracker_get_template(dsm_tracker *t, int lvl, int *n, float *pc_u, float *pc_v, float *pc_idepth,
                             float *pc_color) {
  if (!t || !n || lvl < 0 || lvl >= t->nlevels) return invalid("dsm_tracker_get_template: bad argument");
  dsm_context *ctx = t->ctx;
  DSM_HIP(hipSetDevice(ctx->device));
  const size_t nl = t->desc.lv[lvl].n;
  *n = (int)nl;
  if (!pc_u && !pc_v && !pc_idepth && !pc_color) return DSM_OK;
  if (!pc_u || !pc_v || !pc_idepth || !pc_color) return invalid("dsm_tracker_get_template: all four outputs or none");
  if (!nl) return DSM_OK;
  int rc = ensure_stage(ctx, 4 * nl);
  if (rc) return rc;
  float *su = ctx->d_stage, *sv = su + nl, *si = sv + nl, *sc = si + nl;
  launch_deinterleave_template(ctx->stream, (int)nl, t->d_pts[lvl], su, sv, si, sc);
  DSM_HIP(hipMemcpyAsync(pc_u, su, nl * 4, hipMemcpyDeviceToHost, ctx->stream));
  DSM_HIP(hipMemcpyAsync(pc_v, sv, nl * 4, hipMemcpyDeviceToHost, ctx->stream));
  DSM_HIP(hipMemcpyAsync(pc_idepth, si, nl * 4, hipMemcpyDeviceToHost, ctx->stream));
  DSM_HIP(hipMemcpyAsync(pc_color, sc, nl * 4, hipMemcpyDeviceToHost, ctx->stream));
  DSM_HIP(hipStreamSynchronize(ctx->stream));
  return DSM_OK;
}

int dsm_tracker_upload_frame(dsm_tracker *t, int slot, const float *const *dIp, float ab_exposure) {
  if (!t || !dIp || slot < 0 || slot > 1) return invalid("dsm_tracker_upload_frame: bad argument");
  dsm_context *ctx = t->ctx;
  DSM_HIP(hipSetDevice(ctx->device));
  // The device keeps channel 0 only; channels 1 and 2 must be what FrameHessian::makeImages derives
  // from it -- which is all the reference ever passes -- and that is checked (dsm_params.frame_check, frame_grad_tol), not
  // assumed: per level the number of offending texels and the first of them.
  const size_t npx0 = (size_t)t->w * t->h;
  int rc = ensure_stage(ctx, 3 * npx0 + 4 * DSM_MAX_LEVELS);
  if (rc) return rc;
  int *d_bad = (int *)(ctx->d_stage + 3 * npx0); // [level]{count, first index}
  int h_bad[2 * DSM_MAX_LEVELS];
  for (int l = 0; l < DSM_MAX_LEVELS; l++) h_bad[2 * l] = 0, h_bad[2 * l + 1] = 0x7FFFFFFF;
  const bool check = t->params.frame_check != 0;
  if (check) DSM_HIP(hipMemcpyAsync(d_bad, h_bad, sizeof h_bad, hipMemcpyHostToDevice, ctx->stream));
  for (int l = 0; l < t->nlevels; l++) {
    const int wl = t->w >> l, hl = t->h >> l;
    DSM_HIP(hipMemcpyAsync(ctx->d_stage, dIp[l], (size_t)wl * hl * 12, hipMemcpyHostToDevice, ctx->stream));
    launch_dip_import(ctx->stream, wl, hl, ctx->d_stage, t->d_img[slot][l], check ? d_bad + 2 * l : nullptr, t->params.frame_grad_tol);
  }
  if (check) DSM_HIP(hipMemcpyAsync(h_bad, d_bad, sizeof h_bad, hipMemcpyDeviceToHost, ctx->stream));
  DSM_HIP(hipStreamSynchronize(ctx->stream));
  for (int l = 0; check && l < t->nlevels; l++)
    if (h_bad[2 * l]) {
      t->have_frame[slot] = false;
      const int wl = t->w >> l, idx = h_bad[2 * l + 1];
      char msg[320];
      snprintf(msg, sizeof msg,
               "dsm_tracker_upload_frame: level %d: %d texel(s) whose gradient channels are not the central differences of channel 0 "
               "(makeImages), the first at index %d (x = %d, y = %d); see dsm_params.frame_check / frame_grad_tol",
               l, h_bad[2 * l], idx, idx % wl, idx / wl);
      return invalid(msg);
    }
  t->desc.exposure[slot] = ab_exposure;
  t->have_frame[slot] = true;
  t->desc_dirty = true;
  return DSM_OK;
}

int dsm_tracker_upload_intensity(dsm_tracker *t, int slot, const float *const *I, float ab_exposure) {
  if (!t || !I || slot < 0 || slot > 1) return invalid("dsm_tracker_upload_intensity: bad argument");
  dsm_context *ctx = t->ctx;
  DSM_HIP(hipSetDevice(ctx->device));
  for (int l = 0; l < t->nlevels; l++) {
    if (!I[l]) return invalid("dsm_tracker_upload_intensity: null level");
    DSM_HIP(hipMemcpyAsync(t->d_img[slot][l], I[l], sizeof(float) * (size_t)(t->w >> l) * (t->h >> l), hipMemcpyHostToDevice, ctx->stream));
  }
  DSM_HIP(hipStreamSynchronize(ctx->stream));
  t->desc.exposure[slot] = ab_exposure;
  t->have_frame[slot] = true;
  t->desc_dirty = true;
  return DSM_OK;
}

int dsm_tracker_upload_image(dsm_tracker *t, int slot, const float *image, float ab_exposure) {
  if (!t || !image || slot < 0 || slot > 1) return invalid("dsm_tracker_upload_image: bad argument");
  dsm_context *ctx = t->ctx;
  DSM_HIP(hipSetDevice(ctx->device));
  const size_t npx0 = (size_t)t->w * t->h;
  // the raw image is staged in a buffer of this tracker and slot, so that nothing but the host->device copy has to finish
  // before the call returns (the caller's buffer is free again); the pyramid kernels run on behind it.  With a pinned
  // caller buffer (dsm_host_alloc) the copy is a straight DMA.
  if (!t->d_raw[slot]) DSM_HIP(hipMalloc(&t->d_raw[slot], npx0 * sizeof(float)));
  DSM_HIP(hipMemcpyAsync(t->d_raw[slot], image, npx0 * 4, hipMemcpyHostToDevice, ctx->stream));
  DSM_HIP(hipEventRecord(ctx->copy_event, ctx->stream));
  launch_pyramid(ctx->stream, t->w, t->h, t->nlevels, t->d_raw[slot], t->d_img[slot]);
  DSM_HIP(hipGetLastError());
  DSM_HIP(hipEventSynchronize(ctx->copy_event));
  t->desc.exposure[slot] = ab_exposure;
  t->have_frame[slot] = true;
  t->desc_dirty = true;
  return DSM_OK;
}

// Target buffers of a hand-over: the frame slot itself (0, 1) or its back buffers (DSM_SLOT_NEXT_*), which
// dsm_frames_advance later swaps in.  Back buffers are allocated on first use.
// raw_bytes: what the staged image needs; more than the 4 w h bytes of a level-0 float image (raw camera bytes of a larger
// camera, dsm_upload_images_undistorted) grows the staging buffer once
static int upload_target(dsm_tracker *t, int slot, float **raw, float **img, size_t raw_bytes) {
  const size_t npx0 = (size_t)t->w * t->h;
  const int s = slot & 1;
  const bool back = slot >= 2;
  if (raw_bytes > npx0 * sizeof(float)) {
    float *&buf = back ? t->d_raw_back[s] : t->d_raw[s];
    size_t &cap = back ? t->raw_back_bytes[s] : t->raw_bytes[s];
    if (buf && cap < raw_bytes) {
      // the pyramid kernels of an earlier hand-over may still read it
      dsm_context *ctx = t->ctx;
      DSM_HIP(hipStreamSynchronize(ctx->stream));
      if (ctx->upload_stream) DSM_HIP(hipStreamSynchronize(ctx->upload_stream));
      if (ctx->copy_stream) DSM_HIP(hipStreamSynchronize(ctx->copy_stream));
      DSM_HIP(hipFree(buf));
      buf = nullptr;
    }
    if (!buf) {
      DSM_HIP(hipMalloc(&buf, raw_bytes));
      cap = raw_bytes;
    }
  }
  if (back) {
    for (int l = 0; l < t->nlevels; l++)
      if (!t->d_img_back[s][l]) {
        DSM_HIP(hipMalloc(&t->d_img_back[s][l], plane_bytes(t->w >> l, t->h >> l)));
        DSM_HIP(hipMemsetAsync(t->d_img_back[s][l], 0, plane_bytes(t->w >> l, t->h >> l), t->ctx->stream));
      }
    if (!t->d_raw_back[s]) DSM_HIP(hipMalloc(&t->d_raw_back[s], npx0 * sizeof(float)));
  } else if (!t->d_raw[s]) {
    DSM_HIP(hipMalloc(&t->d_raw[s], npx0 * sizeof(float)));
  }
  *raw = back ? t->d_raw_back[s] : t->d_raw[s];
  for (int l = 0; l < DSM_MAX_LEVELS; l++) img[l] = l < t->nlevels ? (back ? t->d_img_back[s][l] : t->d_img[s][l]) : nullptr;
  return DSM_OK;
}

static void upload_mark(dsm_tracker *t, int slot, float exposure) {
  if (slot >= 2) {
    t->have_back[slot & 1] = true;
    t->back_exposure[slot & 1] = exposure;
  } else {
    t->desc.exposure[slot] = exposure;
    t->have_frame[slot] = true;
    t->desc_dirty = true;
  }
}

// async = false: copies and pyramids ordered on the context's stream, returns when the copies are through.
// async = true: everything on the context's upload stream, returns at once; dsm_upload_wait waits for the copies.
// und != null (dsm_upload_images_undistorted): the images are und's raw w_in x h_in camera bytes, staged as they are; level
// 0 is their undistortion.
static int upload_images_impl(dsm_context *ctx, int n, dsm_tracker *const *trackers, const int *slots, const void *const *images,
                              const float *ab_exposures, int pixel_type, size_t row_pitch_bytes, bool async, bool nowait = false,
                              const dsm_undistorter *und = nullptr) {
  if (!ctx || n < 0 || (n > 0 && (!trackers || !slots || !images)))
    return invalid("dsm_upload_images: bad argument");
  if (pixel_type != DSM_PIXEL_F32 && pixel_type != DSM_PIXEL_U8) return invalid("dsm_upload_images: bad pixel type");
  if (n == 0) return DSM_OK;
  DSM_HIP(hipSetDevice(ctx->device));
  const size_t px = pixel_type == DSM_PIXEL_U8 ? 1 : 4;
  const dsm_tracker *t0 = trackers[0];
  for (int i = 0; i < n; i++) {
    const dsm_tracker *t = trackers[i];
    if (!t || !images[i] || slots[i] < 0 || slots[i] > 3) return invalid("dsm_upload_images: bad entry");
    if (t->ctx != ctx) return invalid("dsm_upload_images: tracker of another context");
    if (t->w != t0->w || t->h != t0->h || t->nlevels != t0->nlevels)
      return invalid("dsm_upload_images: trackers of different geometry in one call");
    if (und && (t->w != und->tab.w_out || t->h != und->tab.h_out))
      return invalid("dsm_upload_images_undistorted: tracker size differs from the undistorter's output size");
    for (int j = 0; j < i; j++)
      if (trackers[j] == t && slots[j] == slots[i]) return invalid("dsm_upload_images: the same slot twice");
  }
  // the staged source image: und's camera bytes, else level-0 pixels of the trackers' size
  const int src_w = und ? und->tab.w_in : t0->w, src_h = und ? und->tab.h_in : t0->h;
  const size_t row = (size_t)src_w * px;
  if (row_pitch_bytes != 0 && row_pitch_bytes < row) return invalid("dsm_upload_images: row pitch smaller than a row");
  if (!ctx->copy_stream) DSM_HIP(hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
  if (async && !ctx->upload_stream) {
    DSM_HIP(hipStreamCreateWithFlags(&ctx->upload_stream, hipStreamNonBlocking));
    DSM_HIP(hipEventCreateWithFlags(&ctx->upload_copies_event, hipEventDisableTiming));
    DSM_HIP(hipEventCreateWithFlags(&ctx->upload_done_event, hipEventDisableTiming));
  }
  // the job table and the caller's buffers of the previous asynchronous hand-over are still being read until its
  // copies are through
  if (ctx->upload_pending) {
    DSM_HIP(hipEventSynchronize(ctx->upload_copies_event));
    ctx->upload_pending = false;
  }
  if (ctx->enqueue_pending) { // (dsm_upload_images_enqueue: its copy kernel still reads the job table and the caller's buffers)
    DSM_HIP(hipEventSynchronize(ctx->copy_event));
    ctx->enqueue_pending = false;
  }
  if (n > ctx->pyr_jobs_cap) {
    if (ctx->upload_stream) DSM_HIP(hipStreamSynchronize(ctx->upload_stream)); // pyramid kernels read the old table
    DSM_HIP(hipStreamSynchronize(ctx->stream));
    int rc = realloc_dev(&ctx->d_pyr_jobs, (size_t)n);
    if (rc) return rc;
    rc = realloc_pinned(&ctx->h_pyr_jobs, (size_t)n);
    if (rc) return rc;
    ctx->pyr_jobs_cap = n;
  }
  const size_t npx0 = (size_t)src_w * src_h;
  const size_t pitch = row_pitch_bytes ? row_pitch_bytes : row;
  // pinned caller buffers (dsm_host_alloc, hipHostMalloc, hipHostRegister) are read by the GPU directly
  bool all_pinned = true;
  uintptr_t align = (uintptr_t)row | (uintptr_t)pitch;
  for (int i = 0; i < n; i++) {
    float *raw = nullptr;
    int rc = upload_target(trackers[i], slots[i], &raw, ctx->h_pyr_jobs[i].img, npx0 * px);
    if (rc) return rc;
    ctx->h_pyr_jobs[i].raw = raw;
    ctx->h_pyr_jobs[i].src = nullptr;
    if (all_pinned) {
      hipPointerAttribute_t attr{};
      if (hipPointerGetAttributes(&attr, images[i]) == hipSuccess && attr.type == hipMemoryTypeHost && attr.devicePointer) {
        ctx->h_pyr_jobs[i].src = attr.devicePointer;
        align |= (uintptr_t)attr.devicePointer;
      } else {
        (void)hipGetLastError(); // pageable memory: not an error
        all_pinned = false;
      }
    }
  }
  const hipStream_t work = async ? ctx->upload_stream : ctx->stream; // job table, copy kernel, pyramid kernels
  const bool u8 = pixel_type == DSM_PIXEL_U8;
  // the job table of the previous hand-over may still be read by its pyramid kernels on the other work stream
  if (async) {
    DSM_HIP(hipEventRecord(ctx->copy_event, ctx->stream));
    DSM_HIP(hipStreamWaitEvent(work, ctx->copy_event, 0));
  } else if (ctx->upload_stream) {
    DSM_HIP(hipStreamWaitEvent(work, ctx->upload_done_event, 0));
  }
  if (all_pinned) {
    const int unit = (align & 15) == 0 ? 16 : (align & 3) == 0 ? 4 : 1;
    DSM_HIP(hipMemcpyAsync(ctx->d_pyr_jobs, ctx->h_pyr_jobs, sizeof(dsm::PyrJob) * n, hipMemcpyHostToDevice, work));
    // asynchronous: few workgroups, so that the host reads (microseconds of latency each) do not sit in the memory
    // pipelines of the CUs the tracking kernels run on
    launch_host_rows_copy(work, ctx->d_pyr_jobs, n, (int)row, src_h, pitch, unit, async ? ctx->async_copy_blocks : 1 << 20);
    DSM_HIP(hipGetLastError());
    DSM_HIP(hipEventRecord(async ? ctx->upload_copies_event : ctx->copy_event, work));
    if (und)
      launch_undistort_pyramid_batched(work, und->tab, t0->nlevels, ctx->d_pyr_jobs, n);
    else
      launch_pyramid_batched(work, t0->w, t0->h, t0->nlevels, ctx->d_pyr_jobs, n, u8);
    DSM_HIP(hipGetLastError());
    if (!async && nowait)
      ctx->enqueue_pending = true; // (waited for by the next hand-over or dsm_upload_wait)
    else if (!async)
      DSM_HIP(hipEventSynchronize(ctx->copy_event)); // the caller's buffers are free; the pyramid kernels run on behind
  } else {
    // the staging buffers may still be read by the pyramid kernels of the previous hand-over
    DSM_HIP(hipEventRecord(ctx->copy_event, work));
    DSM_HIP(hipStreamWaitEvent(ctx->copy_stream, ctx->copy_event, 0));
    DSM_HIP(hipMemcpyAsync(ctx->d_pyr_jobs, ctx->h_pyr_jobs, sizeof(dsm::PyrJob) * n, hipMemcpyHostToDevice, ctx->copy_stream));
    // groups: the pyramids of one group are built under the copies of the next
    const int group = 16;
    const int ngroups = (n + group - 1) / group;
    while ((int)ctx->upload_events.size() < ngroups) {
      hipEvent_t ev;
      DSM_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
      ctx->upload_events.push_back(ev);
    }
    for (int g = 0; g < ngroups; g++) {
      const int i0 = g * group, i1 = i0 + group < n ? i0 + group : n;
      for (int i = i0; i < i1; i++) {
        void *dst = const_cast<void *>(ctx->h_pyr_jobs[i].raw);
        if (pitch == row)
          DSM_HIP(hipMemcpyAsync(dst, images[i], npx0 * px, hipMemcpyHostToDevice, ctx->copy_stream));
        else
          DSM_HIP(hipMemcpy2DAsync(dst, row, images[i], pitch, row, (size_t)src_h, hipMemcpyHostToDevice, ctx->copy_stream));
      }
      DSM_HIP(hipEventRecord(ctx->upload_events[g], ctx->copy_stream));
      DSM_HIP(hipStreamWaitEvent(work, ctx->upload_events[g], 0));
      if (und)
        launch_undistort_pyramid_batched(work, und->tab, t0->nlevels, ctx->d_pyr_jobs + i0, i1 - i0);
      else
        launch_pyramid_batched(work, t0->w, t0->h, t0->nlevels, ctx->d_pyr_jobs + i0, i1 - i0, u8);
      DSM_HIP(hipGetLastError());
    }
    if (async)
      DSM_HIP(hipEventRecord(ctx->upload_copies_event, ctx->copy_stream));
    else
      DSM_HIP(hipStreamSynchronize(ctx->copy_stream)); // the caller's buffers are free; the pyramid kernels run on behind
  }
  if (async) {
    DSM_HIP(hipEventRecord(ctx->upload_done_event, work));
    ctx->upload_pending = true;
  }
  for (int i = 0; i < n; i++) upload_mark(trackers[i], slots[i], ab_exposures ? ab_exposures[i] : 1.0f);
  return DSM_OK;
}

int dsm_upload_images(dsm_context *ctx, int n, dsm_tracker *const *trackers, const int *slots, const void *const *images,
                      const float *ab_exposures, int pixel_type, size_t row_pitch_bytes) {
  return upload_images_impl(ctx, n, trackers, slots, images, ab_exposures, pixel_type, row_pitch_bytes, false);
}

int dsm_upload_images_async(dsm_context *ctx, int n, dsm_tracker *const *trackers, const int *slots, const void *const *images,
                            const float *ab_exposures, int pixel_type, size_t row_pitch_bytes) {
  return upload_images_impl(ctx, n, trackers, slots, images, ab_exposures, pixel_type, row_pitch_bytes, true);
}

int dsm_upload_images_enqueue(dsm_context *ctx, int n, dsm_tracker *const *trackers, const int *slots, const void *const *images,
                              const float *ab_exposures, int pixel_type, size_t row_pitch_bytes) {
  for (int i = 0; trackers && slots && i < n; i++)
    if (slots[i] > 1) return invalid("dsm_upload_images_enqueue: front buffers only (slots 0 / 1)");
  return upload_images_impl(ctx, n, trackers, slots, images, ab_exposures, pixel_type, row_pitch_bytes, false, true);
}

int dsm_undistorter_create(dsm_context *ctx, int w_in, int h_in, int w_out, int h_out, const float *remap_x, const float *remap_y,
                           const float *G, const float *vignette_inv, dsm_undistorter **out) {
  if (!ctx || !out) return invalid("dsm_undistorter_create: null argument");
  *out = nullptr;
  if (w_in < 2 || h_in < 2 || w_out < 1 || h_out < 1 || (long long)w_in * h_in >= (1ll << 31) || (long long)w_out * h_out >= (1ll << 31))
    return invalid("dsm_undistorter_create: bad image size");
  if (!remap_x != !remap_y) return invalid("dsm_undistorter_create: remap_x and remap_y are both given or both NULL");
  const bool pass = !remap_x;
  if (pass && (w_out != w_in || h_out != h_in)) return invalid("dsm_undistorter_create: passthrough requires the input size");
  const size_t n_out = (size_t)w_out * h_out, n_in = (size_t)w_in * h_in;
  std::vector<float2> remap;
  if (!pass) {
    // every entry outside (x < 0) or with its whole bilinear footprint inside: xi + 1 <= w_in - 1, yi + 1 <= h_in - 1
    remap.resize(n_out);
    const float wm1 = (float)(w_in - 1), hm1 = (float)(h_in - 1);
    for (size_t i = 0; i < n_out; i++) {
      const float x = remap_x[i], y = remap_y[i];
      if (!(x < 0) && !(x >= 0 && x < wm1 && y >= 0 && y < hm1)) {
        char msg[256];
        snprintf(msg, sizeof msg,
                 "dsm_undistorter_create: remap entry %zu (x = %d, y = %d) = (%.9g, %.9g): its 2x2 footprint leaves the %d x %d source",
                 i, (int)(i % w_out), (int)(i / w_out), x, y, w_in, h_in);
        return invalid(msg);
      }
      remap[i] = make_float2(x, y);
    }
  }
  DSM_HIP(hipSetDevice(ctx->device));
  dsm_undistorter *u = new dsm_undistorter();
  u->ctx = ctx;
  u->tab.w_in = w_in, u->tab.h_in = h_in, u->tab.w_out = w_out, u->tab.h_out = h_out;
  float2 *d_remap = nullptr;
  float *d_G = nullptr, *d_vig = nullptr;
  hipError_t e = hipSuccess;
  if (!pass && e == hipSuccess) e = hipMalloc(&d_remap, n_out * sizeof(float2));
  if (!pass && e == hipSuccess) e = hipMemcpy(d_remap, remap.data(), n_out * sizeof(float2), hipMemcpyHostToDevice);
  if (G && e == hipSuccess) e = hipMalloc(&d_G, 256 * sizeof(float));
  if (G && e == hipSuccess) e = hipMemcpy(d_G, G, 256 * sizeof(float), hipMemcpyHostToDevice);
  if (vignette_inv && e == hipSuccess) e = hipMalloc(&d_vig, n_in * sizeof(float));
  if (vignette_inv && e == hipSuccess) e = hipMemcpy(d_vig, vignette_inv, n_in * sizeof(float), hipMemcpyHostToDevice);
  u->tab.remap = d_remap, u->tab.G = d_G, u->tab.vig = d_vig;
  if (e != hipSuccess) {
    dsm_undistorter_destroy(u);
    DSM_HIP(e);
  }
  *out = u;
  return DSM_OK;
}

int dsm_undistorter_destroy(dsm_undistorter *u) {
  if (!u) return DSM_OK;
  dsm_context *ctx = u->ctx;
  hipSetDevice(ctx->device);
  // hand-overs still in flight read the tables
  hipStreamSynchronize(ctx->stream);
  if (ctx->upload_stream) hipStreamSynchronize(ctx->upload_stream);
  hipFree(const_cast<float2 *>(u->tab.remap));
  hipFree(const_cast<float *>(u->tab.G));
  hipFree(const_cast<float *>(u->tab.vig));
  delete u;
  return DSM_OK;
}

int dsm_upload_images_undistorted(dsm_context *ctx, const dsm_undistorter *u, int n, dsm_tracker *const *trackers, const int *slots,
                                  const void *const *images_u8, const float *ab_exposures, size_t row_pitch_bytes, int form) {
  if (!u) return invalid("dsm_upload_images_undistorted: null undistorter");
  if (u->ctx != ctx) return invalid("dsm_upload_images_undistorted: undistorter of another context");
  switch (form) {
  case DSM_UPLOAD_SYNC:
    return upload_images_impl(ctx, n, trackers, slots, images_u8, ab_exposures, DSM_PIXEL_U8, row_pitch_bytes, false, false, u);
  case DSM_UPLOAD_ASYNC:
    return upload_images_impl(ctx, n, trackers, slots, images_u8, ab_exposures, DSM_PIXEL_U8, row_pitch_bytes, true, false, u);
  case DSM_UPLOAD_ENQUEUE:
    for (int i = 0; trackers && slots && i < n; i++)
      if (slots[i] > 1) return invalid("dsm_upload_images_undistorted: the enqueue form takes front buffers only (slots 0 / 1)");
    return upload_images_impl(ctx, n, trackers, slots, images_u8, ab_exposures, DSM_PIXEL_U8, row_pitch_bytes, false, true, u);
  default:
    return invalid("dsm_upload_images_undistorted: bad form");
  }
}

int dsm_upload_wait(dsm_context *ctx) {
  if (!ctx) return invalid("dsm_upload_wait: null context");
  if (ctx->upload_pending) {
    DSM_HIP(hipSetDevice(ctx->device));
    DSM_HIP(hipEventSynchronize(ctx->upload_copies_event));
    ctx->upload_pending = false;
  }
  if (ctx->enqueue_pending) {
    DSM_HIP(hipSetDevice(ctx->device));
    DSM_HIP(hipEventSynchronize(ctx->copy_event));
    ctx->enqueue_pending = false;
  }
  return DSM_OK;
}

int dsm_frames_advance(dsm_context *ctx, int n, dsm_tracker *const *trackers, const int *slots) {
  if (!ctx || n < 0 || (n > 0 && (!trackers || !slots))) return invalid("dsm_frames_advance: bad argument");
  for (int i = 0; i < n; i++) {
    const dsm_tracker *t = trackers[i];
    if (!t || t->ctx != ctx || slots[i] < 0 || slots[i] > 1) return invalid("dsm_frames_advance: bad entry");
    if (!t->have_back[slots[i]]) return invalid("dsm_frames_advance: nothing was handed over to DSM_SLOT_NEXT_* of this slot");
    for (int j = 0; j < i; j++)
      if (trackers[j] == t && slots[j] == slots[i]) return invalid("dsm_frames_advance: the same slot twice");
  }
  if (n == 0) return DSM_OK;
  DSM_HIP(hipSetDevice(ctx->device));
  // everything enqueued on the context's stream from here on sees the finished pyramids
  if (ctx->upload_stream) DSM_HIP(hipStreamWaitEvent(ctx->stream, ctx->upload_done_event, 0));
  for (int i = 0; i < n; i++) {
    dsm_tracker *t = trackers[i];
    const int s = slots[i];
    for (int l = 0; l < t->nlevels; l++) {
      float *f = t->d_img[s][l];
      t->d_img[s][l] = t->d_img_back[s][l];
      t->d_img_back[s][l] = f;
      t->desc.lv[l].img[s] = t->d_img[s][l];
    }
    float *r = t->d_raw[s];
    t->d_raw[s] = t->d_raw_back[s];
    t->d_raw_back[s] = r;
    const size_t rb = t->raw_bytes[s];
    t->raw_bytes[s] = t->raw_back_bytes[s];
    t->raw_back_bytes[s] = rb;
    t->desc.exposure[s] = t->back_exposure[s];
    t->have_frame[s] = true;
    t->have_back[s] = false;
    t->desc_dirty = true;
  }
  return DSM_OK;
}

int dsm_host_alloc(size_t bytes, void **out) {
  if (!out || bytes == 0) return invalid("dsm_host_alloc: bad argument");
  *out = nullptr;
  DSM_HIP(hipHostMalloc(out, bytes, hipHostMallocDefault));
  return DSM_OK;
}

int dsm_host_free(void *p) {
  if (p) DSM_HIP(hipHostFree(p));
  return DSM_OK;
}

int dsm_tracker_get_frame(dsm_tracker *t, int slot, int lvl, float *dIp_out) {
  if (!t || !dIp_out || slot < 0 || slot > 1 || lvl < 0 || lvl >= t->nlevels) return invalid("dsm_tracker_get_frame: bad argument");
  dsm_context *ctx = t->ctx;
  DSM_HIP(hipSetDevice(ctx->device));
  const int wl = t->w >> lvl, hl = t->h >> lvl;
  const size_t npx = (size_t)wl * hl;
  int rc = ensure_stage(ctx, 3 * npx);
  if (rc) return rc;
  launch_dip_export(ctx->stream, wl, hl, t->d_img[slot][lvl], ctx->d_stage);
  DSM_HIP(hipMemcpyAsync(dIp_out, ctx->d_stage, npx * 12, hipMemcpyDeviceToHost, ctx->stream));
  DSM_HIP(hipStreamSynchronize(ctx->stream));
  return DSM_OK;
}

int dsm_tracker_ref_frame_id(dsm_tracker *t) { return t ? t->ref_frame_id : -1; }

int dsm_reduction_geometry(dsm_tracker *t, int lvl, int n, int *threads, int *pts_per_thread_out, int *chunks) {
  (void)lvl;
  if (!t) return invalid("dsm_reduction_geometry: null tracker");
  if (threads) *threads = kThreads;
  if (pts_per_thread_out) *pts_per_thread_out = pts_per_thread(n, t->desc.p.geometry);
  if (chunks) *chunks = num_chunks(n, t->desc.p.geometry);
  return DSM_OK;
}

// ---- common batch plumbing ------------------------------------------------------------------
} // extern "C"
namespace dsm {
int check_ready(dsm_tracker *t, int mode) {
  if (!t->have_k || !t->have_ref || !t->have_frame[mode == 1 ? 1 : 0]) {
    set_error(mode ? "optimize_scale needs make_k, set_ref and the right frame (slot 1)"
                   : "track needs make_k, set_ref and the new left frame (slot 0)");
    return DSM_ERR_STATE;
  }
  return DSM_OK;
}
} // namespace dsm
extern "C" {

// ts: n trackers of a call in mode `mode`, followed by n2 trackers of the companion segment in mode `mode2`
static int prepare_batch(dsm_context *ctx, int n, dsm_tracker *const *ts, int mode, int n2 = 0, int mode2 = 1) {
  if (!ctx || n <= 0 || n2 < 0 || !ts) return invalid("batch: bad argument");
  DSM_HIP(hipSetDevice(ctx->device));
  int ps = 0;
  for (int i = 0; i < n + n2; i++) {
    dsm_tracker *t = ts[i];
    if (!t || t->ctx != ctx) return invalid("batch: tracker does not belong to this context");
    if (t->w != ts[0]->w || t->h != ts[0]->h || t->nlevels != ts[0]->nlevels)
      return invalid("batch: all trackers must share image size and levels");
    int rc = check_ready(t, i < n ? mode : mode2);
    if (rc) return rc;
    const int need = 2 * max_chunks_upto(t->w * t->h) * kPartialStride; // second half: the speculative candidate's partials
    if (need > ps) ps = need;
  }
  int rc = ensure_batch_capacity(ctx, n + n2, ps);
  if (rc) return rc;
  rc = sync_descs(ctx, ts, n + n2);
  if (rc) return rc;
  for (int i = 0; i < n + n2; i++) ctx->h_tracker_ptrs[i] = ts[i]->d_desc;
  DSM_HIP(hipMemcpyAsync(ctx->d_tracker_ptrs, ctx->h_tracker_ptrs, sizeof(TrackerDev *) * (n + n2), hipMemcpyHostToDevice, ctx->stream));
  return DSM_OK;
}

} // extern "C"

// Work-queue form: one launch of persistent workgroups for the whole call (queue_kernel).  Scheduling only:
// results are bit-identical to the launch-per-step form (run_passes).
// Default rule (measured): the queue form wins while the batch is large enough to fill the
// persistent workgroups and small enough that its per-item cost (a few microseconds per chunk) does not add up --
// up to about 24 k finest-level chunks per call (about 200 dense KITTI frames; thousands of sparse ones).
static bool queue_wanted(const dsm_params &P, int n, int n2, dsm_tracker *const *ts) {
  bool use_queue = P.work_queue >= 2 && n2 == 0;
  if (P.work_queue == 1 && n >= 32 && n2 == 0) {
    long long chunks0 = 0;
    for (int i = 0; i < n; i++) chunks0 += level_chunks(ts[i]->desc, 0);
    use_queue = chunks0 <= 24576; // (256 dense S2 frames = 29.7 k chunks: 4 % slower than the launch form; 192: faster)
  }
  return use_queue;
}
static int run_queue(dsm_context *ctx, dsm_tracker *const *ts, int n, int mode, int coarsest) {
  int max_items = 1;
  for (int L = 0; L <= coarsest; L++)
    for (int i = 0; i < n; i++) {
      const int c = level_chunks(ts[i]->desc, L);
      if (c > max_items) max_items = c;
    }
  if (max_items >= (1 << kQueueChunkBits) || n >= (1 << (32 - kQueueChunkBits))) return invalid("work queue: batch or level too large");
  size_t qcap = 1024; // outstanding items <= problems x chunks of one evaluation: a problem has one evaluation in flight
  while (qcap < (size_t)n * max_items) qcap <<= 1;
  if (qcap > ctx->qcap) {
    ctx->qcap = 0;
    const int rc = realloc_dev(&ctx->d_qitems, qcap);
    if (rc) return rc;
    ctx->qcap = qcap;
  }
  if (!ctx->d_queue) DSM_HIP(hipMalloc(&ctx->d_queue, sizeof(WorkQueue)));
  if (!ctx->h_queue) DSM_HIP(hipHostMalloc(&ctx->h_queue, sizeof(WorkQueue), hipHostMallocDefault));
  DSM_HIP(hipMemsetAsync(ctx->d_queue, 0, sizeof(WorkQueue), ctx->stream));
  DSM_HIP(hipMemsetAsync(ctx->d_qitems, 0, ctx->qcap * sizeof(unsigned long long), ctx->stream)); // stale publication tags
  if (ctx->queue_blocks[mode] == 0) {
    hipDeviceProp_t prop;
    DSM_HIP(hipGetDeviceProperties(&prop, ctx->device));
    const int per_cu = queue_kernel_blocks_per_cu(mode);
    if (per_cu < 1) return invalid("work queue: kernel does not fit the device");
    ctx->queue_blocks[mode] = per_cu * prop.multiProcessorCount; // all workgroups must be co-resident
  }
  hipEvent_t qa = ctx->timing ? get_event(ctx, 0) : nullptr, qb = ctx->timing ? get_event(ctx, 1) : nullptr;
  if (qa) DSM_HIP(hipEventRecord(qa, ctx->stream));
  launch_queue(ctx->stream, mode, ctx->queue_blocks[mode], n, ctx->d_tracker_ptrs, ctx->d_states, ctx->d_partials,
               ctx->partial_stride, ctx->d_tickets, ctx->d_queue, ctx->d_qitems, (unsigned)(ctx->qcap - 1));
  if (qb) DSM_HIP(hipEventRecord(qb, ctx->stream));
  DSM_HIP(hipGetLastError());
  DSM_HIP(hipMemcpyAsync(ctx->h_queue, ctx->d_queue, sizeof(WorkQueue), hipMemcpyDeviceToHost, ctx->stream));
  ctx->stats.queue_blocks = ctx->queue_blocks[mode];
  return DSM_OK;
}
// after the call's read-back: the queue kernel's verdict and statistics
static int queue_outcome(dsm_context *ctx) {
  if (ctx->h_queue->error) {
    // leave the arrival counters clean for the next call
    DSM_HIP(hipMemsetAsync(ctx->d_tickets, 0, sizeof(int) * ctx->cap_prob, ctx->stream));
    DSM_HIP(hipStreamSynchronize(ctx->stream));
    set_error("internal: work-queue kernel gave up waiting (bounded wait expired)");
    return DSM_ERR_STATE;
  }
  ctx->stats.queue_items = ctx->h_queue->tail;
  if (ctx->timing && ctx->ev_pool.size() >= 2) {
    float qm = 0;
    if (hipEventElapsedTime(&qm, ctx->ev_pool[0], ctx->ev_pool[1]) == hipSuccess) ctx->stats.queue_kernel_ms = qm;
  }
  return DSM_OK;
}

// Small levels as a CHAIN (chain_kernel, dsm_params.persistent_coarse < 0): every problem whose evaluation at the coarsest level is one
// chunk runs its LM loop in one launch, down to its first level of several chunks.  One launch per stream group and one for the
// companion segment.  top / top2 (in: the coarsest level, -1 for no companion): the first level of each segment that the
// launch-per-step schedule has to run.
static int run_chain_prefix(dsm_context *ctx, dsm_tracker *const *ts, int n, int n2, const std::vector<Seg> &segs, int coarsest, int &top, int &top2) {
  const int N = n + n2;
  auto one_chunk = [&](int i, int L) { return level_chunks(ts[i]->desc, L) <= 1; };
  bool any = false;
  for (int i = 0; i < N && !any; i++) any = one_chunk(i, coarsest);
  if (!any) return DSM_OK;
  const int rc = fork_segments(ctx, segs, top2 >= 0);
  if (rc) return rc;
  for (const Seg &sg : segs) launch_chain(sg.st, sg.mode, sg.i1 - sg.i0, ctx->d_tracker_ptrs + sg.i0, ctx->d_states + sg.i0, ctx->d_status + 2 * sg.i0);
  ctx->stats.coarse_launches = 1;
  auto first_launch_level = [&](int i0, int i1) { // (the launch-per-step schedule starts at the first level some problem cannot chain through)
    int t = -1;
    for (int i = i0; i < i1; i++)
      for (int L = coarsest; L > t; L--)
        if (!one_chunk(i, L)) {
          t = L;
          break;
        }
    return t;
  };
  top = first_launch_level(0, n);
  if (n2 > 0) top2 = first_launch_level(n, N);
  return DSM_OK;
}

// Launch-per-step form.  The LM loop is sequential per problem and its length is data dependent
// (TrackerAndScaler.cpp:477,505,588,601); polling the device after every few launches costs a
// host round trip each time.  Instead every level gets a speculative number of (eval, lm) launch
// pairs -- the largest count any problem needed in recent calls plus slack -- and the state is
// read back ONCE per pass.  Problems that finish a level early idle through the remaining
// launches (their workgroups exit on the first instruction); problems that need more simply stay
// at their level and are continued by the next pass.  Results do not depend on the schedule.
struct PassRun { // what the passes of one call share
  dsm_context *ctx;
  const dsm_params &P;
  std::vector<Seg> &segs;
  int mode, mode2;
  LMBuffers B;
  EvalTimer tm;
  int worst[DSM_MAX_LEVELS]; // upper bound of evaluations at one level
  RoundShape shape[DSM_MAX_LEVELS];
};

static void plan_levels(PassRun &run, dsm_tracker *const *ts, int N, int nlevels) {
  dsm_context *ctx = run.ctx;
  for (int L = 0; L < nlevels; L++) {
    int max_chunks = 1, max_it = 0, max_n = 0;
    for (int i = 0; i < N; i++) {
      const int c = level_chunks(ts[i]->desc, L);
      if (c > max_chunks) max_chunks = c;
      if (ts[i]->desc.lv[L].n > max_n) max_n = ts[i]->desc.lv[L].n;
      const int it_i = ts[i]->params.fixed_schedule > 0 ? ts[i]->params.fixed_schedule : ts[i]->params.max_iterations[L];
      if (it_i > max_it) max_it = it_i;
    }
    run.worst[L] = 2 * (7 + (max_it > 0 ? max_it : 0));
    // the points of one launch, for the speculative candidate's rule: a stream group's share of the call's problems
    int groups = ctx->n_streams < 1 ? 1 : ctx->n_streams;
    if (groups > N) groups = N;
    run.shape[L] = RoundShape{max_chunks < 8 ? max_chunks : round8(max_chunks), max_n, (long long)((N + groups - 1) / groups) * max_n, 0, false};
  }
}

// one (evaluate, step) round of a segment at level L: the fused step for segments of few problems and for compact launches
static int batch_round(PassRun &run, const Seg &sg, int L, int k) {
  RoundShape R = run.shape[L];
  R.fuse_count = sg.i1 - sg.i0;
  R.fuse_also = sg.rows[L] >= 0;
  return launch_round(run.ctx, run.B, run.P, sg, L, k, run.ctx->d_rowmap + sg.i0, R, run.tm);
}

// row map of a segment: the problems (relative to its first) for which `keep(status, level)` holds, from h_status
template <typename Keep>
static int build_rowmap(dsm_context *ctx, const Seg &sg, Keep keep, int *rows) {
  int r = 0;
  for (int i = sg.i0; i < sg.i1; i++)
    if (keep(ctx->h_status[2 * i], ctx->h_status[2 * i + 1])) ctx->h_rowmap[sg.i0 + r++] = i - sg.i0;
  *rows = r;
  if (r > 0) DSM_HIP(hipMemcpyAsync(ctx->d_rowmap + sg.i0, ctx->h_rowmap + sg.i0, sizeof(int) * r, hipMemcpyHostToDevice, sg.st));
  return DSM_OK;
}

// Level L of a pass; steps / steps2: the rounds of the main segments / the companion.
// Phase A: the rounds most problems need (up to the third quartile of what recent calls' problems took), one row per
// problem.  Phase B, first pass only: ONE read-back of the level's status, then the remaining rounds as compact
// launches over the problems still at this level -- the stragglers (a level's last rounds are needed by a handful of
// problems: 52 launches at levels 2 and 3 of 512 distinct S2 frames where the median problem needs 6 and 10).
static int run_level(PassRun &run, int L, int pass, bool compact_ok, int steps, int steps2) {
  dsm_context *ctx = run.ctx;
  std::vector<Seg> &segs = run.segs;
  auto seg_steps = [&](const Seg &sg) { return sg.companion ? steps2 : steps; };
  auto seg_bulk = [&](const Seg &sg) {
    const int st = seg_steps(sg), bk = ctx->sched_bulk[sg.companion ? run.mode2 : run.mode][L];
    const bool worth = compact_ok && pass == 0 && sg.i1 - sg.i0 >= 32 && (long long)run.shape[L].grid_x * (sg.i1 - sg.i0) >= 1024 && st - bk >= 3;
    return worth ? bk : st;
  };
  int kmax = 0;
  for (const Seg &sg : segs) kmax = seg_bulk(sg) > kmax ? seg_bulk(sg) : kmax;
  for (int k = 0; k < kmax; k++)
    for (int si = (int)segs.size() - 1; si >= 0; si--) { // (the companion's round first, as before)
      const Seg &sg = segs[si];
      if (k < seg_bulk(sg)) {
        const int rc = batch_round(run, sg, L, k);
        if (rc) return rc;
      }
    }
  bool any_tail = false;
  for (const Seg &sg : segs) any_tail = any_tail || seg_bulk(sg) < seg_steps(sg);
  if (!any_tail) return DSM_OK;
  for (const Seg &sg : segs)
    if (seg_bulk(sg) < seg_steps(sg))
      DSM_HIP(hipMemcpyAsync(ctx->h_status + 2 * sg.i0, ctx->d_status + 2 * sg.i0, sizeof(int) * 2 * (sg.i1 - sg.i0), hipMemcpyDeviceToHost, sg.st));
  // the segments in the order their read-backs complete (the others keep their queues busy meanwhile): whichever stream is
  // idle already, else the first one still pending
  std::vector<char> tail_done(segs.size(), 0);
  DSM_HIP(hipGetLastError()); // (launch errors so far; a "not ready" answer below is consumed where it is returned)
  auto idle = [](hipStream_t st) {
    const hipError_t q = hipStreamQuery(st);
    if (q == hipErrorNotReady) (void)hipGetLastError();
    return q == hipSuccess;
  };
  for (size_t done = 0; done < segs.size(); done++) {
    int pick = -1;
    for (size_t si = 0; si < segs.size() && pick < 0; si++)
      if (!tail_done[si] && (seg_bulk(segs[si]) >= seg_steps(segs[si]) || idle(segs[si].st))) pick = (int)si;
    for (size_t si = 0; si < segs.size() && pick < 0; si++)
      if (!tail_done[si]) pick = (int)si;
    tail_done[pick] = 1;
    Seg &sg = segs[pick];
    const int kb = seg_bulk(sg), ks = seg_steps(sg);
    if (kb >= ks) continue;
    DSM_HIP(hipStreamSynchronize(sg.st));
    int rc = build_rowmap(ctx, sg, [L](int st, int lv) { return st == ST_RUNNING && lv == L; }, &sg.rows[L]);
    for (int k = kb; k < ks && !rc; k++) rc = batch_round(run, sg, L, k);
    if (rc) return rc;
  }
  ctx->stats.polls++;
  return DSM_OK;
}

// top / top2: the first level of the main / companion segment (-1: nothing to run)
static int run_passes(PassRun &run, dsm_tracker *const *ts, int n, int n2, int top, int top2) {
  dsm_context *ctx = run.ctx;
  const dsm_params &P = run.P;
  const int N = n + n2;
  plan_levels(run, ts, N, ts[0]->nlevels);
  const int *sched = ctx->sched[run.mode], *sched2 = ctx->sched[run.mode2];
  for (int pass = 0;; pass++) {
    int rc = fork_segments(ctx, run.segs, top2 >= 0);
    if (rc) return rc;
    // Later passes only continue what the previous one left unfinished: compact launches over the problems still running
    // (a launch over all problems of a batch costs ~1.6 ns per idle workgroup: 100 us for a level-0 grid of 512 problems).
    const bool compact_ok = P.adaptive_schedule != 0 && P.compact_tail != 0;
    for (Seg &sg : run.segs) {
      int rows = -1;
      if (pass > 0 && compact_ok && (rc = build_rowmap(ctx, sg, [](int st, int) { return st == ST_RUNNING; }, &rows))) return rc;
      std::fill(sg.rows, sg.rows + DSM_MAX_LEVELS, rows);
    }
    for (int L = top > top2 ? top : top2; L >= 0; L--) {
      auto rounds = [&](const int *sch) {
        const int s = P.adaptive_schedule ? sch[L] << (pass > 3 ? 3 : pass) : run.worst[L];
        return s > run.worst[L] ? run.worst[L] : s < 1 ? 1 : s;
      };
      const int steps = L > top ? 0 : rounds(sched), steps2 = L > top2 ? 0 : rounds(sched2);
      if ((rc = run_level(run, L, pass, compact_ok, steps, steps2))) return rc;
      ctx->stats.launches[L] += steps;
      ctx->stats2.launches[L] += steps2;
    }
    DSM_HIP(hipGetLastError()); // launch-configuration errors of the kernels enqueued above
    if ((rc = join_segments(ctx, run.segs, top2 >= 0))) return rc;
    DSM_HIP(hipMemcpyAsync(ctx->h_status, ctx->d_status, sizeof(int) * 2 * N, hipMemcpyDeviceToHost, ctx->stream));
    DSM_HIP(hipStreamSynchronize(ctx->stream));
    ctx->stats.polls++;
    top = top2 = -1;
    for (int i = 0; i < n; i++)
      if (ctx->h_status[2 * i] == ST_RUNNING && ctx->h_status[2 * i + 1] > top) top = ctx->h_status[2 * i + 1];
    for (int i = n; i < N; i++)
      if (ctx->h_status[2 * i] == ST_RUNNING && ctx->h_status[2 * i + 1] > top2) top2 = ctx->h_status[2 * i + 1];
    if (top < 0 && top2 < 0) break;
    if (pass > 64) {
      set_error("internal: LM state machine did not terminate within the launch bound");
      return DSM_ERR_STATE;
    }
  }
  return DSM_OK;
}

// after the call's read-back: every problem must have terminated; the statistics of the call (ctx->stats, the companion's ctx->stats2)
// and the schedule the next call starts from
static int account_and_learn(dsm_context *ctx, dsm_tracker *const *ts, int n, int n2, int mode, int mode2) {
  const int nlevels = ts[0]->nlevels;
  const int N = n + n2;
  int *sched = ctx->sched[mode], *sched2 = ctx->sched[mode2];
  int need[DSM_MAX_LEVELS] = {0}, need2[DSM_MAX_LEVELS] = {0};
  for (int i = 0; i < N; i++) {
    const LMState &S = ctx->h_states[i];
    if (S.status == ST_RUNNING) {
      set_error("internal: LM state machine did not terminate within the launch bound");
      return DSM_ERR_STATE;
    }
    dsm_stats &st = i < n ? ctx->stats : ctx->stats2;
    int *nd = i < n ? need : need2;
    for (int l = 0; l < nlevels; l++) {
      if ((int)S.rounds[l] > nd[l]) nd[l] = (int)S.rounds[l]; // launches this problem needed at the level
      st.evals[l] += S.evals[l];
      st.evals_residual_only[l] += S.evals_ro[l];
      st.algorithmic_bytes += S.evals[l] * eval_bytes(ts[i], l);
    }
  }
  // the third quartile of the rounds per problem and level: where the next call's launches turn to the fused form
  std::vector<int> r;
  for (int seg = 0; seg < (n2 > 0 ? 2 : 1); seg++) {
    const int i0 = seg ? n : 0, i1 = seg ? N : n;
    int *dst = ctx->sched_bulk[seg ? mode2 : mode];
    for (int l = 0; l < nlevels; l++) {
      r.clear();
      for (int i = i0; i < i1; i++) r.push_back((int)ctx->h_states[i].rounds[l]);
      std::nth_element(r.begin(), r.begin() + (3 * r.size()) / 4, r.end());
      dst[l] = r[(3 * r.size()) / 4] + 1;
    }
  }
  // next call's schedule: what this batch needed plus one, decaying slowly towards it
  for (int l = 0; l < nlevels; l++) {
    const int want = need[l] + 1;
    const int decayed = sched[l] - (sched[l] + 7) / 8;
    sched[l] = want > decayed ? want : decayed;
    if (n2 > 0) {
      const int want2 = need2[l] + 1, decayed2 = sched2[l] - (sched2[l] + 7) / 8;
      sched2[l] = want2 > decayed2 ? want2 : decayed2;
    }
  }
  return DSM_OK;
}

// runs the device LM state machine for a batch (mode 0 = trackNewestCoarse, 1 = optimizeScale, 2 = loop-closure pose).
// n2 > 0: problems [n, n + n2) form a COMPANION segment in mode2 (dsm_track_and_scale_batch: the keyframes' scale
// optimisations next to the frames' tracking).  The two segments are independent problems; the companion's launches go to a
// stream of their own, so its latency-bound chains of small launches run under the main segment's kernels instead of after
// them.  Launch-per-step form only.  Statistics of the companion: ctx->stats2.
static int run_lm_batch(dsm_context *ctx, int n, dsm_tracker *const *ts, int mode, int coarsest, int n2 = 0, int mode2 = 1) {
  const int nlevels = ts[0]->nlevels;
  if (coarsest < 0 || coarsest >= nlevels) return invalid("coarsest level out of range"); // :457 / :856
  const dsm_params &P = ts[0]->params;
  const int N = n + n2;
  memset(&ctx->stats, 0, sizeof ctx->stats);
  memset(&ctx->stats2, 0, sizeof ctx->stats2);
  DSM_HIP(hipEventRecord(ctx->ev_total[0], ctx->stream));
  DSM_HIP(hipMemcpyAsync(ctx->d_start, ctx->h_start, sizeof(StartInfo) * N, hipMemcpyHostToDevice, ctx->stream));
  launch_lm(ctx->stream, mode, LM_OP_START, coarsest, n, ctx->d_tracker_ptrs, ctx->d_states, ctx->d_partials,
            ctx->partial_stride, ctx->d_start, nullptr, ctx->d_status);
  if (n2 > 0)
    launch_lm(ctx->stream, mode2, LM_OP_START, coarsest, n2, ctx->d_tracker_ptrs + n, ctx->d_states + n,
              ctx->d_partials + (size_t)n * ctx->partial_stride, ctx->partial_stride, ctx->d_start + n, nullptr, ctx->d_status + 2 * n);
  const bool use_queue = queue_wanted(P, n, n2, ts);
  int rc;
  if (use_queue && (rc = run_queue(ctx, ts, n, mode, coarsest))) return rc;
  // the learnt "rounds most problems need" belong to calls of this size and form: another batch-size bucket (powers of four)
  // or form must not inherit them (a batch of hundreds following a single-frame call would switch to compact launches after
  // one round, covering almost every problem)
  int bucket = 0;
  for (int v = N; v >= 4; v >>= 2) bucket++;
  const int key = bucket * 4 + (use_queue ? 2 : 0) + (P.persistent_coarse < 0 ? 1 : 0);
  if (key != ctx->sched_bulk_key) {
    for (int m = 0; m < 3; m++)
      for (int l = 0; l < DSM_MAX_LEVELS; l++) ctx->sched_bulk[m][l] = 1 << 30;
    ctx->sched_bulk_key = key;
  }
  std::vector<Seg> segs = build_segments(ctx->n_streams, n, mode, n2, mode2);
  if ((rc = bind_streams(ctx, segs))) return rc;
  PassRun run{ctx, P, segs, mode, mode2,
              LMBuffers{ctx->d_tracker_ptrs, ctx->d_states, ctx->d_partials, ctx->partial_stride, ctx->d_tickets, ctx->d_status}, EvalTimer{}, {}, {}};
  if (!use_queue) {
    int top = coarsest, top2 = n2 > 0 ? coarsest : -1;
    rc = P.persistent_coarse < 0 ? run_chain_prefix(ctx, ts, n, n2, segs, coarsest, top, top2) : DSM_OK;
    if (!rc) rc = run_passes(run, ts, n, n2, top, top2);
    if (rc) return rc;
  }
  DSM_HIP(hipMemcpyAsync(ctx->h_states, ctx->d_states, sizeof(LMState) * N, hipMemcpyDeviceToHost, ctx->stream));
  DSM_HIP(hipEventRecord(ctx->ev_total[1], ctx->stream));
  DSM_HIP(hipStreamSynchronize(ctx->stream));
  if (use_queue && (rc = queue_outcome(ctx))) return rc;
  float ms = 0;
  DSM_HIP(hipEventElapsedTime(&ms, ctx->ev_total[0], ctx->ev_total[1]));
  ctx->stats.total_ms = ms;
  ctx->stats2.total_ms = ms;
  if (ctx->timing) collect_eval_timing(ctx, run.tm.lvl, nlevels, ctx->stats);
  return account_and_learn(ctx, ts, n, n2, mode, mode2);
}

// the start values and the read-out of n track problems / n scale problems, as the batch calls' arguments hold them
static void fill_track_starts(StartInfo *I, int n, const double *pose, const double *aff, const double *min_res, int coarsest) {
  for (int i = 0; i < n; i++) fill_track_start(I[i], pose + 7 * i, aff + 2 * i, min_res ? min_res + DSM_MAX_LEVELS * i : nullptr, coarsest);
}
static void fill_scale_starts(StartInfo *I, int n, const float *scale, int coarsest) {
  for (int i = 0; i < n; i++) fill_scale_start(I[i], scale[i], coarsest);
}
static void read_track_batch(const LMState *S, int n, double *pose_io, double *aff_io, double *last_residuals, double *flow_out, int *good) {
  for (int i = 0; i < n; i++) {
    read_track(S[i], pose_io + 7 * i, aff_io + 2 * i, good ? good + i : nullptr);
    if (last_residuals) memcpy(last_residuals + DSM_MAX_LEVELS * i, S[i].last_residuals, sizeof(double) * DSM_MAX_LEVELS);
    if (flow_out) memcpy(flow_out + 3 * i, S[i].flow, sizeof(double) * 3);
  }
}
static void read_scale_batch(const LMState *S, int n, float *scale_io, float *err_out) {
  for (int i = 0; i < n; i++) read_scale(S[i], scale_io + i, err_out ? err_out + i : nullptr);
}

extern "C" {

int dsm_track_batch(dsm_context *ctx, int n, dsm_tracker *const *ts, double *pose_io, double *aff_io,
                    int coarsest_lvl, const double *min_res_for_abort, double *last_residuals, double *flow_out,
                    int *good) {
  if (!pose_io || !aff_io) return invalid("dsm_track_batch: null pose/aff");
  int rc = prepare_batch(ctx, n, ts, 0);
  if (rc) return rc;
  fill_track_starts(ctx->h_start, n, pose_io, aff_io, min_res_for_abort, coarsest_lvl);
  rc = run_lm_batch(ctx, n, ts, 0, coarsest_lvl);
  if (rc) return rc;
  read_track_batch(ctx->h_states, n, pose_io, aff_io, last_residuals, flow_out, good);
  return DSM_OK;
}

int dsm_tracker_track(dsm_tracker *t, double pose_io[7], double aff_io[2], int coarsest_lvl,
                      const double *min_res_for_abort, double *last_residuals, double flow_out[3], int *good) {
  if (!t) return invalid("null tracker");
  dsm_tracker *ts[1] = {t};
  return dsm_track_batch(t->ctx, 1, ts, pose_io, aff_io, coarsest_lvl, min_res_for_abort, last_residuals, flow_out, good);
}

int dsm_optimize_scale_batch(dsm_context *ctx, int n, dsm_tracker *const *ts, float *scale_io, int coarsest_lvl,
                             float *err_out) {
  if (!scale_io) return invalid("dsm_optimize_scale_batch: null scale");
  int rc = prepare_batch(ctx, n, ts, 1);
  if (rc) return rc;
  fill_scale_starts(ctx->h_start, n, scale_io, coarsest_lvl);
  rc = run_lm_batch(ctx, n, ts, 1, coarsest_lvl);
  if (rc) return rc;
  read_scale_batch(ctx->h_states, n, scale_io, err_out);
  return DSM_OK;
}

// One step of many sequences: the frames' trackNewestCoarse AND the keyframes' optimizeScale in one call.  The scale problems
// are independent of the track problems (they read the keyframe tracker's template and its right frame, FrontEnd.cpp:992-998;
// the track problems read the same kind of template and the left frame), so their launches run on a stream of their own
// under the tracking kernels.  Same results as dsm_track_batch followed by dsm_optimize_scale_batch, bit for bit.
int dsm_track_and_scale_batch(dsm_context *ctx, int n, dsm_tracker *const *ts, double *pose_io, double *aff_io, int coarsest_lvl,
                              const double *min_res_for_abort, double *last_residuals, double *flow_out, int *good, int n_scale,
                              dsm_tracker *const *ts_scale, float *scale_io, float *err_out) {
  if (!pose_io || !aff_io || n < 1) return invalid("dsm_track_and_scale_batch: null pose/aff");
  if (n_scale < 0 || (n_scale && (!ts_scale || !scale_io))) return invalid("dsm_track_and_scale_batch: bad scale arguments");
  std::vector<dsm_tracker *> all(ts, ts + n);
  all.insert(all.end(), ts_scale, ts_scale + n_scale);
  int rc = prepare_batch(ctx, n, all.data(), 0, n_scale, 1);
  if (rc) return rc;
  fill_track_starts(ctx->h_start, n, pose_io, aff_io, min_res_for_abort, coarsest_lvl);
  fill_scale_starts(ctx->h_start + n, n_scale, scale_io, coarsest_lvl);
  rc = run_lm_batch(ctx, n, all.data(), 0, coarsest_lvl, n_scale, 1);
  if (rc) return rc;
  read_track_batch(ctx->h_states, n, pose_io, aff_io, last_residuals, flow_out, good);
  read_scale_batch(ctx->h_states + n, n_scale, scale_io, err_out);
  return DSM_OK;
}

int dsm_context_get_stats2(dsm_context *ctx, dsm_stats *out) {
  if (!ctx || !out) return invalid("dsm_context_get_stats2: null argument");
  *out = ctx->stats2;
  return DSM_OK;
}

// The untrapped branch of FrontEnd::optimizeScale (FrontEnd.cpp:995-1003): optimizeScale from every initial guess, keep the
// smallest positive error (the first one on ties).  The guesses are independent problems on the same template and right
// image: ONE batched call instead of eight sequential ones.
int dsm_tracker_optimize_scale_guesses(dsm_tracker *t, int n_guesses, const float *scale_guesses, int coarsest_lvl, float *scale_out,
                                       float *err_out, float *scales_all, float *errs_all) {
  if (!t || n_guesses < 1 || !scale_guesses || !scale_out || !err_out) return invalid("dsm_tracker_optimize_scale_guesses: bad argument");
  std::vector<dsm_tracker *> ts((size_t)n_guesses, t);
  std::vector<float> sc(scale_guesses, scale_guesses + n_guesses), er((size_t)n_guesses, 0.f);
  const int rc = dsm_optimize_scale_batch(t->ctx, n_guesses, ts.data(), sc.data(), coarsest_lvl, er.data());
  if (rc) return rc;
  float new_scale = 1.0f, scale_error = -1.0f; // :991-992
  for (int i = 0; i < n_guesses; i++) {
    const float cur_error = er[i];
    if (cur_error > 0 && (scale_error < 0 || scale_error > cur_error)) { // :998-1001 (NaN compares false: rejected)
      scale_error = cur_error;
      new_scale = sc[i];
    }
    if (scales_all) scales_all[i] = sc[i];
    if (errs_all) errs_all[i] = er[i];
  }
  *scale_out = new_scale;
  *err_out = scale_error;
  return DSM_OK;
}

int dsm_tracker_optimize_scale(dsm_tracker *t, float *scale_io, int coarsest_lvl, float *err_out) {
  if (!t) return invalid("null tracker");
  dsm_tracker *ts[1] = {t};
  return dsm_optimize_scale_batch(t->ctx, 1, ts, scale_io, coarsest_lvl, err_out);
}

// ---- loop-closure pose estimation (row N2): PoseEstimator::estimate, PoseEstimator.cpp:298-506 ----
} // extern "C"

// what PoseEstimator::estimate hands back from a terminated problem (:466-505); every output but M may be NULL
static void read_pose_result(const LMState &S, int n_pts, double *M, float *pose_error, int *inlier_percent_out, int *ok) {
  { // refToNew_current.matrix(), :466
    const double x = S.cur[0], y = S.cur[1], z = S.cur[2], w = S.cur[3];
    M[0] = 1 - 2 * (y * y + z * z), M[1] = 2 * (x * y - z * w), M[2] = 2 * (x * z + y * w), M[3] = S.cur[4];
    M[4] = 2 * (x * y + z * w), M[5] = 1 - 2 * (x * x + z * z), M[6] = 2 * (y * z - x * w), M[7] = S.cur[5];
    M[8] = 2 * (x * z - y * w), M[9] = 2 * (y * z + x * w), M[10] = 1 - 2 * (x * x + y * y), M[11] = S.cur[6];
    M[12] = M[13] = M[14] = 0, M[15] = 1;
  }
  const float err = (float)S.last_residuals[0]; // :467
  if (pose_error) *pose_error = err;
  const bool aff_good = S.status == ST_GOOD;                                        // :469-482
  const bool low_res = err < 10.0f;                                                 // RES_THRES, PoseEstimator.h:26
  const int inlier_percent = 100 * float((int)S.last_inners[0]) / (float)n_pts;     // :486
  const bool enough_inlier = inlier_percent > 90;                                   // INNER_PERCENT, PoseEstimator.h:27
  if (inlier_percent_out) *inlier_percent_out = inlier_percent;
  if (ok) *ok = (aff_good && low_res && enough_inlier) ? 1 : 0;                     // :505
}

struct dsm_pose_estimator {
  dsm_tracker *t = nullptr;
  std::vector<float> x, y, z;
};

extern "C" {

int dsm_pose_estimator_create(dsm_context *ctx, int w, int h, int nlevels, const dsm_params *params,
                              dsm_pose_estimator **out) {
  if (!out) return invalid("dsm_pose_estimator_create: out is NULL");
  const double I4[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  const float k1[4] = {1, 1, 0, 0};
  dsm_tracker *t = nullptr;
  int rc = dsm_tracker_create(ctx, w, h, nlevels, I4, k1, params, &t);
  if (rc) return rc;
  // the loop-closure point set is the same on every level: give every level the level-0 capacity
  for (int l = 1; l < nlevels; l++) {
    hipFree(t->d_pts[l]);
    t->d_pts[l] = nullptr;
    hipError_t e = hipMalloc(&t->d_pts[l], sizeof(float4) * ((size_t)w * h + kTemplatePad));
    if (e == hipSuccess) e = hipMemsetAsync(t->d_pts[l], 0, sizeof(float4) * ((size_t)w * h + kTemplatePad), ctx->stream);
    if (e != hipSuccess) {
      dsm_tracker_destroy(t);
      DSM_HIP(e);
    }
    t->pts_cap[l] = w * h;
    t->desc.lv[l].pts = t->d_pts[l];
  }
  t->desc_dirty = true;
  {
    const hipError_t e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
      dsm_tracker_destroy(t);
      DSM_HIP(e);
    }
  }
  dsm_pose_estimator *pe = new dsm_pose_estimator();
  pe->t = t;
  *out = pe;
  return DSM_OK;
}

int dsm_pose_estimator_destroy(dsm_pose_estimator *pe) {
  if (!pe) return DSM_OK;
  dsm_tracker_destroy(pe->t);
  delete pe;
  return DSM_OK;
}

// The loading half of PoseEstimator::estimate (:306-319), shared by dsm_pose_estimator_estimate and dsm_diag_pose_estimator_eval:
// makeK(new_cam), the points narrowed to float, the reference with affine (0, 0), the new frame's pyramid
static int pose_estimator_load(dsm_pose_estimator *pe, int n_pts, const double *xyz, const float *const *ref_colors, float ref_ab_exposure,
                               const float *const *new_dIp, float new_ab_exposure, const float new_cam[4]) {
  dsm_tracker *t = pe->t;
  int rc = dsm_tracker_make_k(t, new_cam[0], new_cam[1], new_cam[2], new_cam[3]); // makeK(new_cam), :306
  if (rc) return rc;
  pe->x.resize(n_pts), pe->y.resize(n_pts), pe->z.resize(n_pts);
  for (int i = 0; i < n_pts; i++) { // `float x = pts_[i].first(0)` ..., PoseEstimator.cpp:183-185
    pe->x[i] = (float)xyz[3 * i];
    pe->y[i] = (float)xyz[3 * i + 1];
    pe->z[i] = (float)xyz[3 * i + 2];
  }
  int n[DSM_MAX_LEVELS];
  const float *px[DSM_MAX_LEVELS], *py[DSM_MAX_LEVELS], *pz[DSM_MAX_LEVELS];
  for (int l = 0; l < t->nlevels; l++) {
    n[l] = n_pts; // the same point set on every level, one reference colour per level (:238)
    px[l] = pe->x.data(), py[l] = pe->y.data(), pz[l] = pe->z.data();
  }
  // the float4 template slot holds (x, y, z, refColor[lvl]); ref_aff_g2l_ = (0,0) (:317)
  rc = dsm_tracker_set_ref(t, 0, 0.0, 0.0, ref_ab_exposure, n, px, py, pz, ref_colors);
  if (rc) return rc;
  return dsm_tracker_upload_frame(t, DSM_SLOT_NEW_LEFT, new_dIp, new_ab_exposure);
}

int dsm_pose_estimator_estimate(dsm_pose_estimator *pe, int n_pts, const double *xyz, const float *const *ref_colors,
                                float ref_ab_exposure, const float *const *new_dIp, float new_ab_exposure,
                                const float new_cam[4], int coarsest_lvl, double ref_to_new_io[16], float *pose_error,
                                int *ok) {
  if (!pe || n_pts < 1 || !xyz || !ref_colors || !new_dIp || !new_cam || !ref_to_new_io)
    return invalid("dsm_pose_estimator_estimate: bad argument");
  dsm_tracker *t = pe->t;
  if (n_pts > t->w * t->h) return invalid("dsm_pose_estimator_estimate: more points than pixels");
  int rc = pose_estimator_load(pe, n_pts, xyz, ref_colors, ref_ab_exposure, new_dIp, new_ab_exposure, new_cam);
  if (rc) return rc;
  dsm_context *ctx = t->ctx;
  dsm_tracker *ts[1] = {t};
  rc = prepare_batch(ctx, 1, ts, 2);
  if (rc) return rc;
  double pose0[7];
  const double aff0[2] = {0.0, 0.0};
  se3_from_matrix(ref_to_new_io, pose0); // SE3(R, t) constructor, :321-322
  fill_track_start(ctx->h_start[0], pose0, aff0, nullptr, coarsest_lvl);
  rc = run_lm_batch(ctx, 1, ts, 2, coarsest_lvl);
  if (rc) return rc;
  read_pose_result(ctx->h_states[0], n_pts, ref_to_new_io, pose_error, nullptr, ok);
  return DSM_OK;
}

// ---- the batched form: PoseEstimator::estimate of many matches in one call ----
} // extern "C"

// One geometry, many jobs.  Device memory follows the points, not the pixels: the templates of a job are nlevels lists of
// n_pts + kTemplatePad float4 in one arena, its target one intensity plane per level in another (shared by the jobs that pass the same
// pyramid).  Both arenas, the staging of the inputs and the staging of imported pyramids grow on demand and are kept.
struct dsm_pose_batch {
  dsm_context *ctx = nullptr;
  int w = 0, h = 0, nlevels = 0;
  dsm_params params{};
  size_t plane_off[DSM_MAX_LEVELS] = {}, planes_floats = 0; // an intensity pyramid: plane_bytes() per level, each level 16-byte aligned
  size_t dip_off[DSM_MAX_LEVELS] = {}, dip_floats = 0;      // a staged (I, dx, dy) pyramid, likewise
  unsigned char *d_in = nullptr, *h_in = nullptr;           // descriptors, job tables, check counters, staged points and colours (device / pinned)
  size_t in_bytes = 0;
  float4 *d_tpl = nullptr;
  size_t tpl_entries = 0;
  float *d_img = nullptr;
  size_t img_slots = 0;
  float *d_dip = nullptr; // kPoseImportWave staged pyramids
  std::vector<dsm_tracker> trackers; // what run_lm_batch reads of a problem: geometry, parameters, the host copy of the descriptor
  std::vector<dsm_tracker *> ts;
};

namespace {
constexpr int kPoseImportWave = 8; // pyramids staged at a time: 12 B x sum of pixels each, whatever the batch size
size_t align16(size_t bytes) { return (bytes + 15) & ~(size_t)15; }
struct PosePyramid { // a distinct target pyramid of a call
  bool dip;
  const float *const *lv;
};
} // namespace

extern "C" {

int dsm_pose_batch_create(dsm_context *ctx, int w, int h, int nlevels, const dsm_params *params, dsm_pose_batch **out) {
  if (!out) return invalid("dsm_pose_batch_create: out is NULL");
  *out = nullptr;
  if (!ctx) return invalid("dsm_pose_batch_create: null context");
  if (nlevels < 1 || nlevels > DSM_MAX_LEVELS) return invalid("dsm_pose_batch_create: nlevels out of range");
  if ((w >> (nlevels - 1)) < 8 || (h >> (nlevels - 1)) < 8) return invalid("dsm_pose_batch_create: image too small for nlevels");
  if ((long long)w * h * 16 >= (1ll << 32)) return invalid("dsm_pose_batch_create: image too large");
  dsm_params P;
  const int rc = take_params(params, &P);
  if (rc) return rc;
  dsm_pose_batch *pb = new dsm_pose_batch();
  pb->ctx = ctx, pb->w = w, pb->h = h, pb->nlevels = nlevels, pb->params = P;
  for (int l = 0; l < nlevels; l++) {
    const size_t npx = (size_t)(w >> l) * (h >> l);
    pb->plane_off[l] = pb->planes_floats;
    pb->planes_floats += align16(plane_bytes(w >> l, h >> l)) / sizeof(float);
    pb->dip_off[l] = pb->dip_floats;
    pb->dip_floats += align16(npx * 12) / sizeof(float);
  }
  *out = pb;
  return DSM_OK;
}

int dsm_pose_batch_destroy(dsm_pose_batch *pb) {
  if (!pb) return DSM_OK;
  hipSetDevice(pb->ctx->device);
  hipStreamSynchronize(pb->ctx->stream);
  hipFree(pb->d_in);
  if (pb->h_in) hipHostFree(pb->h_in);
  hipFree(pb->d_tpl);
  hipFree(pb->d_img);
  hipFree(pb->d_dip);
  delete pb;
  return DSM_OK;
}

int dsm_pose_estimate_batch(dsm_pose_batch *pb, int n_jobs, const dsm_pose_job *jobs, int coarsest_lvl) {
  if (!pb || !jobs || n_jobs < 1) return invalid("dsm_pose_estimate_batch: null handle, null jobs or n_jobs < 1");
  dsm_context *ctx = pb->ctx;
  const int nl = pb->nlevels, n = n_jobs;
  if (coarsest_lvl < 0 || coarsest_lvl >= nl) return invalid("dsm_pose_estimate_batch: coarsest level out of range");
  // ---- all-or-nothing validation, and the call's distinct target pyramids ----
  std::vector<PosePyramid> pyr;
  std::vector<int> pyr_of(n);
  char msg[200];
  for (int j = 0; j < n; j++) {
    const dsm_pose_job &J = jobs[j];
    const char *what = nullptr;
    if (!J.xyz || !J.ref_colors || !J.ref_to_new_io || !J.ok) what = "a NULL pointer (xyz, ref_colors, ref_to_new_io, ok)";
    else if (J.n_pts < 1) what = "n_pts < 1";
    else if ((long long)J.n_pts > (long long)pb->w * pb->h) what = "more points than pixels";
    else if ((J.new_dIp != nullptr) == (J.new_I != nullptr)) what = "exactly one of new_dIp and new_I must be given";
    if (!what) {
      const float *const *lv = J.new_dIp ? J.new_dIp : J.new_I;
      for (int l = 0; l < nl && !what; l++)
        if (!J.ref_colors[l] || !lv[l]) what = "a NULL level pointer";
      for (int k = 0; k < 16 && !what; k++)
        if (!std::isfinite(J.ref_to_new_io[k])) what = "a non-finite guess";
      if (!what) {
        int p = -1;
        for (size_t q = 0; q < pyr.size() && p < 0; q++) {
          bool same = pyr[q].dip == (J.new_dIp != nullptr);
          for (int l = 0; l < nl && same; l++) same = pyr[q].lv[l] == lv[l];
          if (same) p = (int)q;
        }
        if (p < 0) {
          p = (int)pyr.size();
          pyr.push_back(PosePyramid{J.new_dIp != nullptr, lv});
        }
        pyr_of[j] = p;
      }
    }
    if (what) {
      snprintf(msg, sizeof msg, "dsm_pose_estimate_batch: job %d: %s", j, what);
      return invalid(msg);
    }
  }
  DSM_HIP(hipSetDevice(ctx->device));
  // ---- layout ----
  const size_t npyr = pyr.size();
  size_t nimp = 0;
  std::vector<int> imp_of(npyr, -1); // imported pyramids first come, first served
  for (size_t q = 0; q < npyr; q++)
    if (pyr[q].dip) imp_of[q] = (int)nimp++;
  const size_t desc_off = 0, pack_off = align16(desc_off + sizeof(TrackerDev) * n), imp_off = align16(pack_off + sizeof(PosePackJob) * n);
  const size_t bad_off = align16(imp_off + sizeof(PoseImportJob) * nimp);
  size_t in_need = align16(bad_off + sizeof(int) * 2 * DSM_MAX_LEVELS * nimp);
  size_t tpl_need = 0;
  std::vector<size_t> xyz_off(n), col_off(n), tpl_off(n);
  std::vector<const void *> dev_xyz(n, nullptr);
  std::vector<const void *> dev_col((size_t)n * DSM_MAX_LEVELS, nullptr);
  int max_n = 0;
  for (int j = 0; j < n; j++) {
    const dsm_pose_job &J = jobs[j];
    const size_t np = (size_t)J.n_pts;
    // page-locked caller arrays are read in place by the pack kernel; anything else goes through the staging buffer
    bool in_place = (dev_xyz[j] = pinned_device_pointer(J.xyz)) != nullptr;
    for (int l = 0; l < nl && in_place; l++) in_place = (dev_col[(size_t)j * DSM_MAX_LEVELS + l] = pinned_device_pointer(J.ref_colors[l])) != nullptr;
    if (!in_place) {
      dev_xyz[j] = nullptr;
      xyz_off[j] = in_need;
      in_need += align16(np * 3 * sizeof(double));
      col_off[j] = in_need;
      in_need += align16(np * sizeof(float)) * nl;
    }
    tpl_off[j] = tpl_need;
    tpl_need += (np + kTemplatePad) * nl;
    if (J.n_pts > max_n) max_n = J.n_pts;
  }
  // ---- arenas (a call ends with the stream idle: nothing reads the old ones) ----
  if (in_need > pb->in_bytes) {
    pb->in_bytes = 0;
    int rc = realloc_dev(&pb->d_in, in_need);
    if (!rc) rc = realloc_pinned(&pb->h_in, in_need);
    if (rc) return rc;
    pb->in_bytes = in_need;
  }
  if (tpl_need > pb->tpl_entries) {
    pb->tpl_entries = 0;
    const int rc = realloc_dev(&pb->d_tpl, tpl_need);
    if (rc) return rc;
    pb->tpl_entries = tpl_need;
  }
  if (npyr > pb->img_slots) {
    pb->img_slots = 0;
    const int rc = realloc_dev(&pb->d_img, npyr * pb->planes_floats);
    if (rc) return rc;
    DSM_HIP(hipMemsetAsync(pb->d_img, 0, npyr * pb->planes_floats * sizeof(float), ctx->stream)); // (the slack behind every plane)
    pb->img_slots = npyr;
  }
  if (nimp && !pb->d_dip) {
    const int rc = realloc_dev(&pb->d_dip, (size_t)kPoseImportWave * pb->dip_floats);
    if (rc) return rc;
  }
  // ---- the problems: descriptor, pack job and staged inputs of every job ----
  if ((int)pb->trackers.size() < n) pb->trackers.resize(n);
  pb->ts.resize(n);
  TrackerDev *h_desc = (TrackerDev *)(pb->h_in + desc_off), *d_desc = (TrackerDev *)(pb->d_in + desc_off);
  PosePackJob *h_pack = (PosePackJob *)(pb->h_in + pack_off);
  const double I4[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  const float k1[4] = {1, 1, 0, 0};
  for (int j = 0; j < n; j++) {
    const dsm_pose_job &J = jobs[j];
    const size_t np = (size_t)J.n_pts;
    TrackerDev D; // as dsm_pose_estimator_create + make_k + set_ref + upload_frame leave the single handle's
    desc_init(D, nl, pb->params);
    se3_from_matrix(I4, D.T10);
    desc_cam1(D, nl, k1);
    desc_make_k(D, nl, J.new_cam[0], J.new_cam[1], J.new_cam[2], J.new_cam[3]); // makeK(new_cam), :306
    PosePackJob &K = h_pack[j];
    memset(&K, 0, sizeof K);
    K.n = J.n_pts;
    const bool in_place = dev_xyz[j] != nullptr;
    K.xyz = in_place ? (const double *)dev_xyz[j] : (const double *)(pb->d_in + xyz_off[j]);
    if (!in_place) memcpy(pb->h_in + xyz_off[j], J.xyz, np * 3 * sizeof(double));
    float *planes = pb->d_img + (size_t)pyr_of[j] * pb->planes_floats;
    for (int l = 0; l < nl; l++) {
      const size_t co = col_off[j] + (size_t)l * align16(np * sizeof(float));
      K.col[l] = in_place ? (const float *)dev_col[(size_t)j * DSM_MAX_LEVELS + l] : (const float *)(pb->d_in + co);
      if (!in_place) memcpy(pb->h_in + co, J.ref_colors[l], np * sizeof(float));
      K.pts[l] = pb->d_tpl + tpl_off[j] + (size_t)l * (np + kTemplatePad);
      D.lv[l].w = pb->w >> l;
      D.lv[l].h = pb->h >> l;
      D.lv[l].pts = K.pts[l];
      D.lv[l].n = J.n_pts; // the same point set on every level, one reference colour per level (:238)
      D.lv[l].img[0] = D.lv[l].img[1] = planes + pb->plane_off[l];
    }
    D.ref_a = 0.0, D.ref_b = 0.0; // ref_aff_g2l_ = (0,0) (:317)
    D.ref_exposure = J.ref_ab_exposure;
    D.exposure[0] = J.new_ab_exposure;
    h_desc[j] = D;
    dsm_tracker &t = pb->trackers[j];
    t.ctx = ctx, t.w = pb->w, t.h = pb->h, t.nlevels = nl, t.params = pb->params;
    t.desc = D;
    t.d_desc = d_desc + j;
    t.have_k = t.have_ref = t.have_frame[0] = true;
    t.desc_dirty = false; // (the descriptor travels with the staged inputs)
    pb->ts[j] = &t;
  }
  PoseImportJob *h_imp = (PoseImportJob *)(pb->h_in + imp_off), *d_imp = (PoseImportJob *)(pb->d_in + imp_off);
  int *h_bad = (int *)(pb->h_in + bad_off), *d_bad = (int *)(pb->d_in + bad_off);
  for (size_t q = 0; q < npyr; q++) {
    if (!pyr[q].dip) continue;
    const int k = imp_of[q];
    PoseImportJob &M = h_imp[k];
    memset(&M, 0, sizeof M);
    for (int l = 0; l < nl; l++) {
      M.in3[l] = pb->d_dip + (size_t)(k % kPoseImportWave) * pb->dip_floats + pb->dip_off[l];
      M.plane[l] = pb->d_img + q * pb->planes_floats + pb->plane_off[l];
    }
    M.bad = d_bad + 2 * DSM_MAX_LEVELS * k;
    for (int l = 0; l < DSM_MAX_LEVELS; l++) h_bad[2 * DSM_MAX_LEVELS * k + 2 * l] = 0, h_bad[2 * DSM_MAX_LEVELS * k + 2 * l + 1] = 0x7FFFFFFF;
  }
  int rc = prepare_batch(ctx, n, pb->ts.data(), 2);
  if (rc) return rc;
  const double aff0[2] = {0.0, 0.0};
  for (int j = 0; j < n; j++) {
    double pose0[7];
    se3_from_matrix(jobs[j].ref_to_new_io, pose0); // SE3(R, t) constructor, :321-322
    fill_track_start(ctx->h_start[j], pose0, aff0, nullptr, coarsest_lvl);
  }
  // ---- one transfer, one pack launch, the targets, one LM run ----
  DSM_HIP(hipMemcpyAsync(pb->d_in, pb->h_in, in_need, hipMemcpyHostToDevice, ctx->stream));
  launch_pose_pack(ctx->stream, (const PosePackJob *)(pb->d_in + pack_off), n, nl, max_n);
  const bool check = pb->params.frame_check != 0;
  std::vector<int> wave; // pyramids (indices into pyr) of the wave being staged
  for (size_t q = 0; q < npyr; q++) {
    for (int l = 0; l < nl; l++) {
      const size_t npx = (size_t)(pb->w >> l) * (pb->h >> l);
      if (pyr[q].dip)
        DSM_HIP(hipMemcpyAsync(pb->d_dip + (size_t)(imp_of[q] % kPoseImportWave) * pb->dip_floats + pb->dip_off[l], pyr[q].lv[l], npx * 12,
                               hipMemcpyHostToDevice, ctx->stream));
      else
        DSM_HIP(hipMemcpyAsync(pb->d_img + q * pb->planes_floats + pb->plane_off[l], pyr[q].lv[l], npx * sizeof(float), hipMemcpyHostToDevice,
                               ctx->stream));
    }
    if (pyr[q].dip) wave.push_back((int)q);
    if (!wave.empty() && ((int)wave.size() == kPoseImportWave || q + 1 == npyr)) { // (import jobs are numbered in the order they are staged)
      launch_pose_import(ctx->stream, d_imp + imp_of[wave[0]], (int)wave.size(), pb->w, pb->h, nl, check, pb->params.frame_grad_tol);
      wave.clear();
    }
  }
  DSM_HIP(hipGetLastError());
  if (check && nimp) DSM_HIP(hipMemcpyAsync(h_bad, d_bad, sizeof(int) * 2 * DSM_MAX_LEVELS * nimp, hipMemcpyDeviceToHost, ctx->stream));
  rc = run_lm_batch(ctx, n, pb->ts.data(), 2, coarsest_lvl); // (ends with the stream idle: the check's counters are home as well)
  if (rc) return rc;
  for (int j = 0; check && j < n; j++) {
    const int k = imp_of[pyr_of[j]];
    for (int l = 0; k >= 0 && l < nl; l++) {
      const int *bad = h_bad + 2 * DSM_MAX_LEVELS * k + 2 * l;
      if (!bad[0]) continue;
      const int wl = pb->w >> l, idx = bad[1];
      char m[360];
      snprintf(m, sizeof m,
               "dsm_pose_estimate_batch: job %d: level %d: %d texel(s) whose gradient channels are not the central differences of channel 0 "
               "(makeImages), the first at index %d (x = %d, y = %d); see dsm_params.frame_check / frame_grad_tol",
               j, l, bad[0], idx, idx % wl, idx / wl);
      return invalid(m);
    }
  }
  for (int j = 0; j < n; j++)
    read_pose_result(ctx->h_states[j], jobs[j].n_pts, jobs[j].ref_to_new_io, jobs[j].pose_error, jobs[j].inlier_percent, jobs[j].ok);
  return DSM_OK;
}

// The middle launch of dsm_diag_single_eval's forms 1-3 (form 0 is single_eval's own launch): problem 0's staged evaluation of `nch` chunks
static int launch_eval_form(dsm_context *ctx, int mode, int lvl, int nch, int form, std::vector<void *> &scratch) {
  if (form == 1) { // the split pair: full evaluations in one kernel, residual-only ones in the other
    launch_eval(ctx->stream, mode, lvl, round8(nch > 0 ? nch : 1), 1, ctx->d_tracker_ptrs, ctx->d_states, ctx->d_partials, ctx->partial_stride,
                nullptr, nullptr, false, /*split_ro=*/true);
  } else if (form == 2) { // the tick engine's items: this evaluation's chunks as the list of a one-slot segment, the count set here
    std::vector<unsigned> h(sizeof(TickSegCtl) / sizeof(unsigned) + (nch > 0 ? nch : 1), 0u);
    TickSegCtl *hseg = (TickSegCtl *)h.data();
    hseg->count[0] = nch;
    for (int c = 0; c < nch; c++) h[sizeof(TickSegCtl) / sizeof(unsigned) + c] = (0u << kTickChunkBits) | (unsigned)c;
    unsigned *d = nullptr;
    DSM_HIP(hipMalloc(&d, h.size() * sizeof(unsigned)));
    scratch.push_back(d);
    DSM_HIP(hipMemcpyAsync(d, h.data(), h.size() * sizeof(unsigned), hipMemcpyHostToDevice, ctx->stream));
    DSM_HIP(hipStreamSynchronize(ctx->stream)); // (h is pageable and goes out of scope)
    TickChainArgs none;
    memset(&none, 0, sizeof none);
    launch_tick_eval(ctx->stream, mode, nch, ctx->d_states, ctx->d_partials, ctx->partial_stride, d + sizeof(TickSegCtl) / sizeof(unsigned),
                     (TickSegCtl *)d, /*buf=*/0, /*cap=*/nch, none, /*with_chains=*/false);
  } else { // the chains' one-chunk form
    launch_diag_chain_eval(ctx->stream, mode, ctx->d_states, ctx->d_partials);
  }
  return DSM_OK;
}

// single fused evaluation.  form / residual_only: dsm_diag_single_eval alone (every other caller: 0, 0)
static int single_eval(dsm_tracker *t, int mode, int lvl, const double *pose, const double *aff, float scale,
                       float cutoff, SingleOut *out, int form = 0, int residual_only = 0) {
  if (!t) return invalid("null tracker");
  if (lvl < 0 || lvl >= t->nlevels) return invalid("level out of range");
  dsm_context *ctx = t->ctx;
  dsm_tracker *ts[1] = {t};
  int rc = prepare_batch(ctx, 1, ts, mode);
  if (rc) return rc;
  const int nch = level_chunks(t->desc, lvl);
  if (form == 2 && nch >= (1 << kTickChunkBits)) return invalid("dsm_diag_single_eval: level too large for an item list");
  if (form == 3 && nch > 1) return invalid("dsm_diag_single_eval: form 3 wants a level of one chunk under the tracker's chunk table");
  StartInfo &I = ctx->h_start[0];
  memset(&I, 0, sizeof I);
  if (pose) memcpy(I.pose, pose, sizeof I.pose);
  if (aff) memcpy(I.aff, aff, sizeof I.aff);
  I.scale = scale;
  I.cutoff = cutoff;
  I.lvl = lvl;
  I.residual_only = residual_only;
  DSM_HIP(hipMemcpyAsync(ctx->d_start, ctx->h_start, sizeof(StartInfo), hipMemcpyHostToDevice, ctx->stream));
  launch_lm(ctx->stream, mode, LM_OP_SINGLE_PREP, lvl, 1, ctx->d_tracker_ptrs, ctx->d_states, ctx->d_partials,
            ctx->partial_stride, ctx->d_start, nullptr, nullptr);
  std::vector<void *> scratch; // device memory of the diagnostic forms, freed once the stream is idle
  if (form == 0)
    launch_eval(ctx->stream, mode, lvl, round8(nch > 0 ? nch : 1), 1, ctx->d_tracker_ptrs,
                ctx->d_states, ctx->d_partials, ctx->partial_stride, nullptr, nullptr);
  else
    rc = launch_eval_form(ctx, mode, lvl, nch, form, scratch);
  if (rc) { // (the prepared state stays RUNNING on a failed launch: harmless, every call prepares its own)
    for (void *p : scratch) (void)hipFree(p);
    return rc;
  }
  launch_lm(ctx->stream, mode, LM_OP_SINGLE_FINISH, lvl, 1, ctx->d_tracker_ptrs, ctx->d_states, ctx->d_partials,
            ctx->partial_stride, nullptr, ctx->d_single, nullptr);
  DSM_HIP(hipGetLastError());
  DSM_HIP(hipMemcpyAsync(ctx->h_single, ctx->d_single, sizeof(SingleOut), hipMemcpyDeviceToHost, ctx->stream));
  const hipError_t sync = hipStreamSynchronize(ctx->stream);
  for (void *p : scratch) (void)hipFree(p);
  DSM_HIP(sync);
  *out = ctx->h_single[0];
  return DSM_OK;
}

int dsm_tracker_calc_res_pose(dsm_tracker *t, int lvl, const double pose[7], const double aff[2], float cutoff_th,
                              double rs[6], double H[64], double b[8], int *n_warped) {
  if (!pose || !aff) return invalid("dsm_tracker_calc_res_pose: null pose/aff");
  SingleOut o;
  int rc = single_eval(t, 0, lvl, pose, aff, 1.0f, cutoff_th, &o);
  if (rc) return rc;
  if (rs) memcpy(rs, o.rs, sizeof o.rs);
  if (H) memcpy(H, o.H, sizeof o.H);
  if (b) memcpy(b, o.b, sizeof o.b);
  if (n_warped) *n_warped = o.n_warped;
  return DSM_OK;
}

int dsm_tracker_calc_res_scale(dsm_tracker *t, int lvl, float scale, float cutoff_th, double rs[6], float *H,
                               float *b, int *n_warped) {
  SingleOut o;
  int rc = single_eval(t, 1, lvl, nullptr, nullptr, scale, cutoff_th, &o);
  if (rc) return rc;
  if (rs) memcpy(rs, o.rs, sizeof o.rs);
  if (H) *H = o.Hs;
  if (b) *b = o.bs;
  if (n_warped) *n_warped = o.n_warped;
  return DSM_OK;
}

int dsm_diag_single_eval(dsm_tracker *t, int mode, int lvl, const double pose[7], const double aff[2], float scale, float cutoff_th,
                         int form, int residual_only, double rs[6], double H[64], double b[8], float *Hs, float *bs, int *n_warped) {
  if (mode < 0 || mode > 1) return invalid("dsm_diag_single_eval: mode is 0 (pose) or 1 (scale)");
  if (form < 0 || form > 3) return invalid("dsm_diag_single_eval: form is 0 .. 3");
  if (mode == 0 && (!pose || !aff)) return invalid("dsm_diag_single_eval: null pose/aff");
  SingleOut o;
  int rc = single_eval(t, mode, lvl, mode == 0 ? pose : nullptr, mode == 0 ? aff : nullptr, mode == 0 ? 1.0f : scale, cutoff_th, &o, form,
                       residual_only ? 1 : 0);
  if (rc) return rc;
  if (rs) memcpy(rs, o.rs, sizeof o.rs);
  if (mode == 0) {
    if (H) memcpy(H, o.H, sizeof o.H);
    if (b) memcpy(b, o.b, sizeof o.b);
  } else {
    if (Hs) *Hs = o.Hs;
    if (bs) *bs = o.bs;
  }
  if (n_warped) *n_warped = o.n_warped;
  return DSM_OK;
}

int dsm_diag_pose_estimator_eval(dsm_pose_estimator *pe, int n_pts, const double *xyz, const float *const *ref_colors,
                                 float ref_ab_exposure, const float *const *new_dIp, float new_ab_exposure, const float new_cam[4],
                                 int lvl, const double pose[7], const double aff[2], float cutoff_th, int form, int residual_only,
                                 double rs[6], double H[64], double b[8], int *n_warped) {
  if (!pe || n_pts < 1 || !xyz || !ref_colors || !new_dIp || !new_cam || !pose || !aff)
    return invalid("dsm_diag_pose_estimator_eval: bad argument");
  dsm_tracker *t = pe->t;
  if (n_pts > t->w * t->h) return invalid("dsm_diag_pose_estimator_eval: more points than pixels");
  if (lvl < 0 || lvl >= t->nlevels) return invalid("dsm_diag_pose_estimator_eval: level out of range");
  if (form != 0 && form != 1 && form != 3)
    return invalid("dsm_diag_pose_estimator_eval: form is 0, 1 or 3 (the tick engine has no loop-closure instantiation)");
  if (form == 3 && num_chunks(n_pts, t->desc.p.geometry) > 1) // (every level holds n_pts points: refused before anything is uploaded)
    return invalid("dsm_diag_pose_estimator_eval: form 3 wants n_pts of at most one chunk under the estimator's chunk table");
  int rc = pose_estimator_load(pe, n_pts, xyz, ref_colors, ref_ab_exposure, new_dIp, new_ab_exposure, new_cam);
  if (rc) return rc;
  SingleOut o;
  rc = single_eval(t, 2, lvl, pose, aff, 1.0f, cutoff_th, &o, form, residual_only ? 1 : 0);
  if (rc) return rc;
  if (rs) memcpy(rs, o.rs, sizeof o.rs);
  if (H) memcpy(H, o.H, sizeof o.H);
  if (b) memcpy(b, o.b, sizeof o.b);
  if (n_warped) *n_warped = o.n_warped;
  return DSM_OK;
}

static_assert(sizeof(dsm_lm_propose_in) == 672 && sizeof(dsm_lm_propose_out) == 264, "mirrored by _lib.py's LmProposeIn / LmProposeOut");
int dsm_diag_lm_propose(dsm_tracker *t, int mode, int lvl, int n, const dsm_lm_propose_in *in, int spec, int helper,
                        dsm_lm_propose_out *out) {
  if (!t || !in || !out) return invalid("dsm_diag_lm_propose: null argument");
  if (n < 1 || n > 65536) return invalid("dsm_diag_lm_propose: n is 1 .. 65536");
  if (mode < 0 || mode > 2) return invalid("dsm_diag_lm_propose: mode is 0 (pose), 1 (scale) or 2 (loop-closure pose)");
  if (lvl < 0 || lvl >= t->nlevels) return invalid("dsm_diag_lm_propose: level out of range");
  if (!t->have_k) return invalid("dsm_diag_lm_propose: dsm_tracker_make_k first");
  dsm_context *ctx = t->ctx;
  DSM_HIP(hipSetDevice(ctx->device));
  int rc = sync_desc(t);
  if (rc) return rc;
  const int expired_before = lm_spin_expired();
  if (expired_before < 0) return hip_fail(hipGetLastError(), "lm_spin_expired", __FILE__, __LINE__);
  dsm_lm_propose_in *d_in = nullptr;
  dsm_lm_propose_out *d_out = nullptr;
  std::vector<dsm_lm_propose_out> h_out((size_t)n); // (the caller's array is written only by a call that succeeds)
  hipError_t e = hipMalloc(&d_in, sizeof(dsm_lm_propose_in) * (size_t)n);
  if (e == hipSuccess) e = hipMalloc(&d_out, sizeof(dsm_lm_propose_out) * (size_t)n);
  if (e == hipSuccess) e = hipMemcpyAsync(d_in, in, sizeof(dsm_lm_propose_in) * (size_t)n, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(d_out, 0, sizeof(dsm_lm_propose_out) * (size_t)n, ctx->stream);
  if (e == hipSuccess) {
    launch_diag_lm_propose(ctx->stream, mode, lvl, t->d_desc, n, d_in, d_out, spec != 0, helper != 0);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(h_out.data(), d_out, sizeof(dsm_lm_propose_out) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream);
  const hipError_t sync = hipStreamSynchronize(ctx->stream); // (also before the buffers are freed after a failed enqueue)
  if (e == hipSuccess) e = sync;
  if (d_in) (void)hipFree(d_in);
  if (d_out) (void)hipFree(d_out);
  DSM_HIP(e);
  const int expired_after = lm_spin_expired();
  if (expired_after != expired_before) {
    set_error("dsm_diag_lm_propose: a bounded wait of the LM step's wave hand-shake expired");
    return DSM_ERR_STATE;
  }
  memcpy(out, h_out.data(), sizeof(dsm_lm_propose_out) * (size_t)n);
  return DSM_OK;
}

} // extern "C"
