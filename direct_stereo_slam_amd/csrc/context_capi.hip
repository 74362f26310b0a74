// context_capi.hip -- what every handle of include/dsm_hotpath.h hangs off: the thread's error text, the ABI version, dsm_params,
// the context with its owners' buffers (dsm_internal.hpp), page-locked host memory.
#include <cstdio>
#include <cstring>

#include "dsm_internal.hpp"

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

const void *pinned_device_pointer(const void *p) {
  hipPointerAttribute_t a{};
  if (hipPointerGetAttributes(&a, p) == hipSuccess && a.type == hipMemoryTypeHost && a.devicePointer) return a.devicePointer;
  (void)hipGetLastError(); // (pageable memory is reported as an error by some runtimes)
  return nullptr;
}

// the caller's parameters, checked, or the defaults
int take_params(const dsm_params *params, dsm_params *out) {
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

} // namespace dsm

using namespace dsm;

// ---- the owners of the context's buffers (dsm_internal.hpp): each gives back exactly what it holds ----
void dsm_context::StreamGroups::release() {
  for (hipEvent_t &ev : join_events) hipEventDestroy(ev);
  join_events.clear();
  for (hipStream_t &st : extra_streams) hipStreamDestroy(st);
  extra_streams.clear();
  if (companion_stream) hipStreamDestroy(companion_stream);
  if (companion_event) hipEventDestroy(companion_event);
  if (fork_event) hipEventDestroy(fork_event);
  companion_stream = nullptr, companion_event = nullptr, fork_event = nullptr;
}

void dsm_context::DescStaging::release() {
  if (desc_event) hipEventDestroy(desc_event);
  desc_event = nullptr;
  release_dev(d_desc_stage);
  release_pinned(h_desc_stage);
  desc_stage_cap = 0, desc_stage_busy = false;
}

void dsm_context::HandOver::release() {
  for (hipEvent_t &ev : upload_events) hipEventDestroy(ev);
  upload_events.clear();
  if (copy_event) hipEventDestroy(copy_event);
  if (copy_stream) hipStreamDestroy(copy_stream);
  if (upload_stream) hipStreamDestroy(upload_stream);
  if (upload_copies_event) hipEventDestroy(upload_copies_event);
  if (upload_done_event) hipEventDestroy(upload_done_event);
  copy_event = nullptr, copy_stream = nullptr, upload_stream = nullptr, upload_copies_event = nullptr, upload_done_event = nullptr;
  upload_pending = enqueue_pending = false;
  release_dev(d_pyr_jobs);
  release_pinned(h_pyr_jobs);
  pyr_jobs_cap = 0;
}

void dsm_context::LmWorkspace::release() {
  release_dev(d_tracker_ptrs), release_pinned(h_tracker_ptrs);
  release_dev(d_states), release_pinned(h_states);
  release_dev(d_partials);
  release_dev(d_start), release_pinned(h_start);
  release_dev(d_single), release_pinned(h_single);
  release_dev(d_status), release_pinned(h_status);
  release_dev(d_queue), release_pinned(h_queue);
  release_dev(d_qitems);
  release_dev(d_rowmap), release_pinned(h_rowmap);
  release_dev(d_tickets);
  cap_prob = 0, partial_stride = 0, qcap = 0;
}

void dsm_context::Timing::release() {
  for (hipEvent_t &ev : ev_pool) hipEventDestroy(ev);
  ev_pool.clear();
  for (hipEvent_t &ev : ev_total) {
    if (ev) hipEventDestroy(ev);
    ev = nullptr;
  }
}

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
  if (ce == hipSuccess) ce = hipEventCreate(&ctx->timers.ev_total[0]);
  if (ce == hipSuccess) ce = hipEventCreate(&ctx->timers.ev_total[1]);
  if (ce == hipSuccess) ce = hipEventCreateWithFlags(&ctx->groups.fork_event, hipEventDisableTiming);
  if (ce == hipSuccess) ce = hipEventCreateWithFlags(&ctx->handover.copy_event, hipEventDisableTiming);
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
  (void)ctx->handover.drain(ctx->stream);
  ctx->lm.release();
  ctx->arena.release();
  ctx->timers.release();
  ctx->groups.release();
  ctx->descs.release();
  ctx->handover.release();
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
  ctx->timers.timing = enable != 0;
  return DSM_OK;
}
int dsm_context_set_streams(dsm_context *ctx, int n_streams) {
  if (!ctx || n_streams < 1 || n_streams > 16) return invalid("dsm_context_set_streams: 1..16");
  ctx->groups.n_streams = n_streams;
  return DSM_OK;
}
int dsm_context_get_stats(dsm_context *ctx, dsm_stats *out) {
  if (!ctx || !out) return invalid("null argument");
  *out = ctx->timers.stats;
  return DSM_OK;
}
void *dsm_context_stream(dsm_context *ctx) { return ctx ? (void *)ctx->stream : nullptr; }
int dsm_context_stream_queues(dsm_context *ctx, int *streams_out, int *sharing_out) {
  if (!ctx) return invalid("dsm_context_stream_queues: null context");
  if (streams_out) *streams_out = 1 + (int)ctx->groups.extra_streams.size() + (ctx->groups.companion_stream ? 1 : 0);
  if (sharing_out) *sharing_out = ctx->groups.streams_sharing_a_queue;
  return DSM_OK;
}

int dsm_context_get_stats2(dsm_context *ctx, dsm_stats *out) {
  if (!ctx || !out) return invalid("dsm_context_get_stats2: null argument");
  *out = ctx->timers.stats2;
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

} // extern "C"
