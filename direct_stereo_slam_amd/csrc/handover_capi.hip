// handover_capi.hip -- the batched and the asynchronous image hand-over (dsm_upload_images*, dsm_upload_wait, dsm_frames_advance)
// and the undistorter (dsm_undistorter_*).  The kernels are frame_kernels.hip's.
#include <cstdio>
#include <vector>

#include "dsm_internal.hpp"

using namespace dsm;

// ---- the hand-over owner's two waits (dsm_internal.hpp) ----
int dsm_context::HandOver::drain(hipStream_t main) {
  if (main) DSM_HIP(hipStreamSynchronize(main));
  if (upload_stream) DSM_HIP(hipStreamSynchronize(upload_stream));
  if (copy_stream) DSM_HIP(hipStreamSynchronize(copy_stream));
  return DSM_OK;
}

int dsm_context::HandOver::wait_copies() {
  if (upload_pending) {
    DSM_HIP(hipEventSynchronize(upload_copies_event));
    upload_pending = false;
  }
  if (enqueue_pending) { // (dsm_upload_images_enqueue: its copy kernel still reads the job table and the caller's buffers)
    DSM_HIP(hipEventSynchronize(copy_event));
    enqueue_pending = false;
  }
  return DSM_OK;
}

extern "C" {

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
      const int rc = t->ctx->handover.drain(t->ctx->stream);
      if (rc) return rc;
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
  if (!ctx->handover.copy_stream) DSM_HIP(hipStreamCreateWithFlags(&ctx->handover.copy_stream, hipStreamNonBlocking));
  if (async && !ctx->handover.upload_stream) {
    DSM_HIP(hipStreamCreateWithFlags(&ctx->handover.upload_stream, hipStreamNonBlocking));
    DSM_HIP(hipEventCreateWithFlags(&ctx->handover.upload_copies_event, hipEventDisableTiming));
    DSM_HIP(hipEventCreateWithFlags(&ctx->handover.upload_done_event, hipEventDisableTiming));
  }
  // the job table and the caller's buffers of the previous asynchronous hand-over are still being read until its
  // copies are through
  const int wrc = ctx->handover.wait_copies();
  if (wrc) return wrc;
  if (n > ctx->handover.pyr_jobs_cap) {
    if (ctx->handover.upload_stream) DSM_HIP(hipStreamSynchronize(ctx->handover.upload_stream)); // pyramid kernels read the old table
    DSM_HIP(hipStreamSynchronize(ctx->stream));
    int rc = realloc_dev(&ctx->handover.d_pyr_jobs, (size_t)n);
    if (rc) return rc;
    rc = realloc_pinned(&ctx->handover.h_pyr_jobs, (size_t)n);
    if (rc) return rc;
    ctx->handover.pyr_jobs_cap = n;
  }
  const size_t npx0 = (size_t)src_w * src_h;
  const size_t pitch = row_pitch_bytes ? row_pitch_bytes : row;
  // pinned caller buffers (dsm_host_alloc, hipHostMalloc, hipHostRegister) are read by the GPU directly
  bool all_pinned = true;
  uintptr_t align = (uintptr_t)row | (uintptr_t)pitch;
  for (int i = 0; i < n; i++) {
    float *raw = nullptr;
    int rc = upload_target(trackers[i], slots[i], &raw, ctx->handover.h_pyr_jobs[i].img, npx0 * px);
    if (rc) return rc;
    ctx->handover.h_pyr_jobs[i].raw = raw;
    ctx->handover.h_pyr_jobs[i].src = nullptr;
    ctx->handover.h_pyr_jobs[i].plain = trackers[i]->plane_fact_words(slots[i]); // armed by the build's first launch (launch_pyr_facts_arm)
    if (all_pinned) {
      hipPointerAttribute_t attr{};
      if (hipPointerGetAttributes(&attr, images[i]) == hipSuccess && attr.type == hipMemoryTypeHost && attr.devicePointer) {
        ctx->handover.h_pyr_jobs[i].src = attr.devicePointer;
        align |= (uintptr_t)attr.devicePointer;
      } else {
        (void)hipGetLastError(); // pageable memory: not an error
        all_pinned = false;
      }
    }
  }
  const hipStream_t work = async ? ctx->handover.upload_stream : ctx->stream; // job table, copy kernel, pyramid kernels
  const bool u8 = pixel_type == DSM_PIXEL_U8;
  // the job table of the previous hand-over may still be read by its pyramid kernels on the other work stream
  if (async) {
    DSM_HIP(hipEventRecord(ctx->handover.copy_event, ctx->stream));
    DSM_HIP(hipStreamWaitEvent(work, ctx->handover.copy_event, 0));
  } else if (ctx->handover.upload_stream) {
    DSM_HIP(hipStreamWaitEvent(work, ctx->handover.upload_done_event, 0));
  }
  if (all_pinned) {
    const int unit = (align & 15) == 0 ? 16 : (align & 3) == 0 ? 4 : 1;
    DSM_HIP(hipMemcpyAsync(ctx->handover.d_pyr_jobs, ctx->handover.h_pyr_jobs, sizeof(dsm::PyrJob) * n, hipMemcpyHostToDevice, work));
    // asynchronous: few workgroups, so that the host reads (microseconds of latency each) do not sit in the memory
    // pipelines of the CUs the tracking kernels run on
    launch_host_rows_copy(work, ctx->handover.d_pyr_jobs, n, (int)row, src_h, pitch, unit, async ? ctx->handover.async_copy_blocks : 1 << 20);
    DSM_HIP(hipGetLastError());
    DSM_HIP(hipEventRecord(async ? ctx->handover.upload_copies_event : ctx->handover.copy_event, work));
    if (und)
      launch_undistort_pyramid_batched(work, und->tab, t0->nlevels, ctx->handover.d_pyr_jobs, n);
    else
      launch_pyramid_batched(work, t0->w, t0->h, t0->nlevels, ctx->handover.d_pyr_jobs, n, u8);
    DSM_HIP(hipGetLastError());
    if (!async && nowait)
      ctx->handover.enqueue_pending = true; // (waited for by the next hand-over or dsm_upload_wait)
    else if (!async)
      DSM_HIP(hipEventSynchronize(ctx->handover.copy_event)); // the caller's buffers are free; the pyramid kernels run on behind
  } else {
    // the staging buffers may still be read by the pyramid kernels of the previous hand-over
    DSM_HIP(hipEventRecord(ctx->handover.copy_event, work));
    DSM_HIP(hipStreamWaitEvent(ctx->handover.copy_stream, ctx->handover.copy_event, 0));
    DSM_HIP(hipMemcpyAsync(ctx->handover.d_pyr_jobs, ctx->handover.h_pyr_jobs, sizeof(dsm::PyrJob) * n, hipMemcpyHostToDevice, ctx->handover.copy_stream));
    // groups: the pyramids of one group are built under the copies of the next
    const int group = 16;
    const int ngroups = (n + group - 1) / group;
    while ((int)ctx->handover.upload_events.size() < ngroups) {
      hipEvent_t ev;
      DSM_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
      ctx->handover.upload_events.push_back(ev);
    }
    for (int g = 0; g < ngroups; g++) {
      const int i0 = g * group, i1 = i0 + group < n ? i0 + group : n;
      for (int i = i0; i < i1; i++) {
        void *dst = const_cast<void *>(ctx->handover.h_pyr_jobs[i].raw);
        if (pitch == row)
          DSM_HIP(hipMemcpyAsync(dst, images[i], npx0 * px, hipMemcpyHostToDevice, ctx->handover.copy_stream));
        else
          DSM_HIP(hipMemcpy2DAsync(dst, row, images[i], pitch, row, (size_t)src_h, hipMemcpyHostToDevice, ctx->handover.copy_stream));
      }
      DSM_HIP(hipEventRecord(ctx->handover.upload_events[g], ctx->handover.copy_stream));
      DSM_HIP(hipStreamWaitEvent(work, ctx->handover.upload_events[g], 0));
      if (und)
        launch_undistort_pyramid_batched(work, und->tab, t0->nlevels, ctx->handover.d_pyr_jobs + i0, i1 - i0);
      else
        launch_pyramid_batched(work, t0->w, t0->h, t0->nlevels, ctx->handover.d_pyr_jobs + i0, i1 - i0, u8);
      DSM_HIP(hipGetLastError());
    }
    if (async)
      DSM_HIP(hipEventRecord(ctx->handover.upload_copies_event, ctx->handover.copy_stream));
    else
      DSM_HIP(hipStreamSynchronize(ctx->handover.copy_stream)); // the caller's buffers are free; the pyramid kernels run on behind
  }
  if (async) {
    DSM_HIP(hipEventRecord(ctx->handover.upload_done_event, work));
    ctx->handover.upload_pending = true;
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
  (void)ctx->handover.drain(ctx->stream); // hand-overs still in flight read the tables
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
  if (ctx->handover.upload_pending || ctx->handover.enqueue_pending) DSM_HIP(hipSetDevice(ctx->device));
  return ctx->handover.wait_copies();
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
  if (ctx->handover.upload_stream) DSM_HIP(hipStreamWaitEvent(ctx->stream, ctx->handover.upload_done_event, 0));
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
    t->swap_frame_facts(s);
    t->desc.exposure[s] = t->back_exposure[s];
    t->have_frame[s] = true;
    t->have_back[s] = false;
    t->desc_dirty = true;
  }
  return DSM_OK;
}

} // extern "C"
