// diag_capi.hip -- single evaluations and the diagnostic calls (dsm_tracker_calc_res_*, dsm_diag_*): one evaluation form or one LM
// proposal at a time on the buffers of the batch form, for the tests' exact checks; and the tick engine's diagnostics
// (dsm_diag_tick_reserve / _stage / _step), on device memory of their own.
#include <cstring>
#include <vector>

#include "dsm_internal.hpp"

using namespace dsm;

// The middle launch of dsm_diag_single_eval's forms 1-3 (form 0 is single_eval's own launch): problem 0's staged evaluation of `nch` chunks
static int launch_eval_form(dsm_context *ctx, int mode, int lvl, int nch, int form, std::vector<void *> &scratch) {
  if (form == 1) { // the split pair: full evaluations in one kernel, residual-only ones in the other
    launch_eval(ctx->stream, mode, lvl, round8(nch > 0 ? nch : 1), 1, ctx->lm.d_tracker_ptrs, ctx->lm.d_states, ctx->lm.d_partials, ctx->lm.partial_stride,
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
    launch_tick_eval(ctx->stream, mode, nch, ctx->lm.d_states, ctx->lm.d_partials, ctx->lm.partial_stride, d + sizeof(TickSegCtl) / sizeof(unsigned),
                     (TickSegCtl *)d, /*buf=*/0, /*cap=*/nch, none, /*with_chains=*/false);
  } else { // the chains' one-chunk form
    launch_diag_chain_eval(ctx->stream, mode, ctx->lm.d_states, ctx->lm.d_partials);
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
  StartInfo &I = ctx->lm.h_start[0];
  memset(&I, 0, sizeof I);
  if (pose) memcpy(I.pose, pose, sizeof I.pose);
  if (aff) memcpy(I.aff, aff, sizeof I.aff);
  I.scale = scale;
  I.cutoff = cutoff;
  I.lvl = lvl;
  I.residual_only = residual_only;
  DSM_HIP(hipMemcpyAsync(ctx->lm.d_start, ctx->lm.h_start, sizeof(StartInfo), hipMemcpyHostToDevice, ctx->stream));
  launch_lm(ctx->stream, mode, LM_OP_SINGLE_PREP, lvl, 1, ctx->lm.d_tracker_ptrs, ctx->lm.d_states, ctx->lm.d_partials,
            ctx->lm.partial_stride, ctx->lm.d_start, nullptr, nullptr);
  std::vector<void *> scratch; // device memory of the diagnostic forms, freed once the stream is idle
  if (form == 0)
    launch_eval(ctx->stream, mode, lvl, round8(nch > 0 ? nch : 1), 1, ctx->lm.d_tracker_ptrs,
                ctx->lm.d_states, ctx->lm.d_partials, ctx->lm.partial_stride, nullptr, nullptr);
  else
    rc = launch_eval_form(ctx, mode, lvl, nch, form, scratch);
  if (rc) { // (the prepared state stays RUNNING on a failed launch: harmless, every call prepares its own)
    for (void *p : scratch) (void)hipFree(p);
    return rc;
  }
  launch_lm(ctx->stream, mode, LM_OP_SINGLE_FINISH, lvl, 1, ctx->lm.d_tracker_ptrs, ctx->lm.d_states, ctx->lm.d_partials,
            ctx->lm.partial_stride, nullptr, ctx->lm.d_single, nullptr);
  DSM_HIP(hipGetLastError());
  DSM_HIP(hipMemcpyAsync(ctx->lm.h_single, ctx->lm.d_single, sizeof(SingleOut), hipMemcpyDeviceToHost, ctx->stream));
  const hipError_t sync = hipStreamSynchronize(ctx->stream);
  for (void *p : scratch) (void)hipFree(p);
  DSM_HIP(sync);
  *out = ctx->lm.h_single[0];
  return DSM_OK;
}

extern "C" {

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

int dsm_diag_eval_facts(dsm_tracker *t, int lvl, const double pose[7], int out[4], float bounds[5]) {
  if (!t || !pose || !out || lvl < 0 || lvl >= t->nlevels) return invalid("dsm_diag_eval_facts: bad argument");
  dsm_context *ctx = t->ctx;
  DSM_HIP(hipSetDevice(ctx->device));
  int rc = sync_desc(t);
  if (rc) return rc;
  void *d = nullptr;
  int h[9];
  DSM_HIP(hipMalloc(&d, 64 + sizeof h));
  hipError_t e = hipMemcpyAsync(d, pose, 7 * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) {
    launch_diag_eval_facts(ctx->stream, t->d_desc, lvl, (const double *)d, (int *)((char *)d + 64));
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(h, (char *)d + 64, sizeof h, hipMemcpyDeviceToHost, ctx->stream);
  const hipError_t sync = hipStreamSynchronize(ctx->stream);
  (void)hipFree(d);
  DSM_HIP(e);
  DSM_HIP(sync);
  memcpy(out, h, 4 * sizeof(int));
  if (bounds) memcpy(bounds, h + 4, 5 * sizeof(float));
  return DSM_OK;
}

int dsm_diag_tracker_force_general(dsm_tracker *t, int on) {
  if (!t || !t->facts.d) return invalid("dsm_diag_tracker_force_general: bad argument");
  DSM_HIP(hipSetDevice(t->ctx->device));
  const int v = on ? 1 : 0;
  DSM_HIP(hipMemcpyAsync(&t->facts.d->force_general, &v, sizeof v, hipMemcpyHostToDevice, t->ctx->stream));
  DSM_HIP(hipStreamSynchronize(t->ctx->stream)); // (v is a local)
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

static_assert(sizeof(dsm_lm_step_eval) == 112 && sizeof(dsm_lm_step_state) == 1464, "mirrored by _lib.py's LmStepEval / LmStepState");
static_assert(DSM_LM_IDLE == ST_IDLE && DSM_LM_RUNNING == ST_RUNNING && DSM_LM_GOOD == ST_GOOD && DSM_LM_ABORTED == ST_ABORTED &&
                  DSM_LM_BAD_AFFINE == ST_BAD_AFFINE,
              "dsm_lm_step_state.status is LMState::status");
int dsm_diag_lm_step(dsm_tracker *t, int mode, int lvl, int n, const dsm_lm_step_state *in, const float *partials,
                     long long partial_stride, int spec, int spec_off, int helper, int coherent, dsm_lm_step_state *out) {
  if (!t || !in || !out || !partials) return invalid("dsm_diag_lm_step: null argument");
  if (n < 1 || n > 65536) return invalid("dsm_diag_lm_step: n is 1 .. 65536");
  if (mode < 0 || mode > 2) return invalid("dsm_diag_lm_step: mode is 0 (pose), 1 (scale) or 2 (loop-closure pose)");
  if (lvl < 0 || lvl >= t->nlevels) return invalid("dsm_diag_lm_step: level out of range");
  if (!t->have_k) return invalid("dsm_diag_lm_step: dsm_tracker_make_k first");
  if (partial_stride < 4 || partial_stride % 4 || partial_stride > (1ll << 24)) return invalid("dsm_diag_lm_step: partial_stride is a multiple of 4, 4 .. 2^24");
  if (spec && (spec_off < 0 || spec_off % 4 || spec_off > partial_stride)) return invalid("dsm_diag_lm_step: spec_off is a multiple of 4 inside the problem's block");
  for (int i = 0; i < n; i++) { // every 16-byte read of the reduction stays inside the problem's block
    const long long floats = (long long)in[i].nch * kPartialStride;
    if (in[i].nch < 0 || in[i].nch > 4096) return invalid("dsm_diag_lm_step: nch is 0 .. 4096");
    if (in[i].phase != PH_INIT && in[i].phase != PH_ITER) return invalid("dsm_diag_lm_step: phase is 0 or 1");
    if (floats > (spec ? (long long)spec_off : partial_stride) || (spec && spec_off + floats > partial_stride))
      return invalid("dsm_diag_lm_step: the partials of nch chunks do not fit partial_stride / spec_off");
  }
  dsm_context *ctx = t->ctx;
  DSM_HIP(hipSetDevice(ctx->device));
  int rc = sync_desc(t);
  if (rc) return rc;
  const int expired_before = lm_spin_expired();
  if (expired_before < 0) return hip_fail(hipGetLastError(), "lm_spin_expired", __FILE__, __LINE__);
  dsm_lm_step_state *d_in = nullptr, *d_out = nullptr;
  LMState *d_states = nullptr;
  float *d_partials = nullptr;
  const size_t io_bytes = sizeof(dsm_lm_step_state) * (size_t)n, part_bytes = sizeof(float) * (size_t)partial_stride * (size_t)n;
  std::vector<dsm_lm_step_state> h_out((size_t)n); // (the caller's array is written only by a call that succeeds)
  hipError_t e = hipMalloc(&d_in, io_bytes);
  if (e == hipSuccess) e = hipMalloc(&d_out, io_bytes);
  if (e == hipSuccess) e = hipMalloc(&d_states, sizeof(LMState) * (size_t)n);
  if (e == hipSuccess) e = hipMalloc(&d_partials, part_bytes);
  if (e == hipSuccess) e = hipMemcpyAsync(d_in, in, io_bytes, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_partials, partials, part_bytes, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(d_out, 0, io_bytes, ctx->stream);
  if (e == hipSuccess) {
    launch_diag_lm_step(ctx->stream, mode, lvl, t->d_desc, n, d_in, d_out, d_states, d_partials, partial_stride, spec != 0, spec ? spec_off : 0,
                        helper != 0, coherent != 0);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(h_out.data(), d_out, io_bytes, hipMemcpyDeviceToHost, ctx->stream);
  const hipError_t sync = hipStreamSynchronize(ctx->stream); // (also before the buffers are freed after a failed enqueue)
  if (e == hipSuccess) e = sync;
  if (d_in) (void)hipFree(d_in);
  if (d_out) (void)hipFree(d_out);
  if (d_states) (void)hipFree(d_states);
  if (d_partials) (void)hipFree(d_partials);
  DSM_HIP(e);
  const int expired_after = lm_spin_expired();
  if (expired_after != expired_before) {
    set_error("dsm_diag_lm_step: a bounded wait of the LM step's wave hand-shake expired");
    return DSM_ERR_STATE;
  }
  memcpy(out, h_out.data(), io_bytes);
  return DSM_OK;
}

} // extern "C"

// ---- the tick engine's diagnostics: dsm_diag_tick_reserve / _stage / _step ----
static_assert(sizeof(dsm_tick_seg) == sizeof(TickSegDesc) && sizeof(dsm_tick_seg_ctl) == sizeof(TickSegCtl) && sizeof(TickSegCtl) == 128 &&
                  sizeof(dsm_tick_mode_ctl) == sizeof(TickModeCtl) && sizeof(TickModeCtl) == 176 && sizeof(dsm_tick_result) == sizeof(TickResult) &&
                  sizeof(TickResult) == 312 && sizeof(dsm_tick_pending) == 136 && sizeof(dsm_tick_slot) == 352 && sizeof(dsm_tick_slot_out) == 48 &&
                  sizeof(dsm_tick_list_cfg) == 24,
              "mirrored by _lib.py's Tick* structures");
static_assert(DSM_TICK_NOOP == kTickNoop && DSM_TICK_CAND == kTickCand && DSM_TICK_CHUNK_BITS == kTickChunkBits && DSM_TICK_MAX_SEGS == kTickMaxSegs,
              "the item encoding of include/dsm_hotpath.h is form_tick.hpp's");
static_assert((DSM_TICK_SENTINEL & (kTickNoop | kTickCand)) == 0 && (DSM_TICK_SENTINEL >> kTickChunkBits) > 65536,
              "the sentinel is neither a no-op nor an item of a slot a call can have");

namespace {
constexpr int kDiagMaxSlots = 65536;
constexpr long long kDiagMaxItems = 1ll << 28;
int tick_npos(int nch) { return nch < 8 ? nch : 8 * ((nch + 7) / 8); }

// the device side of dsm_diag_tick_stage / _step: everything tick_after_step, tick_admit_kernel and tick_lm_kernel may write, owned here
struct TickRig {
  hipStream_t stream = nullptr;
  std::vector<void *> owned;
  unsigned *d_items = nullptr;
  TickSegCtl *d_seg = nullptr;
  TickModeCtl *d_mc = nullptr;
  TickPending *d_pending = nullptr;
  TickResult *d_results = nullptr;
  unsigned long long *d_slot_ticket = nullptr;
  const TrackerDev **d_trackers = nullptr, **d_start_trackers = nullptr;
  TrackerDev *d_desc_copy = nullptr;
  LMState *d_states = nullptr, *d_start_states = nullptr;
  StartInfo *d_start = nullptr;
  dsm_tick_slot *d_slots = nullptr;
  dsm_lm_step_state *d_state_out = nullptr;
  dsm_tick_slot_out *d_slot_out = nullptr;
  long long items_len = 0;
  TickList list{};
  template <class T>
  hipError_t alloc(T **p, size_t n) {
    const hipError_t e = hipMalloc((void **)p, (n ? n : 1) * sizeof(T));
    if (e == hipSuccess) owned.push_back((void *)*p);
    return e;
  }
  ~TickRig() {
    if (stream) (void)hipStreamSynchronize(stream); // (also after a failed enqueue: nothing may still use what is freed)
    for (void *p : owned) (void)hipFree(p);
  }
};

// what both calls refuse in the list, the control block and the waiting entries (NULL: nothing); *needed: words behind the item list,
// slot_words: the sum over the slots of what a slot itself could write
const char *tick_rig_error(const dsm_tracker *t, int mode, int n, const dsm_tick_list_cfg *list, const dsm_tick_mode_ctl *ctl, int n_pending,
                           const dsm_tick_pending *pending, long long slot_words, long long *needed) {
  if (mode < 0 || mode > 1) return "mode is 0 (pose) or 1 (scale)";
  if (n < 1 || n > kDiagMaxSlots) return "n is 1 .. 65536 (the item encoding holds the slot number)";
  if (!t->have_k) return "dsm_tracker_make_k first";
  if (list->cap < 0 || list->chain_cap < 0 || list->count < 0 || list->chain < 0) return "negative cap, chain_cap, count or chain";
  if (list->count > list->cap || list->chain > list->chain_cap) return "count > cap or chain > chain_cap at the start";
  if (list->buf < 0 || list->buf > 1) return "buf is 0 or 1";
  if (ctl->ring < 1 || ctl->ring > (1 << 20) || (ctl->ring & (ctl->ring - 1))) return "ring is a power of two, 1 .. 2^20";
  if (ctl->pending_head < 0 || ctl->pending_count < 0 || ctl->retired < 0) return "negative pending_head, pending_count or retired";
  if (n_pending < 0 || n_pending > ctl->ring || (n_pending > 0 && !pending)) return "n_pending is 0 .. ring, with its entries";
  if (ctl->pending_count > ctl->pending_head + n_pending) return "pending_count > pending_head + n_pending: the device would take an entry nobody supplied";
  int start_npos = 0; // the first items of an admitted problem: its coarsest level's
  for (int l = 0; l < t->nlevels; l++) {
    const int np = tick_npos(level_chunks(t->desc, l));
    if (np >= (1 << kTickChunkBits)) return "a level of the tracker has too many chunks for the item encoding";
    if (np > start_npos) start_npos = np;
  }
  for (int k = 0; k < n_pending; k++)
    if (pending[k].coarsest < 0 || pending[k].coarsest >= t->nlevels) return "a waiting entry's coarsest level is out of range";
  const long long total = (long long)list->cap + list->chain_cap + slot_words + (long long)n * start_npos;
  if (total > kDiagMaxItems) return "the item list and its guard region exceed 2^28 words";
  *needed = total;
  return nullptr;
}

// allocates and fills everything but the slot states (d_states: allocated, not filled).  trackers[]: null (stage) or a COPY of the
// descriptor (step: the LM step reads it), so that a pointer an admission wrote is told from what was there
int tick_rig_setup(TickRig &R, dsm_tracker *t, int n, const dsm_tick_slot *slots, const dsm_tick_list_cfg *list, const dsm_tick_mode_ctl *ctl,
                   int n_pending, const dsm_tick_pending *pending, long long items_len, bool desc_copy) {
  dsm_context *ctx = t->ctx;
  R.stream = ctx->stream;
  R.items_len = items_len;
  const int ring = ctl->ring;
  DSM_HIP(R.alloc(&R.d_items, (size_t)items_len));
  DSM_HIP(R.alloc(&R.d_seg, 1));
  DSM_HIP(R.alloc(&R.d_mc, 1));
  DSM_HIP(R.alloc(&R.d_pending, (size_t)ring));
  DSM_HIP(R.alloc(&R.d_results, (size_t)ring));
  DSM_HIP(R.alloc(&R.d_slot_ticket, (size_t)n));
  DSM_HIP(R.alloc(&R.d_trackers, (size_t)n));
  DSM_HIP(R.alloc(&R.d_start_trackers, (size_t)n_pending));
  DSM_HIP(R.alloc(&R.d_desc_copy, 1));
  DSM_HIP(R.alloc(&R.d_states, (size_t)n));
  DSM_HIP(R.alloc(&R.d_start_states, (size_t)n_pending));
  DSM_HIP(R.alloc(&R.d_start, (size_t)n_pending));
  DSM_HIP(R.alloc(&R.d_slots, (size_t)n));
  DSM_HIP(R.alloc(&R.d_state_out, (size_t)n));
  DSM_HIP(R.alloc(&R.d_slot_out, (size_t)n));
  // (pageable sources: every copy below is complete when it returns)
  std::vector<unsigned> items((size_t)items_len, DSM_TICK_SENTINEL);
  DSM_HIP(hipMemcpy(R.d_items, items.data(), items.size() * sizeof(unsigned), hipMemcpyHostToDevice));
  TickSegCtl seg;
  memset(&seg, 0, sizeof seg);
  seg.count[list->buf] = list->count, seg.chain[list->buf] = list->chain;
  seg.count[list->buf ^ 1] = 7, seg.chain[list->buf ^ 1] = 7; // (what tick_lm_kernel's slot 0 clears)
  DSM_HIP(hipMemcpy(R.d_seg, &seg, sizeof seg, hipMemcpyHostToDevice));
  TickModeCtl mc;
  memset(&mc, 0, sizeof mc);
  mc.pending_head = ctl->pending_head, mc.pending_count = ctl->pending_count, mc.retired = ctl->retired, mc.ring = ring;
  for (int l = 0; l < DSM_MAX_LEVELS; l++) mc.sched_evals[l] = ctl->sched_evals[l], mc.sched_ro[l] = ctl->sched_ro[l], mc.sched_items[l] = ctl->sched_items[l];
  DSM_HIP(hipMemcpy(R.d_mc, &mc, sizeof mc, hipMemcpyHostToDevice));
  // the ring: entry k of the caller at (head + k) mod ring; every other entry this tracker too, zero start, a ticket nobody handed in
  std::vector<TickPending> pend((size_t)ring);
  std::vector<StartInfo> starts((size_t)n_pending);
  memset(pend.data(), 0, pend.size() * sizeof(TickPending));
  for (auto &P : pend) P.trk = t->d_desc, P.ticket = ~0ull;
  for (int k = 0; k < n_pending; k++) {
    StartInfo &I = starts[(size_t)k];
    memset(&I, 0, sizeof I);
    memcpy(I.pose, pending[k].pose, sizeof I.pose);
    memcpy(I.aff, pending[k].aff, sizeof I.aff);
    memcpy(I.min_res, pending[k].min_res, sizeof I.min_res);
    I.scale = pending[k].scale, I.coarsest = pending[k].coarsest;
    TickPending &P = pend[(size_t)((ctl->pending_head + k) & (ring - 1))];
    P.start = I, P.ticket = pending[k].ticket;
  }
  DSM_HIP(hipMemcpy(R.d_pending, pend.data(), pend.size() * sizeof(TickPending), hipMemcpyHostToDevice));
  if (n_pending) DSM_HIP(hipMemcpy(R.d_start, starts.data(), starts.size() * sizeof(StartInfo), hipMemcpyHostToDevice));
  DSM_HIP(hipMemset(R.d_results, 0xA5, (size_t)ring * sizeof(TickResult)));
  DSM_HIP(hipMemset(R.d_start_states, 0, (size_t)(n_pending ? n_pending : 1) * sizeof(LMState)));
  DSM_HIP(hipMemset(R.d_state_out, 0, (size_t)n * sizeof(dsm_lm_step_state)));
  DSM_HIP(hipMemset(R.d_slot_out, 0, (size_t)n * sizeof(dsm_tick_slot_out)));
  DSM_HIP(hipMemcpy(R.d_desc_copy, &t->desc, sizeof(TrackerDev), hipMemcpyHostToDevice));
  std::vector<unsigned long long> tickets((size_t)n);
  std::vector<const TrackerDev *> trks((size_t)n, desc_copy ? R.d_desc_copy : nullptr), start_trks((size_t)(n_pending ? n_pending : 1), t->d_desc);
  for (int i = 0; i < n; i++) tickets[(size_t)i] = slots[i].ticket;
  DSM_HIP(hipMemcpy(R.d_slot_ticket, tickets.data(), tickets.size() * sizeof(unsigned long long), hipMemcpyHostToDevice));
  DSM_HIP(hipMemcpy(R.d_trackers, trks.data(), trks.size() * sizeof(void *), hipMemcpyHostToDevice));
  DSM_HIP(hipMemcpy(R.d_start_trackers, start_trks.data(), start_trks.size() * sizeof(void *), hipMemcpyHostToDevice));
  DSM_HIP(hipMemcpy(R.d_slots, slots, (size_t)n * sizeof(dsm_tick_slot), hipMemcpyHostToDevice));
  R.list = TickList{R.d_items, R.d_seg, list->buf, list->cap, list->chain_cap, list->chain_max_n0};
  return DSM_OK;
}

struct TickOutputs {
  unsigned *items;
  dsm_tick_seg_ctl *seg_out;
  dsm_tick_mode_ctl *ctl_out;
  dsm_tick_result *results;
  dsm_tick_slot_out *slot_out;
  dsm_lm_step_state *state_out;
  unsigned char *state_raw, *start_raw;
};
// behind the production launches: what LM_OP_START leaves for every waiting entry, the states unpacked, everything read back; the
// caller's arrays are written only when all of it succeeded
int tick_rig_collect(TickRig &R, dsm_tracker *t, int mode, int n, int ring, int n_pending, const TickOutputs &O) {
  if (n_pending)
    launch_lm(R.stream, mode, LM_OP_START, 0, n_pending, R.d_start_trackers, R.d_start_states, nullptr, 0, R.d_start, nullptr, nullptr);
  launch_diag_tick_unpack(R.stream, n, R.d_states, R.d_trackers, t->d_desc, R.d_slot_ticket, R.d_state_out, R.d_slot_out);
  DSM_HIP(hipGetLastError());
  DSM_HIP(hipStreamSynchronize(R.stream));
  std::vector<unsigned> items((size_t)R.items_len);
  std::vector<dsm_tick_result> results((size_t)ring);
  std::vector<dsm_tick_slot_out> slot_out((size_t)n);
  std::vector<dsm_lm_step_state> state_out((size_t)n);
  std::vector<unsigned char> raw((size_t)n * sizeof(LMState)), start_raw((size_t)n_pending * sizeof(LMState));
  dsm_tick_seg_ctl seg;
  dsm_tick_mode_ctl mc;
  DSM_HIP(hipMemcpy(items.data(), R.d_items, items.size() * sizeof(unsigned), hipMemcpyDeviceToHost));
  DSM_HIP(hipMemcpy(&seg, R.d_seg, sizeof seg, hipMemcpyDeviceToHost));
  DSM_HIP(hipMemcpy(&mc, R.d_mc, sizeof mc, hipMemcpyDeviceToHost));
  DSM_HIP(hipMemcpy(results.data(), R.d_results, results.size() * sizeof(dsm_tick_result), hipMemcpyDeviceToHost));
  DSM_HIP(hipMemcpy(slot_out.data(), R.d_slot_out, slot_out.size() * sizeof(dsm_tick_slot_out), hipMemcpyDeviceToHost));
  DSM_HIP(hipMemcpy(state_out.data(), R.d_state_out, state_out.size() * sizeof(dsm_lm_step_state), hipMemcpyDeviceToHost));
  DSM_HIP(hipMemcpy(raw.data(), R.d_states, raw.size(), hipMemcpyDeviceToHost));
  if (n_pending) DSM_HIP(hipMemcpy(start_raw.data(), R.d_start_states, start_raw.size(), hipMemcpyDeviceToHost));
  memcpy(O.items, items.data(), items.size() * sizeof(unsigned));
  *O.seg_out = seg, *O.ctl_out = mc;
  memcpy(O.results, results.data(), results.size() * sizeof(dsm_tick_result));
  memcpy(O.slot_out, slot_out.data(), slot_out.size() * sizeof(dsm_tick_slot_out));
  memcpy(O.state_out, state_out.data(), state_out.size() * sizeof(dsm_lm_step_state));
  memcpy(O.state_raw, raw.data(), raw.size());
  if (n_pending) memcpy(O.start_raw, start_raw.data(), start_raw.size());
  return DSM_OK;
}
int tick_invalid(const char *entry, const char *what) {
  set_error(std::string(entry) + ": " + what);
  return DSM_ERR_INVALID;
}
} // namespace

extern "C" {

int dsm_diag_tick_reserve(dsm_context *ctx, int nseg, const dsm_tick_seg *segs, int nslots, const unsigned char *running,
                          const long long head[2], const long long count[2], long long *admit_idx, long long head_out[2], int *ctl_intact) {
  const char *me = "dsm_diag_tick_reserve";
  if (!ctx || !running || !head || !count || !admit_idx || !head_out || !ctl_intact || (nseg > 0 && !segs)) return tick_invalid(me, "null argument");
  if (nseg < 0 || nseg > kTickMaxSegs) return tick_invalid(me, "nseg is 0 .. DSM_TICK_MAX_SEGS");
  if (nslots < 1 || nslots > kDiagMaxSlots) return tick_invalid(me, "nslots is 1 .. 65536");
  TickReserveArgs ra;
  memset(&ra, 0, sizeof ra);
  ra.nseg = nseg;
  for (int si = 0; si < nseg; si++) {
    if (segs[si].mode < 0 || segs[si].mode > 1) return tick_invalid(me, "a segment's mode is 0 or 1");
    if (segs[si].i0 < 0 || segs[si].ns < 0 || (long long)segs[si].i0 + segs[si].ns > nslots) return tick_invalid(me, "a segment's slots lie in [0, nslots)");
    ra.seg[si] = TickSegDesc{segs[si].mode, segs[si].i0, segs[si].ns};
  }
  DSM_HIP(hipSetDevice(ctx->device));
  struct Rig { // (freed once the stream is idle)
    hipStream_t s;
    LMState *d_states = nullptr;
    TickModeCtl *d_mc = nullptr;
    long long *d_idx = nullptr;
    ~Rig() {
      (void)hipStreamSynchronize(s);
      if (d_states) (void)hipFree(d_states);
      if (d_mc) (void)hipFree(d_mc);
      if (d_idx) (void)hipFree(d_idx);
    }
  } R{ctx->stream};
  DSM_HIP(hipMalloc(&R.d_states, sizeof(LMState) * (size_t)nslots));
  DSM_HIP(hipMalloc(&R.d_mc, 2 * sizeof(TickModeCtl)));
  DSM_HIP(hipMalloc(&R.d_idx, sizeof(long long) * (size_t)nslots));
  std::vector<LMState> hs((size_t)nslots);
  memset(hs.data(), 0, hs.size() * sizeof(LMState));
  for (int i = 0; i < nslots; i++) hs[(size_t)i].status = running[i] ? ST_RUNNING : ST_IDLE;
  TickModeCtl mc[2];
  memset(mc, 0x5A, sizeof mc);
  for (int m = 0; m < 2; m++) mc[m].pending_head = head[m], mc[m].pending_count = count[m];
  std::vector<long long> idx((size_t)nslots, -2ll);
  DSM_HIP(hipMemcpy(R.d_states, hs.data(), hs.size() * sizeof(LMState), hipMemcpyHostToDevice));
  DSM_HIP(hipMemcpy(R.d_mc, mc, sizeof mc, hipMemcpyHostToDevice));
  DSM_HIP(hipMemcpy(R.d_idx, idx.data(), idx.size() * sizeof(long long), hipMemcpyHostToDevice));
  launch_tick_reserve(ctx->stream, ra, R.d_states, R.d_mc, R.d_idx);
  DSM_HIP(hipGetLastError());
  DSM_HIP(hipStreamSynchronize(ctx->stream));
  TickModeCtl got[2];
  DSM_HIP(hipMemcpy(got, R.d_mc, sizeof got, hipMemcpyDeviceToHost));
  DSM_HIP(hipMemcpy(idx.data(), R.d_idx, idx.size() * sizeof(long long), hipMemcpyDeviceToHost));
  memcpy(admit_idx, idx.data(), idx.size() * sizeof(long long));
  for (int m = 0; m < 2; m++) head_out[m] = got[m].pending_head, mc[m].pending_head = got[m].pending_head;
  *ctl_intact = memcmp(mc, got, sizeof mc) == 0 ? 1 : 0;
  return DSM_OK;
}

int dsm_diag_tick_stage(dsm_tracker *t, int mode, int n, const dsm_tick_slot *slots, const dsm_tick_list_cfg *list,
                        const dsm_tick_mode_ctl *ctl, int n_pending, const dsm_tick_pending *pending, int stepped, unsigned *items,
                        int *items_len, dsm_tick_seg_ctl *seg_out, dsm_tick_mode_ctl *ctl_out, dsm_tick_result *results,
                        dsm_tick_slot_out *slot_out, dsm_lm_step_state *state_out, unsigned char *state_raw, int *state_bytes,
                        unsigned char *start_raw) {
  const char *me = "dsm_diag_tick_stage";
  if (!t || !slots || !list || !ctl || !items_len || !state_bytes) return tick_invalid(me, "null argument");
  if (items && (!seg_out || !ctl_out || !results || !slot_out || !state_out || !state_raw || (n_pending > 0 && !start_raw)))
    return tick_invalid(me, "null argument");
  if (n < 1 || n > kDiagMaxSlots) return tick_invalid(me, "n is 1 .. 65536 (the item encoding holds the slot number)");
  long long slot_words = 0, needed = 0;
  for (int i = 0; i < n; i++) {
    const dsm_tick_slot &S = slots[i];
    if (S.status < ST_IDLE || S.status > ST_BAD_AFFINE) return tick_invalid(me, "a slot's status is 0 .. 4");
    if (S.lvl < 0 || S.lvl >= DSM_MAX_LEVELS) return tick_invalid(me, "a slot's level is out of range");
    if (S.reserve < 0 || S.reserve > 3) return tick_invalid(me, "reserve is 0 .. 3");
    if (S.n < 0 || S.ppt < 0 || S.ppt > 16 || ((S.status == ST_RUNNING || S.reserve == 1 || S.reserve == 2) && S.ppt < 1))
      return tick_invalid(me, "n >= 0 and ppt 1 .. 16 where the slot's evaluation is looked at");
    const int np = S.ppt > 0 ? tick_npos(chunks_of(S.n, S.ppt)) : 0;
    if (np >= (1 << kTickChunkBits)) return tick_invalid(me, "n is beyond the item encoding");
    if (S.reserve == 3 && (S.res_base < 0 || S.res_total < 0)) return tick_invalid(me, "negative res_base or res_total");
    slot_words += 4ll * np + (S.reserve == 3 ? S.res_total : 0);
  }
  const char *err = tick_rig_error(t, mode, n, list, ctl, n_pending, pending, slot_words, &needed);
  if (err) return tick_invalid(me, err);
  for (int i = 0; i < n; i++)
    if (slots[i].reserve == 3 && (long long)slots[i].res_base + slots[i].res_total > needed)
      return tick_invalid(me, "an explicit reservation lies outside the allocation");
  *state_bytes = (int)sizeof(LMState);
  if (!items) {
    *items_len = (int)needed;
    return DSM_OK;
  }
  if (*items_len < needed) return tick_invalid(me, "*items_len is smaller than cap + chain_cap + the guard region (ask with items NULL)");
  dsm_context *ctx = t->ctx;
  DSM_HIP(hipSetDevice(ctx->device));
  int rc = sync_desc(t);
  if (rc) return rc;
  TickRig R;
  rc = tick_rig_setup(R, t, n, slots, list, ctl, n_pending, pending, needed, /*desc_copy=*/false);
  if (rc) return rc;
  std::vector<LMState> hs((size_t)n);
  memset(hs.data(), 0, hs.size() * sizeof(LMState));
  for (int i = 0; i < n; i++) {
    LMState &S = hs[(size_t)i];
    const dsm_tick_slot &I = slots[i];
    S.status = I.status, S.lvl = I.lvl, S.is_scale = mode, S.stepped = I.stepped;
    S.in.n = I.n, S.in.ppt = I.ppt, S.in.residual_only = I.residual_only;
    S.spec_valid = I.spec_valid, S.n0 = I.n0, S.ticks = I.ticks;
    memcpy(S.cur, I.cur, sizeof S.cur), memcpy(S.aff_cur, I.aff_cur, sizeof S.aff_cur);
    memcpy(S.last_residuals, I.last_residuals, sizeof S.last_residuals), memcpy(S.flow, I.flow, sizeof S.flow);
    S.scale_cur = I.scale_cur;
    memcpy(S.evals, I.evals, sizeof S.evals), memcpy(S.evals_ro, I.evals_ro, sizeof S.evals_ro), memcpy(S.rounds, I.rounds, sizeof S.rounds);
  }
  DSM_HIP(hipMemcpy(R.d_states, hs.data(), hs.size() * sizeof(LMState), hipMemcpyHostToDevice));
  launch_diag_tick_stage(ctx->stream, mode, n, R.d_slots, R.d_trackers, R.d_states, R.list, R.d_mc, R.d_pending, R.d_results, R.d_slot_ticket, stepped);
  DSM_HIP(hipGetLastError());
  rc = tick_rig_collect(R, t, mode, n, ctl->ring, n_pending, TickOutputs{items, seg_out, ctl_out, results, slot_out, state_out, state_raw, start_raw});
  if (rc) return rc;
  *items_len = (int)needed;
  return DSM_OK;
}

int dsm_diag_tick_step(dsm_tracker *t, int mode, int lvl, int n, const dsm_lm_step_state *in, const dsm_tick_slot *slots,
                       const float *partials, long long partial_stride, int speculate, int opts, const dsm_tick_list_cfg *list,
                       const dsm_tick_mode_ctl *ctl, int n_pending, const dsm_tick_pending *pending, const long long *admit_idx,
                       unsigned *items, int *items_len, dsm_tick_seg_ctl *seg_out, dsm_tick_mode_ctl *ctl_out, dsm_tick_result *results,
                       dsm_tick_slot_out *slot_out, dsm_lm_step_state *state_out, unsigned char *state_raw, int *state_bytes,
                       unsigned char *start_raw) {
  const char *me = "dsm_diag_tick_step";
  if (!t || !in || !slots || !partials || !list || !ctl || !items_len || !state_bytes) return tick_invalid(me, "null argument");
  if (items && (!seg_out || !ctl_out || !results || !slot_out || !state_out || !state_raw || (n_pending > 0 && !start_raw)))
    return tick_invalid(me, "null argument");
  if (lvl < 0 || lvl >= t->nlevels) return tick_invalid(me, "level out of range");
  if (speculate < 0 || speculate > 2 || opts < 0 || opts > 7) return tick_invalid(me, "speculate is 0 .. 2, opts 0 .. 7");
  if (partial_stride < 8 || partial_stride % 8 || partial_stride > (1ll << 24)) return tick_invalid(me, "partial_stride is a multiple of 8, 8 .. 2^24");
  int top_nch = 0; // the largest evaluation a slot can hold when the LM launch reduces it: the caller's, or an admitted problem's first
  if (admit_idx)
    for (int l = 0; l < t->nlevels; l++) top_nch = level_chunks(t->desc, l) > top_nch ? level_chunks(t->desc, l) : top_nch;
  if (n < 1 || n > kDiagMaxSlots) return tick_invalid(me, "n is 1 .. 65536 (the item encoding holds the slot number)");
  long long slot_words = 0, needed = 0;
  for (int i = 0; i < n; i++) {
    if (in[i].nch < 0 || in[i].nch > 4096) return tick_invalid(me, "nch is 0 .. 4096");
    if (in[i].phase != PH_INIT && in[i].phase != PH_ITER) return tick_invalid(me, "phase is 0 or 1");
    if (slots[i].status != ST_IDLE && slots[i].status != ST_RUNNING) return tick_invalid(me, "a slot is idle (0) or running (1)");
    if (tick_npos(in[i].nch) >= (1 << kTickChunkBits)) return tick_invalid(me, "nch is beyond the item encoding");
    top_nch = in[i].nch > top_nch ? in[i].nch : top_nch;
    slot_words += 4ll * tick_npos(in[i].nch);
  }
  if ((long long)top_nch * kPartialStride > partial_stride / 2) return tick_invalid(me, "the partials of the largest evaluation do not fit partial_stride / 2");
  int lvl_npos = 0;
  for (int l = 0; l < t->nlevels; l++) lvl_npos = tick_npos(level_chunks(t->desc, l)) > lvl_npos ? tick_npos(level_chunks(t->desc, l)) : lvl_npos;
  slot_words += 4ll * lvl_npos * n; // a step may hand the problem down to any level; an admitted problem reserves and stages at the tracker's
  const char *err = tick_rig_error(t, mode, n, list, ctl, n_pending, pending, slot_words, &needed);
  if (err) return tick_invalid(me, err);
  if (admit_idx)
    for (int i = 0; i < n; i++)
      if (admit_idx[i] >= 0 && (admit_idx[i] < ctl->pending_head || admit_idx[i] >= ctl->pending_head + n_pending))
        return tick_invalid(me, "admit_idx names a ring entry nobody supplied");
  *state_bytes = (int)sizeof(LMState);
  if (!items) {
    *items_len = (int)needed;
    return DSM_OK;
  }
  if (*items_len < needed) return tick_invalid(me, "*items_len is smaller than cap + chain_cap + the guard region (ask with items NULL)");
  dsm_context *ctx = t->ctx;
  DSM_HIP(hipSetDevice(ctx->device));
  int rc = sync_desc(t);
  if (rc) return rc;
  const int expired_before = lm_spin_expired();
  if (expired_before < 0) return hip_fail(hipGetLastError(), "lm_spin_expired", __FILE__, __LINE__);
  {
    TickRig R;
    rc = tick_rig_setup(R, t, n, slots, list, ctl, n_pending, pending, needed, /*desc_copy=*/true);
    if (rc) return rc;
    dsm_lm_step_state *d_in = nullptr;
    float *d_partials = nullptr;
    long long *d_admit = nullptr;
    const size_t part_bytes = sizeof(float) * (size_t)partial_stride * (size_t)n;
    DSM_HIP(R.alloc(&d_in, (size_t)n));
    DSM_HIP(R.alloc(&d_partials, (size_t)partial_stride * (size_t)n));
    DSM_HIP(R.alloc(&d_admit, (size_t)n));
    DSM_HIP(hipMemcpy(d_in, in, sizeof(dsm_lm_step_state) * (size_t)n, hipMemcpyHostToDevice));
    DSM_HIP(hipMemcpy(d_partials, partials, part_bytes, hipMemcpyHostToDevice));
    if (admit_idx) DSM_HIP(hipMemcpy(d_admit, admit_idx, sizeof(long long) * (size_t)n, hipMemcpyHostToDevice));
    launch_diag_tick_fill(ctx->stream, mode, lvl, R.d_desc_copy, n, d_in, R.d_slots, R.d_states);
    if (admit_idx) launch_tick_admit(ctx->stream, mode, n, R.d_trackers, R.d_states, R.list, R.d_mc, R.d_pending, R.d_slot_ticket, d_admit);
    if (!(opts & 4))
      launch_tick_lm(ctx->stream, mode, n, R.d_trackers, R.d_states, d_partials, (int)partial_stride, R.list, R.d_mc, R.d_pending, R.d_results,
                     R.d_slot_ticket, speculate, opts & 3);
    DSM_HIP(hipGetLastError());
    rc = tick_rig_collect(R, t, mode, n, ctl->ring, n_pending, TickOutputs{items, seg_out, ctl_out, results, slot_out, state_out, state_raw, start_raw});
    if (rc) return rc;
  }
  const int expired_after = lm_spin_expired();
  if (expired_after != expired_before) {
    set_error("dsm_diag_tick_step: a bounded wait of the LM step's wave hand-shake expired");
    return DSM_ERR_STATE;
  }
  *items_len = (int)needed;
  return DSM_OK;
}

} // extern "C"
