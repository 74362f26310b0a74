// diag_capi.hip -- single evaluations and the diagnostic calls (dsm_tracker_calc_res_*, dsm_diag_*): one evaluation form or one LM
// proposal at a time on the buffers of the batch form, for the tests' exact checks.
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
