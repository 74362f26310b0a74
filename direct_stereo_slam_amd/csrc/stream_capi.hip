// stream_capi.hip -- the streaming (continuous-admission) form of the batched track / scale calls (dsm_stream_*).
//
// dsm_track_and_scale_batch is a synchronous call: every problem of the batch is taken from its first evaluation to its
// last before the call returns, so the lock-step launch schedule runs as many (evaluate, step) rounds per level as the
// SLOWEST problem needs -- 52 rounds on levels 2 and 3 of 512 distinct frames where the median problem needs 6 and 10 --
// and a third of the call is the dependency chain of a few dozen stragglers with the chip nearly idle.  The
// LM loop of a frame is sequential (TrackerAndScaler.cpp:505-593); frames of different sequences are independent
// (FrontEnd.cpp:585-686): the only parallelism there is lies ACROSS frames, and nothing says they must start and end together.
//
// A dsm_stream is a pool of resident LM problems (slots: track slots first, then scale slots) with a waiting queue in front and
// a result queue behind.  Problems take a slot when one is free and retire individually; dsm_stream_advance moves everything
// resident forward, by one of two engines over the same slot states (dsm_stream_set_engine; a switch wants the stream empty):
//  * TICK engine (engine 1, the default; stream_tick.hip: tick_setup / tick_advance / tick_collect): one tick advances every
//    resident problem by one LM round, whatever level it stands on -- per segment one evaluation launch over a device-built item
//    list and one LM launch.  Admission and retirement happen ON THE DEVICE: the host appends waiting problems to a ring, a slot freed by a retirement
//    takes the next one on the spot, results come back through a result ring.  An advance is a number of ticks, PIPELINED: it
//    returns once enqueued and reads back the advance before it.  One-chunk evaluations may run several rounds inside a tick
//    (chains, dsm_stream_set_chain).
//  * PASS engine (engine 0; stream_pass.hip: pass_advance and its steps): one pass = one sweep down the pyramid, coarsest level
//    first, with a fixed number of rounds per level -- the rounds MOST problems need (a quantile of what recently retired problems took).  A
//    problem that has not finished its level when the pass moves on simply stays where it is -- its LMState is resident in
//    device memory and resumable by construction -- and is CARRIED: in the next pass it rides with the newly admitted
//    problems' launches at that level, so a straggler's extra rounds cost no launches of their own.  The host admits and
//    retires between passes; no launch in a pass depends on a host read-back, the state is read back once per pass.
//
// Same evaluations, same LM steps, same partial order per problem as the batch form, in either engine: results are
// bit-identical (tests/test_stream.py); segments, fork / join, the (evaluate, step) round and the start / read-out rules are the
// batch form's own (lm_schedule.hip).  The work-queue kernel -- every problem at its own pace inside one launch -- was the other
// candidate for this; measured with the tail amortised over 2048 frames it runs at 42.7 k frames/s against 48.5 k for the
// launch form (profiles/r04_queue_form_b2048.json, r04_launch_form_b2048.json): its per-item cost is there in steady
// state too, so the streaming form is built on the launches.
//
// Hypothesis groups (dsm_stream_submit_hypotheses, stream_groups.hip): FrontEnd::trackNewCoarse's list of tries as one submission.  Its
// tries are ordinary track problems without abort thresholds; their results go to the group (route_result) instead of `done`, and the loop
// is replayed on the host by dsm_hypotheses_resolve (host_capi.cpp).  Host bookkeeping only: no launch or copy changes, with or without groups.
//
// This file: the pool itself -- create and destroy, the submissions and the host's waiting queues, tickets and `origin`, results, counts,
// statistics, the setters -- and the dispatch of an advance to the active engine.  stream_internal.hpp says which part of a dsm_stream
// belongs to whom.
#include <cstring>

#include "stream_internal.hpp"

using namespace dsm;

void dsm_stream::SlotArrays::release() {
  release_dev(d_tracker_ptrs), release_pinned(h_tracker_ptrs), release_dev(d_states), release_pinned(h_states), release_dev(d_partials);
  release_dev(d_start), release_pinned(h_start), release_dev(d_status), release_dev(d_tickets), release_dev(d_rowmap), release_pinned(h_rowmap);
  partial_stride = 0;
}

static void stream_free(dsm_stream *s) {
  s->arr.release();
  s->tick.release();
  delete s;
}

// the partials need the trackers' geometry: allocated on the first submission
static int stream_bind_geometry(dsm_stream *s, dsm_tracker *t) {
  if (s->arr.partial_stride) {
    if (t->w != s->w || t->h != s->h || t->nlevels != s->nlevels) return invalid("dsm_stream: all trackers of a stream must share image size and levels");
    return DSM_OK;
  }
  DSM_HIP(hipSetDevice(s->ctx->device));
  s->w = t->w, s->h = t->h, s->nlevels = t->nlevels;
  const int ps = 2 * max_chunks_upto(t->w * t->h) * kPartialStride; // second half: the speculative candidate's partials
  int rc = realloc_dev(&s->arr.d_partials, (size_t)s->N * ps);
  if (rc) return rc;
  s->arr.partial_stride = ps;
  return DSM_OK;
}

int dsm::submit_common(dsm_stream *s, int mode, int n, dsm_tracker *const *ts, int coarsest) {
  if (!s || n < 0 || (n && !ts)) return invalid("dsm_stream_submit: bad argument");
  if (s->cap[mode] == 0 && n) return invalid("dsm_stream_submit: the stream has no slots of this kind");
  for (int i = 0; i < n; i++) {
    dsm_tracker *t = ts[i];
    if (!t || t->ctx != s->ctx) return invalid("dsm_stream_submit: tracker does not belong to the stream's context");
    int rc = stream_bind_geometry(s, t);
    if (rc) return rc;
    if (coarsest < 0 || coarsest >= t->nlevels) return invalid("coarsest level out of range"); // :457 / :856
    rc = check_ready(t, mode);
    if (rc) return rc;
    if (s->tick.chain_max_n0 <= 0 || t->desc.lv[0].n <= s->tick.chain_max_n0) s->tick.chain_possible = true;
  }
  return DSM_OK;
}

// a problem of kind `mode` into the host's waiting queue; returns its ticket
static uint64_t enqueue(dsm_stream *s, int mode, dsm_tracker *t, const StartInfo &start) {
  const Waiting wq{s->next_ticket++, t, start};
  dsm_stream::Origin og;
  og.trk = t, og.admitted_at = -1;
  memcpy(og.pose0, start.pose, sizeof og.pose0);
  memcpy(og.aff0, start.aff, sizeof og.aff0);
  s->origin[wq.ticket] = og;
  s->waiting[mode].push_back(wq);
  return wq.ticket;
}
uint64_t dsm::enqueue_track(dsm_stream *s, dsm_tracker *t, const double *pose0, const double *aff0, int coarsest_lvl, const double *min_res) {
  StartInfo start;
  fill_track_start(start, pose0, aff0, min_res, coarsest_lvl);
  return enqueue(s, 0, t, start);
}

std::unordered_map<uint64_t, dsm_stream::Origin>::iterator dsm::origin_of(dsm_stream *s, uint64_t ticket) {
  auto it = s->origin.find(ticket);
  if (it == s->origin.end()) set_error("internal: a problem retired with an unknown ticket");
  return it;
}

extern "C" {

int dsm_stream_create(dsm_context *ctx, int track_slots, int scale_slots, dsm_stream **out) {
  if (!ctx || !out || track_slots < 0 || scale_slots < 0 || track_slots + scale_slots < 1) return invalid("dsm_stream_create: bad argument");
  *out = nullptr;
  DSM_HIP(hipSetDevice(ctx->device));
  dsm_stream *s = new dsm_stream();
  s->ctx = ctx;
  s->cap[0] = track_slots, s->cap[1] = scale_slots;
  const int N = s->N = track_slots + scale_slots;
  s->pass.slots.resize(N);
  int rc = DSM_OK;
  if (!rc) rc = realloc_dev(&s->arr.d_tracker_ptrs, N);
  if (!rc) rc = realloc_pinned(&s->arr.h_tracker_ptrs, N);
  if (!rc) rc = realloc_dev(&s->arr.d_states, N);
  if (!rc) rc = realloc_pinned(&s->arr.h_states, N);
  if (!rc) rc = realloc_dev(&s->arr.d_start, N);
  if (!rc) rc = realloc_pinned(&s->arr.h_start, N);
  if (!rc) rc = realloc_dev(&s->arr.d_status, 2 * (size_t)N);
  if (!rc) rc = realloc_dev(&s->arr.d_tickets, N);
  if (!rc) rc = realloc_dev(&s->arr.d_rowmap, (size_t)(DSM_MAX_LEVELS + 1) * N);
  if (!rc) rc = realloc_pinned(&s->arr.h_rowmap, (size_t)(DSM_MAX_LEVELS + 1) * N);
  if (!rc) {
    hipError_t e = hipMemsetAsync(s->arr.d_tickets, 0, sizeof(int) * N, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(s->arr.d_states, 0, sizeof(LMState) * N, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) rc = hip_fail(e, "dsm_stream_create: clearing the slot arrays", __FILE__, __LINE__);
  }
  if (rc) {
    stream_free(s);
    return rc;
  }
  memset(s->arr.h_tracker_ptrs, 0, sizeof(TrackerDev *) * N);
  memset(s->arr.h_start, 0, sizeof(StartInfo) * N);
  *out = s;
  return DSM_OK;
}

int dsm_stream_destroy(dsm_stream *s) {
  if (!s) return DSM_OK;
  hipSetDevice(s->ctx->device);
  hipStreamSynchronize(s->ctx->stream);
  for (hipStream_t st : s->ctx->groups.extra_streams) hipStreamSynchronize(st);
  if (s->ctx->groups.companion_stream) hipStreamSynchronize(s->ctx->groups.companion_stream);
  stream_free(s);
  return DSM_OK;
}

int dsm_stream_set_quantile(dsm_stream *s, int lvl, double q) {
  if (!s || !(q > 0.0 && q <= 1.0) || lvl >= DSM_MAX_LEVELS) return invalid("dsm_stream_set_quantile: level < DSM_MAX_LEVELS (negative: all), 0 < q <= 1");
  for (int l = 0; l < DSM_MAX_LEVELS; l++)
    if (lvl < 0 || l == lvl) s->pass.quantile[l] = q;
  return DSM_OK;
}

int dsm_stream_set_engine(dsm_stream *s, int engine, int ticks_per_advance) {
  if (!s || engine < 0 || engine > 1 || ticks_per_advance < -1 || ticks_per_advance > 4096)
    return invalid("dsm_stream_set_engine: engine 0 / 1, ticks -1 (the stream's own choice), 0 (keep), 1 .. 4096");
  if (engine != s->engine) {
    // both engines share the slot states: a switch needs the stream EMPTY on the device -- every advance read back (the pipelined
    // counts are one advance old), nothing resident, nothing handed to the device's waiting ring and not yet admitted
    if (s->engine == 1 && s->tick.ready) {
      DSM_HIP(hipSetDevice(s->ctx->device));
      const int rc = tick_sync(s);
      if (rc) return rc;
    }
    int resident = 0;
    dsm_stream_counts(s, &resident, nullptr, nullptr);
    if (resident || s->tick.in_transit()) return invalid("dsm_stream_set_engine: problems are resident or on their way to the device (drain the stream first)");
  }
  s->engine = engine;
  if (ticks_per_advance > 0) s->tick.ticks = ticks_per_advance, s->tick.auto_ticks = false;
  if (ticks_per_advance < 0) s->tick.auto_ticks = true;
  return DSM_OK;
}

int dsm_stream_set_chain(dsm_stream *s, int max_rounds) {
  if (!s || max_rounds < -1 || max_rounds > 4096) return invalid("dsm_stream_set_chain: rounds 0 (off) .. 4096, or -1 (the default)");
  s->tick.chain_rounds = max_rounds < 0 ? DSM_STREAM_CHAIN_DEFAULT : max_rounds; // (takes effect with the next advance: the lists of both kinds are read every tick)
  s->tick.chain_max_n0 = max_rounds < 0 ? DSM_STREAM_CHAIN_DEFAULT_MAX_N0 : 0;
  if (max_rounds > 0) s->tick.chain_possible = true; // (a bound named by the caller applies to every problem)
  return DSM_OK;
}

int dsm_stream_set_rounds(dsm_stream *s, int mode, const int *rounds_per_level) {
  if (!s || mode < 0 || mode > 1) return invalid("dsm_stream_set_rounds: bad argument");
  for (int l = 0; l < DSM_MAX_LEVELS; l++) s->pass.fixed_rounds[mode][l] = rounds_per_level ? rounds_per_level[l] : 0;
  return DSM_OK;
}

int dsm_stream_submit_track(dsm_stream *s, int n, dsm_tracker *const *ts, const double *pose0, const double *aff0, int coarsest_lvl,
                            const double *min_res_for_abort, uint64_t *tickets_out) {
  if (n && (!pose0 || !aff0)) return invalid("dsm_stream_submit_track: null pose/aff");
  int rc = submit_common(s, 0, n, ts, coarsest_lvl);
  if (rc) return rc;
  for (int i = 0; i < n; i++) {
    const uint64_t tk = enqueue_track(s, ts[i], pose0 + 7 * i, aff0 + 2 * i, coarsest_lvl, min_res_for_abort ? min_res_for_abort + DSM_MAX_LEVELS * i : nullptr);
    if (tickets_out) tickets_out[i] = tk;
  }
  return DSM_OK;
}

int dsm_stream_submit_scale(dsm_stream *s, int n, dsm_tracker *const *ts, const float *scale0, int coarsest_lvl, uint64_t *tickets_out) {
  if (n && !scale0) return invalid("dsm_stream_submit_scale: null scale");
  int rc = submit_common(s, 1, n, ts, coarsest_lvl);
  if (rc) return rc;
  for (int i = 0; i < n; i++) {
    StartInfo start;
    fill_scale_start(start, scale0[i], coarsest_lvl);
    const uint64_t tk = enqueue(s, 1, ts[i], start);
    if (tickets_out) tickets_out[i] = tk;
  }
  return DSM_OK;
}

int dsm_stream_counts(dsm_stream *s, int *resident_out, int *waiting_out, int *results_out) {
  if (!s) return invalid("null stream");
  // the tick engine's figures are as of the last read-back: in a slot / in the device's waiting ring
  const long long on_the_way = s->engine == 1 ? s->tick.on_the_way(0) + s->tick.on_the_way(1) : 0;
  if (resident_out) *resident_out = s->engine == 1 ? tick_resident(s) : pass_resident(s);
  if (waiting_out) *waiting_out = (int)(s->waiting[0].size() + s->waiting[1].size() + on_the_way);
  if (results_out) *results_out = (int)s->done.size();
  return DSM_OK;
}

int dsm_stream_results(dsm_stream *s, int max_results, dsm_stream_result *out, int *n_out) {
  if (!s || max_results < 0 || (max_results && !out) || !n_out) return invalid("dsm_stream_results: bad argument");
  *n_out = pop_results(s->done, max_results, out);
  return DSM_OK;
}

int dsm_stream_get_stats(dsm_stream *s, dsm_stats *track_out, dsm_stats *scale_out) {
  if (!s) return invalid("null stream");
  if (track_out) *track_out = s->stats[0];
  if (scale_out) *scale_out = s->stats[1];
  return DSM_OK;
}

int dsm_stream_get_schedule(dsm_stream *s, int mode, int *rounds_out, long long *passes_out, long long *retired_out, long long *carried_out) {
  if (!s || mode < 0 || mode > 1) return invalid("dsm_stream_get_schedule: bad argument");
  if (rounds_out)
    for (int l = 0; l < DSM_MAX_LEVELS; l++) rounds_out[l] = s->pass.rounds[mode][l];
  if (passes_out) *passes_out = s->advances_done;
  if (retired_out) *retired_out = s->retired[mode];
  if (carried_out) *carried_out = s->pass.carried_slot_passes;
  return DSM_OK;
}

int dsm_stream_advance(dsm_stream *s) {
  if (!s) return invalid("null stream");
  return s->engine == 1 ? tick_advance(s) : pass_advance(s);
}

int dsm_stream_sync(dsm_stream *s) {
  if (!s) return invalid("null stream");
  if (s->engine != 1 || !s->tick.ready) return DSM_OK;
  DSM_HIP(hipSetDevice(s->ctx->device));
  return tick_sync(s);
}

int dsm_stream_set_pipelined(dsm_stream *s, int on) {
  if (!s) return invalid("null stream");
  const int rc = dsm_stream_sync(s);
  if (rc) return rc;
  s->tick.pipelined = on != 0;
  return DSM_OK;
}

int dsm_stream_drain(dsm_stream *s) {
  if (!s) return invalid("null stream");
  long long last_retired = -1;
  int idle_advances = 0;
  for (;;) {
    int rc = dsm_stream_sync(s); // (the tail is short chains: nothing to overlap)
    const long long ret_now = s->retired[0] + s->retired[1];
    idle_advances = ret_now == last_retired ? idle_advances + 1 : 0;
    last_retired = ret_now;
    if (idle_advances > 4096) { // (a problem's whole life is a few dozen ticks)
      set_error("internal: dsm_stream_drain makes no progress");
      return DSM_ERR_STATE;
    }
    if (rc) return rc;
    int resident = 0, waiting = 0;
    dsm_stream_counts(s, &resident, &waiting, nullptr);
    if (resident == 0 && waiting == 0 && s->hyp.groups.empty()) { // (a group's next tries are queued when the try before them is read back)
      if (lm_spin_expired() != 0) { // (a wave hand-shake inside an LM step gave up waiting: results cannot be trusted -- never seen; the waits are bounded so that a defect shows here, not as a hung device)
        set_error("internal: a bounded wait inside an LM step expired");
        return DSM_ERR_STATE;
      }
      return DSM_OK;
    }
    rc = dsm_stream_advance(s);
    if (rc) return rc;
  }
}

} // extern "C"
