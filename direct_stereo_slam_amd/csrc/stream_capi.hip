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
//  * TICK engine (engine 1, the default; tick_setup / tick_advance / tick_collect): one tick advances every resident problem by one
//    LM round, whatever level it stands on -- per segment one evaluation launch over a device-built item list and one LM launch.
//    Admission and retirement happen ON THE DEVICE: the host appends waiting problems to a ring, a slot freed by a retirement
//    takes the next one on the spot, results come back through a result ring.  An advance is a number of ticks, PIPELINED: it
//    returns once enqueued and reads back the advance before it.  One-chunk evaluations may run several rounds inside a tick
//    (chains, dsm_stream_set_chain).
//  * PASS engine (engine 0; pass_advance and its steps): one pass = one sweep down the pyramid, coarsest level first, with a
//    fixed number of rounds per level -- the rounds MOST problems need (a quantile of what recently retired problems took).  A
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
// Hypothesis groups (dsm_stream_submit_hypotheses): FrontEnd::trackNewCoarse's list of tries as one submission.  Its tries are ordinary
// track problems without abort thresholds; their results go to the group (route_result) instead of `done`, and the loop is replayed on
// the host by dsm_hypotheses_resolve (host_capi.cpp).  Host bookkeeping only: no launch or copy changes, with or without groups.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <deque>
#include <unordered_map>
#include <vector>

#include "dsm_internal.hpp"

using namespace dsm;

namespace {

enum { SLOT_FREE = 0, SLOT_NEW = 1, SLOT_RUNNING = 2 };

struct Slot {
  int state = SLOT_FREE;
  uint64_t ticket = 0;
  dsm_tracker *trk = nullptr;
  int lvl = 0;    // NEW: coarsest level; RUNNING: the level the problem stood at after the last pass
  int passes = 0; // passes it has been resident for
  long long seen_evals[DSM_MAX_LEVELS] = {}, seen_ro[DSM_MAX_LEVELS] = {}; // evaluations already counted in the statistics
};

struct Waiting {
  uint64_t ticket;
  dsm_tracker *trk;
  StartInfo start;
};

constexpr size_t kHistCap = 4096; // retired problems whose round counts the schedule looks at

// A hypothesis group (dsm_stream_submit_hypotheses): the tries of FrontEnd::trackNewCoarse's loop as track problems without abort, their
// outputs kept by try, the loop replayed by dsm_hypotheses_resolve over the tries that are back in order.  Host bookkeeping only.
struct HypGroup {
  dsm_tracker *trk = nullptr;
  int n = 0, coarsest = 0;
  double aff_last[2] = {0, 0}, rmse0 = 0, thr = 0;
  std::vector<double> tries, pose, aff, last, flow; // n x 7 / n x 7 / n x 2 / n x DSM_MAX_LEVELS / n x 3
  std::vector<int> good;
  std::vector<char> back; // try i's result is back
  int prefix = 0;         // tries 0 .. prefix-1 are back
  int next = 1;           // the next try to queue (try 0 is queued at submission)
  int in_flight = 0;      // queued (waiting on the host or handed to the device) and not back
  int run = 0;            // tries whose results came back
  bool decided = false;
  long long born = 0;     // the stream's advance count at submission
  dsm_stream_hyp_result res{};
};

} // namespace

struct dsm_stream {
  dsm_context *ctx = nullptr;
  int cap[2] = {0, 0}; // slots of mode 0 (trackNewestCoarse) / mode 1 (optimizeScale); track slots come first
  int N = 0;
  int w = 0, h = 0, nlevels = 0; // geometry of the first tracker submitted; every tracker of the stream must share it
  int partial_stride = 0;
  TrackerDev **d_tracker_ptrs = nullptr, **h_tracker_ptrs = nullptr;
  LMState *d_states = nullptr, *h_states = nullptr;
  float *d_partials = nullptr;
  StartInfo *d_start = nullptr, *h_start = nullptr;
  int *d_status = nullptr;
  int *d_tickets = nullptr;
  int *d_rowmap = nullptr, *h_rowmap = nullptr; // [DSM_MAX_LEVELS + 1][N]: rows per level (relative to their segment), then the new slots (relative to their mode's base)
  std::vector<Slot> slots;
  std::deque<Waiting> waiting[2];
  std::deque<dsm_stream_result> done;
  uint64_t next_ticket = 1;
  double quantile[DSM_MAX_LEVELS] = {0.75, 0.75, 0.75, 0.75, 0.75, 0.75};
  int fixed_rounds[2][DSM_MAX_LEVELS] = {{0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0}}; // > 0: overrides the learnt schedule
  std::vector<int> hist[2][DSM_MAX_LEVELS];
  size_t hist_pos[2] = {0, 0};
  int rounds[2][DSM_MAX_LEVELS] = {{6, 8, 10, 12, 16, 16}, {4, 4, 4, 4, 4, 4}};
  int rounds_max[2][DSM_MAX_LEVELS] = {{12, 22, 52, 52, 52, 52}, {8, 8, 8, 8, 8, 8}}; // the most any retired problem needed (+ 1)
  dsm_stats stats[2]{};
  long long passes = 0, retired[2] = {0, 0}, carried_slot_passes = 0;
  // ---- tick engine (engine 1): every resident problem advances one LM round per tick, admission and retirement on the device ----
  int engine = 1;
  int ticks = 32; // ticks per advance (one host read-back per advance)
  bool tick_ready = false;
  std::vector<Seg> tsegs;
  TickSegCtl *d_segctl = nullptr, *h_segctl = nullptr;
  TickModeCtl *d_modectl = nullptr, *h_modectl = nullptr;
  std::vector<unsigned *> d_items; // [segment][2]
  std::vector<int> items_cap, last_count, last_chain;
  // chains (tick_eval_kernel): LM rounds a problem whose pending evaluation is ONE chunk may run inside one tick, in the workgroup that
  // evaluates it; 0 = off (every round costs a tick).  A scheduling switch: results are bit-identical.
  int chain_rounds = DSM_STREAM_CHAIN_DEFAULT;
  bool chain_possible = false; // a problem the chains apply to was submitted at some time (else the evaluation launches go without the chains' code)
  int chain_max_n0 = DSM_STREAM_CHAIN_DEFAULT_MAX_N0; // the default chains semi-dense problems only; a number named by the caller: every problem
  // options of the tick kernels' LM step, both measured on (profiles/r06b_ab_lm_step.log, where they were switched through the environment):
  int chain_flags = 1; // bit 0: helper wave in a chain's LM step
  int lm_opts = 3;     // tick_lm_kernel: bit 0 helper waves, bit 1 the next items' place in the list reserved before the solve
  TickPending *d_pending[2] = {nullptr, nullptr}, *h_pending[2] = {nullptr, nullptr}; // waiting rings (device / pinned staging)
  TickResult *d_results[2] = {nullptr, nullptr}, *h_results[2] = {nullptr, nullptr};   // result rings (device / two pinned copies)
  int ring[2] = {0, 0};
  long long *h_count_word = nullptr; // pinned: the pending_count words of the two advances in flight
  hipEvent_t ev_begin[2] = {nullptr, nullptr}, ev_end[2] = {nullptr, nullptr};
  bool pipelined = true;       // advance returns once its work is enqueued; results surface one advance late
  // ticks per advance.  auto_ticks (the default until dsm_stream_set_engine names a number): as many as retire 7/8 of what the
  // advance hands over -- handed x (mean life of a problem in ticks, learnt from the retired ones) / slots x 7/8 (tick_advance)
  bool auto_ticks = true;
  double life_ticks = 0.0;
  int inflight_ticks[2] = {0, 0};
  long long collected = 0;     // advances whose read-back has been processed
  long long handed[2] = {0, 0}; // problems appended to the device's waiting ring so far
  struct Seen {
    long long admitted, retired;
  } seen[2];
  int inflight_parity[2] = {0, 0};
  bool inflight_timed[2] = {false, false}; // the advance was enqueued with per-dispatch events (dsm_context_set_timing)
  EvalTimer tm; // per-dispatch events of the advance in flight
  // scheduling switches of the problems in flight, BY VALUE (a tracker may be destroyed as soon as its own result is back -- ADVICE r04:
  // the stream used to keep a pointer into the first submitted tracker's params for its whole life); refreshed at every hand-over
  bool have_sched = false;
  int sched_fixed_schedule = 0, sched_speculate = 0;
  unsigned long long *d_slot_ticket = nullptr;
  long long *d_admit_idx = nullptr; // per slot: the waiting-ring entry it takes at the start of this advance, or -1 (tick_reserve_kernel)
  int parity = 0;
  int resident[2] = {0, 0};
  struct Origin {
    dsm_tracker *trk;
    double pose0[7], aff0[2];
    long long admitted_at; // advance in which the problem was handed to the device (-1: still waiting)
  };
  std::unordered_map<uint64_t, Origin> origin;
  long long advances = 0, total_ticks = 0;
  // ---- hypothesis groups ----
  std::unordered_map<uint64_t, HypGroup> groups;                // group ticket -> group, until its result is handed back
  std::unordered_map<uint64_t, std::pair<uint64_t, int>> member; // a group try's internal ticket -> (group ticket, try)
  std::deque<dsm_stream_hyp_result> hyp_done;
  int hyp_window = 0; // tries of a group waiting or resident at once after try 0; 0 = all
};

static void free_dev(void *p) { if (p) hipFree(p); }
static void free_pinned(void *p) { if (p) hipHostFree(p); }

// the tick engine's resources (tick_setup); safe on a partially set-up stream, leaves every pointer null
static void tick_free(dsm_stream *s) {
  auto dev = [](auto *&p) { free_dev(p), p = nullptr; };
  auto pin = [](auto *&p) { free_pinned(p), p = nullptr; };
  dev(s->d_segctl), pin(s->h_segctl), dev(s->d_modectl), pin(s->h_modectl);
  for (unsigned *&p : s->d_items) dev(p);
  s->d_items.clear();
  for (int m = 0; m < 2; m++) dev(s->d_pending[m]), pin(s->h_pending[m]), dev(s->d_results[m]), pin(s->h_results[m]);
  dev(s->d_slot_ticket), dev(s->d_admit_idx), pin(s->h_count_word);
  for (int k = 0; k < 2; k++) {
    if (s->ev_begin[k]) hipEventDestroy(s->ev_begin[k]);
    if (s->ev_end[k]) hipEventDestroy(s->ev_end[k]);
    s->ev_begin[k] = s->ev_end[k] = nullptr;
  }
  s->tick_ready = false;
}

static void stream_free(dsm_stream *s) {
  free_dev(s->d_tracker_ptrs), free_pinned(s->h_tracker_ptrs), free_dev(s->d_states), free_pinned(s->h_states), free_dev(s->d_partials);
  free_dev(s->d_start), free_pinned(s->h_start), free_dev(s->d_status), free_dev(s->d_tickets), free_dev(s->d_rowmap), free_pinned(s->h_rowmap);
  tick_free(s);
  delete s;
}

// the partials need the trackers' geometry: allocated on the first submission
static int stream_bind_geometry(dsm_stream *s, dsm_tracker *t) {
  if (s->partial_stride) {
    if (t->w != s->w || t->h != s->h || t->nlevels != s->nlevels) return invalid("dsm_stream: all trackers of a stream must share image size and levels");
    return DSM_OK;
  }
  DSM_HIP(hipSetDevice(s->ctx->device));
  s->w = t->w, s->h = t->h, s->nlevels = t->nlevels;
  const int ps = 2 * max_chunks_upto(t->w * t->h) * kPartialStride; // second half: the speculative candidate's partials
  int rc = realloc_dev(&s->d_partials, (size_t)s->N * ps);
  if (rc) return rc;
  s->partial_stride = ps;
  return DSM_OK;
}

static int tick_advance(dsm_stream *s);
static int tick_sync(dsm_stream *s, long long upto = -1);

extern "C" {

int dsm_stream_create(dsm_context *ctx, int track_slots, int scale_slots, dsm_stream **out) {
  if (!ctx || !out || track_slots < 0 || scale_slots < 0 || track_slots + scale_slots < 1) return invalid("dsm_stream_create: bad argument");
  *out = nullptr;
  DSM_HIP(hipSetDevice(ctx->device));
  dsm_stream *s = new dsm_stream();
  s->ctx = ctx;
  s->cap[0] = track_slots, s->cap[1] = scale_slots;
  const int N = s->N = track_slots + scale_slots;
  s->slots.resize(N);
  int rc = DSM_OK;
  if (!rc) rc = realloc_dev(&s->d_tracker_ptrs, N);
  if (!rc) rc = realloc_pinned(&s->h_tracker_ptrs, N);
  if (!rc) rc = realloc_dev(&s->d_states, N);
  if (!rc) rc = realloc_pinned(&s->h_states, N);
  if (!rc) rc = realloc_dev(&s->d_start, N);
  if (!rc) rc = realloc_pinned(&s->h_start, N);
  if (!rc) rc = realloc_dev(&s->d_status, 2 * (size_t)N);
  if (!rc) rc = realloc_dev(&s->d_tickets, N);
  if (!rc) rc = realloc_dev(&s->d_rowmap, (size_t)(DSM_MAX_LEVELS + 1) * N);
  if (!rc) rc = realloc_pinned(&s->h_rowmap, (size_t)(DSM_MAX_LEVELS + 1) * N);
  if (!rc) {
    hipError_t e = hipMemsetAsync(s->d_tickets, 0, sizeof(int) * N, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(s->d_states, 0, sizeof(LMState) * N, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) rc = hip_fail(e, "dsm_stream_create: clearing the slot arrays", __FILE__, __LINE__);
  }
  if (rc) {
    stream_free(s);
    return rc;
  }
  memset(s->h_tracker_ptrs, 0, sizeof(TrackerDev *) * N);
  memset(s->h_start, 0, sizeof(StartInfo) * N);
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
    if (lvl < 0 || l == lvl) s->quantile[l] = q;
  return DSM_OK;
}

int dsm_stream_set_engine(dsm_stream *s, int engine, int ticks_per_advance) {
  if (!s || engine < 0 || engine > 1 || ticks_per_advance < -1 || ticks_per_advance > 4096)
    return invalid("dsm_stream_set_engine: engine 0 / 1, ticks -1 (the stream's own choice), 0 (keep), 1 .. 4096");
  if (engine != s->engine) {
    // both engines share the slot states: a switch needs the stream EMPTY on the device -- every advance read back (the pipelined
    // counts are one advance old), nothing resident, nothing handed to the device's waiting ring and not yet admitted
    if (s->engine == 1 && s->tick_ready) {
      DSM_HIP(hipSetDevice(s->ctx->device));
      const int rc = tick_sync(s);
      if (rc) return rc;
    }
    int resident = 0;
    dsm_stream_counts(s, &resident, nullptr, nullptr);
    const bool on_the_way = s->handed[0] != s->seen[0].admitted || s->handed[1] != s->seen[1].admitted || s->collected != s->advances;
    if (resident || on_the_way) return invalid("dsm_stream_set_engine: problems are resident or on their way to the device (drain the stream first)");
  }
  s->engine = engine;
  if (ticks_per_advance > 0) s->ticks = ticks_per_advance, s->auto_ticks = false;
  if (ticks_per_advance < 0) s->auto_ticks = true;
  return DSM_OK;
}

int dsm_stream_set_chain(dsm_stream *s, int max_rounds) {
  if (!s || max_rounds < -1 || max_rounds > 4096) return invalid("dsm_stream_set_chain: rounds 0 (off) .. 4096, or -1 (the default)");
  s->chain_rounds = max_rounds < 0 ? DSM_STREAM_CHAIN_DEFAULT : max_rounds; // (takes effect with the next advance: the lists of both kinds are read every tick)
  s->chain_max_n0 = max_rounds < 0 ? DSM_STREAM_CHAIN_DEFAULT_MAX_N0 : 0;
  if (max_rounds > 0) s->chain_possible = true; // (a bound named by the caller applies to every problem)
  return DSM_OK;
}

int dsm_stream_set_rounds(dsm_stream *s, int mode, const int *rounds_per_level) {
  if (!s || mode < 0 || mode > 1) return invalid("dsm_stream_set_rounds: bad argument");
  for (int l = 0; l < DSM_MAX_LEVELS; l++) s->fixed_rounds[mode][l] = rounds_per_level ? rounds_per_level[l] : 0;
  return DSM_OK;
}

static int submit_common(dsm_stream *s, int mode, int n, dsm_tracker *const *ts, int coarsest, uint64_t *tickets_out) {
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
    if (s->chain_max_n0 <= 0 || t->desc.lv[0].n <= s->chain_max_n0) s->chain_possible = true;
  }
  (void)tickets_out;
  return DSM_OK;
}

} // extern "C"

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
// one trackNewestCoarse problem (min_res: DSM_MAX_LEVELS thresholds, NULL = no abort)
static uint64_t enqueue_track(dsm_stream *s, dsm_tracker *t, const double *pose0, const double *aff0, int coarsest_lvl, const double *min_res) {
  StartInfo start;
  fill_track_start(start, pose0, aff0, min_res, coarsest_lvl);
  return enqueue(s, 0, t, start);
}

// ---- hypothesis groups ----
static void group_queue_try(dsm_stream *s, uint64_t gt, HypGroup &g, int i) {
  const uint64_t tk = enqueue_track(s, g.trk, &g.tries[7 * (size_t)i], g.aff_last, g.coarsest, nullptr); // no abort: replayed by the resolver
  s->member[tk] = std::make_pair(gt, i);
  g.in_flight++;
}

// the group's tries that still wait on the host leave the queue (those on the device run to their end)
static void group_drop_waiting(dsm_stream *s, uint64_t gt, HypGroup &g) {
  std::deque<Waiting> &wq = s->waiting[0];
  auto keep_end = std::remove_if(wq.begin(), wq.end(), [&](const Waiting &w) {
    auto it = s->member.find(w.ticket);
    if (it == s->member.end() || it->second.first != gt) return false;
    s->member.erase(it);
    s->origin.erase(w.ticket);
    g.in_flight--;
    return true;
  });
  wq.erase(keep_end, wq.end());
}

// a retired track problem: a group try's result goes to its group, every other result to dsm_stream_results
static void route_result(dsm_stream *s, const dsm_stream_result &r) {
  auto mit = s->member.empty() ? s->member.end() : s->member.find(r.ticket);
  if (mit == s->member.end()) {
    s->done.push_back(r);
    return;
  }
  const uint64_t gt = mit->second.first;
  const int i = mit->second.second;
  s->member.erase(mit);
  HypGroup &g = s->groups.at(gt);
  g.in_flight--, g.run++;
  for (int l = 0; l < DSM_MAX_LEVELS; l++) g.res.evals[l] += r.evals[l];
  if (!g.decided) {
    g.good[i] = r.good;
    memcpy(&g.pose[7 * (size_t)i], r.pose, sizeof r.pose);
    memcpy(&g.aff[2 * (size_t)i], r.aff, sizeof r.aff);
    memcpy(&g.last[DSM_MAX_LEVELS * (size_t)i], r.last_residuals, sizeof r.last_residuals);
    memcpy(&g.flow[3 * (size_t)i], r.flow, sizeof r.flow);
    g.back[i] = 1;
    const int before = g.prefix;
    while (g.prefix < g.n && g.back[g.prefix]) g.prefix++;
    if (g.prefix > before) {
      int64_t evals[DSM_MAX_LEVELS];
      memcpy(evals, g.res.evals, sizeof evals);
      int decided = 0;
      dsm_hypotheses_resolve(g.n, g.tries.data(), g.aff_last, g.coarsest, g.rmse0, g.thr, g.prefix, g.good.data(), g.pose.data(), g.aff.data(),
                             g.last.data(), g.flow.data(), &g.res, &decided);
      memcpy(g.res.evals, evals, sizeof evals);
      g.decided = decided != 0;
    }
    if (g.decided)
      group_drop_waiting(s, gt, g);
    else { // try 0 did not settle the frame: keep `window` of the following tries queued, in try order
      const int w = s->hyp_window > 0 ? s->hyp_window : g.n;
      while (g.next < g.n && g.in_flight < w) group_queue_try(s, gt, g, g.next++);
    }
  }
  if (g.decided && g.in_flight == 0) { // nothing of the group is on the device any more: its result is handed back
    g.res.ticket = gt;
    g.res.tries_run = g.run;
    g.res.advances = (int)(s->passes - g.born);
    s->hyp_done.push_back(g.res);
    s->groups.erase(gt);
  }
}

template <typename T>
static int pop_results(std::deque<T> &q, int max_results, T *out) {
  int k = 0;
  for (; k < max_results && !q.empty(); q.pop_front()) out[k++] = q.front();
  return k;
}

// ---- pass engine (engine 0) --------------------------------------------------------------------------------------------
// One pass.  (i) waiting problems are admitted into free slots, (ii) their state machines are started, (iii) every level
// from the coarsest a resident problem stands on down to level 0 gets its rounds -- compact launches over the slots that
// can be at that level in this pass: the new ones and the carried ones standing at or above it -- (iv) the states are read
// back once; problems that terminated retire (dsm_stream_results), the others are carried.
struct Pass {
  std::vector<Seg> segs;            // the track slots' stream groups, then the scale slots
  std::vector<dsm_tracker *> fresh; // trackers of the problems admitted in this pass
  int n_new[2] = {0, 0};
  int n_live = 0, top = -1, top2 = -1; // resident problems; the coarsest level a track / a scale problem stands on
  const dsm_params *P = nullptr;       // scheduling switches: those of the first resident problem
  bool draining = false;
  int grid_x[DSM_MAX_LEVELS], level_pts[DSM_MAX_LEVELS];
  EvalTimer tm;
};

// (i) admission: a free slot of the problem's kind, in the stream group with the fewest resident problems
static void pass_admit(dsm_stream *s, Pass &p) {
  const int N = s->N, cap0 = s->cap[0];
  std::vector<Seg> &segs = p.segs;
  const int n_track_segs = (int)segs.size() - (s->cap[1] > 0 ? 1 : 0);
  for (int mode = 0; mode < 2; mode++) {
    std::deque<Waiting> &wq = s->waiting[mode];
    if (wq.empty()) continue;
    const int sg0 = mode == 0 ? 0 : n_track_segs, sg1 = mode == 0 ? n_track_segs : (int)segs.size();
    std::vector<int> live(segs.size(), 0), cursor(segs.size(), 0);
    for (int si = sg0; si < sg1; si++) {
      cursor[si] = segs[si].i0;
      for (int i = segs[si].i0; i < segs[si].i1; i++) live[si] += s->slots[i].state != SLOT_FREE;
    }
    while (!wq.empty()) {
      int best = -1;
      for (int si = sg0; si < sg1; si++)
        if (live[si] < segs[si].i1 - segs[si].i0 && (best < 0 || live[si] < live[best])) best = si;
      if (best < 0) break; // every slot of this kind is taken
      int &c = cursor[best];
      while (s->slots[c].state != SLOT_FREE) c++;
      const Waiting &wt = wq.front();
      Slot &sl = s->slots[c];
      sl = Slot();
      sl.state = SLOT_NEW;
      sl.ticket = wt.ticket;
      sl.trk = wt.trk;
      sl.lvl = wt.start.coarsest;
      s->h_start[c] = wt.start;
      s->h_tracker_ptrs[c] = wt.trk->d_desc;
      s->h_rowmap[(size_t)DSM_MAX_LEVELS * N + (mode == 0 ? 0 : cap0) + p.n_new[mode]] = c - (mode == 0 ? 0 : cap0);
      p.n_new[mode]++;
      p.fresh.push_back(wt.trk);
      live[best]++;
      wq.pop_front();
    }
  }
}

// what is resident after the admission; false: nothing
static bool pass_survey(dsm_stream *s, Pass &p) {
  for (int i = 0; i < s->N; i++) {
    const Slot &sl = s->slots[i];
    if (sl.state == SLOT_FREE) continue;
    p.n_live++;
    if (!p.P) p.P = &sl.trk->params;
    if (i < s->cap[0])
      p.top = sl.lvl > p.top ? sl.lvl : p.top;
    else
      p.top2 = sl.lvl > p.top2 ? sl.lvl : p.top2;
  }
  // Nothing is waiting and the pool is at most a quarter full: what is resident is the END of the job -- nothing rides with
  // the stragglers any more, so a pass gives every level the rounds the slowest retired problem needed (they finish in one or
  // two passes instead of one level per pass) and evaluates and steps in one fused launch per round.
  p.draining = s->waiting[0].empty() && s->waiting[1].empty() && 4 * p.n_live <= s->N;
  return p.n_live > 0;
}

// row maps: level L of segment sg = its slots that can stand on level L during this pass
static int pass_row_maps(dsm_stream *s, Pass &p) {
  const int N = s->N;
  for (int L = 0; L < s->nlevels; L++) {
    int max_chunks = 1, max_n = 0;
    for (int i = 0; i < N; i++) {
      const Slot &sl = s->slots[i];
      if (sl.state == SLOT_FREE) continue;
      const int n_l = sl.trk->desc.lv[L].n, c = level_chunks(sl.trk->desc, L);
      if (c > max_chunks) max_chunks = c;
      if (n_l > max_n) max_n = n_l;
    }
    p.grid_x[L] = max_chunks < 8 ? max_chunks : (max_chunks + 7) & ~7;
    p.level_pts[L] = max_n;
    for (Seg &sg : p.segs) {
      int r = 0;
      for (int i = sg.i0; i < sg.i1; i++)
        if (s->slots[i].state != SLOT_FREE && s->slots[i].lvl >= L) s->h_rowmap[(size_t)L * N + sg.i0 + r++] = i - sg.i0;
      sg.rows[L] = r;
    }
  }
  DSM_HIP(hipMemcpyAsync(s->d_rowmap, s->h_rowmap, sizeof(int) * (size_t)(DSM_MAX_LEVELS + 1) * N, hipMemcpyHostToDevice, s->ctx->stream));
  return DSM_OK;
}

// (ii) start the admitted problems (LM_OP_START over the list of new slots of each kind)
static int pass_start_admitted(dsm_stream *s, const Pass &p) {
  dsm_context *ctx = s->ctx;
  const int N = s->N;
  if (p.n_new[0] + p.n_new[1] == 0) return DSM_OK;
  DSM_HIP(hipMemcpyAsync(s->d_tracker_ptrs, s->h_tracker_ptrs, sizeof(TrackerDev *) * N, hipMemcpyHostToDevice, ctx->stream));
  DSM_HIP(hipMemcpyAsync(s->d_start, s->h_start, sizeof(StartInfo) * N, hipMemcpyHostToDevice, ctx->stream));
  for (int mode = 0; mode < 2; mode++) {
    if (!p.n_new[mode]) continue;
    const int base = mode == 0 ? 0 : s->cap[0];
    launch_lm(ctx->stream, mode, LM_OP_START, 0, p.n_new[mode], s->d_tracker_ptrs + base, s->d_states + base,
              s->d_partials + (size_t)base * s->partial_stride, s->partial_stride, s->d_start + base, nullptr, s->d_status + 2 * base, false,
              s->d_rowmap + (size_t)DSM_MAX_LEVELS * N + base);
  }
  return DSM_OK;
}

// (iii) the pass: the other segments' streams start behind the uploads and the START launches
static int pass_rounds(dsm_stream *s, Pass &p) {
  dsm_context *ctx = s->ctx;
  const LMBuffers B{s->d_tracker_ptrs, s->d_states, s->d_partials, s->partial_stride, s->d_tickets, s->d_status};
  int rc = fork_segments(ctx, p.segs);
  if (rc) return rc;
  for (int L = p.top > p.top2 ? p.top : p.top2; L >= 0; L--) {
    auto seg_rounds = [&](const Seg &sg) {
      int r = s->fixed_rounds[sg.mode][L] > 0 ? s->fixed_rounds[sg.mode][L] : p.draining ? s->rounds_max[sg.mode][L] : s->rounds[sg.mode][L];
      if (p.P->fixed_schedule > 0) r = 1 + p.P->fixed_schedule; // the benchmark schedule: every problem needs exactly 1 + K rounds
      return r < 1 ? 1 : r;
    };
    int kmax = 0;
    for (const Seg &sg : p.segs)
      if (sg.rows[L] > 0 && seg_rounds(sg) > kmax) kmax = seg_rounds(sg);
    for (int k = 0; k < kmax; k++)
      for (int si = (int)p.segs.size() - 1; si >= 0; si--) { // (the companion's round first, as in run_lm_batch)
        const Seg &sg = p.segs[si];
        if (k >= seg_rounds(sg)) continue;
        // a launch's points are its rows'; the fused step also for the drain's launches of up to 128 rows
        const int rows = sg.rows[L];
        const RoundShape R{p.grid_x[L], p.level_pts[L], (long long)rows * p.level_pts[L], rows, p.draining && rows <= 128};
        if ((rc = launch_round(ctx, B, *p.P, sg, L, k, s->d_rowmap + (size_t)L * s->N + sg.i0, R, p.tm))) return rc;
      }
    for (const Seg &sg : p.segs)
      if (sg.rows[L] > 0) s->stats[sg.mode].launches[L] += seg_rounds(sg);
  }
  DSM_HIP(hipGetLastError());
  return join_segments(ctx, p.segs);
}

// a resident problem has terminated: its result, its rounds into the schedule's history, its slot free
static void pass_retire(dsm_stream *s, Slot &sl, const LMState &S, int mode) {
  dsm_stream_result r;
  const auto og = s->origin.find(sl.ticket); // (what the problem started from: kept since its submission)
  fill_stream_result(r, S, mode, sl.ticket, sl.passes, og->second.pose0, og->second.aff0);
  s->origin.erase(og);
  route_result(s, r);
  s->retired[mode]++;
  for (int l = 0; l < s->nlevels; l++) {
    std::vector<int> &hv = s->hist[mode][l];
    if (hv.size() < kHistCap)
      hv.push_back((int)S.rounds[l]);
    else
      hv[s->hist_pos[mode] % kHistCap] = (int)S.rounds[l];
  }
  s->hist_pos[mode]++;
  sl = Slot();
}

// (iv) one read-back; what THIS pass evaluated goes into the statistics; terminated problems retire, the others are carried
static int pass_read_back(dsm_stream *s, Pass &p) {
  dsm_context *ctx = s->ctx;
  const int N = s->N, nlevels = s->nlevels;
  DSM_HIP(hipMemcpyAsync(s->h_states, s->d_states, sizeof(LMState) * N, hipMemcpyDeviceToHost, ctx->stream));
  DSM_HIP(hipEventRecord(ctx->timers.ev_total[1], ctx->stream));
  DSM_HIP(hipStreamSynchronize(ctx->stream));
  s->passes++;
  float ms = 0;
  DSM_HIP(hipEventElapsedTime(&ms, ctx->timers.ev_total[0], ctx->timers.ev_total[1]));
  s->stats[0].total_ms += ms, s->stats[1].total_ms += ms;
  s->stats[0].polls += 1;
  if (ctx->timers.timing) collect_eval_timing(ctx, p.tm.lvl, nlevels, s->stats[0]);
  for (int i = 0; i < N; i++) {
    Slot &sl = s->slots[i];
    if (sl.state == SLOT_FREE) continue;
    const int mode = i < s->cap[0] ? 0 : 1;
    const LMState &S = s->h_states[i];
    dsm_stats &st = s->stats[mode];
    sl.passes++;
    for (int l = 0; l < nlevels; l++) {
      const long long de = S.evals[l] - sl.seen_evals[l], dr = S.evals_ro[l] - sl.seen_ro[l];
      sl.seen_evals[l] = S.evals[l], sl.seen_ro[l] = S.evals_ro[l];
      st.evals[l] += de;
      st.evals_residual_only[l] += dr;
      st.algorithmic_bytes += de * eval_bytes(sl.trk, l);
    }
    if (S.status != ST_RUNNING) {
      pass_retire(s, sl, S, mode);
      continue;
    }
    if (sl.passes > 4096) {
      set_error("internal: a resident problem did not terminate within 4096 passes");
      return DSM_ERR_STATE;
    }
    sl.state = SLOT_RUNNING;
    sl.lvl = S.lvl;
    s->carried_slot_passes++;
  }
  return DSM_OK;
}

// the next pass's rounds per level: the quantile of what the recently retired problems needed
static void pass_learn(dsm_stream *s) {
  for (int mode = 0; mode < 2; mode++) {
    if (s->hist[mode][0].size() < 16) continue;
    std::vector<int> r;
    for (int l = 0; l < s->nlevels; l++) {
      r = s->hist[mode][l];
      size_t k = (size_t)(s->quantile[l] * (double)(r.size() - 1) + 0.5);
      if (k >= r.size()) k = r.size() - 1;
      std::nth_element(r.begin(), r.begin() + k, r.end());
      s->rounds[mode][l] = r[k] < 1 ? 1 : r[k];
      s->rounds_max[mode][l] = *std::max_element(r.begin(), r.end()) + 1;
    }
  }
}

static int pass_advance(dsm_stream *s) {
  dsm_context *ctx = s->ctx;
  DSM_HIP(hipSetDevice(ctx->device));
  Pass p;
  p.segs = build_segments(ctx->groups.n_streams, s->cap[0], 0, s->cap[1], 1);
  pass_admit(s, p);
  if (!pass_survey(s, p)) return DSM_OK;
  int rc = bind_streams(ctx, p.segs);
  if (rc) return rc;
  if (!p.fresh.empty() && (rc = sync_descs(ctx, p.fresh.data(), (int)p.fresh.size()))) return rc;
  DSM_HIP(hipEventRecord(ctx->timers.ev_total[0], ctx->stream));
  if ((rc = pass_row_maps(s, p)) || (rc = pass_start_admitted(s, p)) || (rc = pass_rounds(s, p)) || (rc = pass_read_back(s, p))) return rc;
  pass_learn(s);
  return DSM_OK;
}

extern "C" {

int dsm_stream_submit_track(dsm_stream *s, int n, dsm_tracker *const *ts, const double *pose0, const double *aff0, int coarsest_lvl,
                            const double *min_res_for_abort, uint64_t *tickets_out) {
  if (n && (!pose0 || !aff0)) return invalid("dsm_stream_submit_track: null pose/aff");
  int rc = submit_common(s, 0, n, ts, coarsest_lvl, tickets_out);
  if (rc) return rc;
  for (int i = 0; i < n; i++) {
    const uint64_t tk = enqueue_track(s, ts[i], pose0 + 7 * i, aff0 + 2 * i, coarsest_lvl, min_res_for_abort ? min_res_for_abort + DSM_MAX_LEVELS * i : nullptr);
    if (tickets_out) tickets_out[i] = tk;
  }
  return DSM_OK;
}

int dsm_stream_submit_hypotheses(dsm_stream *s, dsm_tracker *tracker, int n_tries, const double *tries, const double aff_last[2], int coarsest_lvl,
                                 double last_coarse_rmse0, double retrack_threshold, uint64_t *ticket_out) {
  if (!s || !tracker || n_tries < 1 || !tries || !aff_last || !ticket_out)
    return invalid("dsm_stream_submit_hypotheses: null stream / tracker / tries / aff_last / ticket_out, or n_tries < 1");
  if (s->cap[0] == 0) return invalid("dsm_stream_submit_hypotheses: the stream has no track slots");
  int rc = submit_common(s, 0, 1, &tracker, coarsest_lvl, nullptr);
  if (rc) return rc;
  const uint64_t gt = s->next_ticket++;
  HypGroup &g = s->groups[gt];
  g.trk = tracker, g.n = n_tries, g.coarsest = coarsest_lvl;
  g.aff_last[0] = aff_last[0], g.aff_last[1] = aff_last[1];
  g.rmse0 = last_coarse_rmse0, g.thr = retrack_threshold;
  g.tries.assign(tries, tries + 7 * (size_t)n_tries);
  g.pose.assign(7 * (size_t)n_tries, 0.0), g.aff.assign(2 * (size_t)n_tries, 0.0);
  g.last.assign(DSM_MAX_LEVELS * (size_t)n_tries, 0.0), g.flow.assign(3 * (size_t)n_tries, 0.0);
  g.good.assign(n_tries, 0), g.back.assign(n_tries, 0);
  g.born = s->passes;
  group_queue_try(s, gt, g, 0); // try 0 (the constant-motion guess): nothing achieved yet, so no abort threshold either
  *ticket_out = gt;
  return DSM_OK;
}

int dsm_stream_hypotheses_results(dsm_stream *s, int max_results, dsm_stream_hyp_result *out, int *n_out) {
  if (!s || max_results < 0 || (max_results && !out) || !n_out) return invalid("dsm_stream_hypotheses_results: bad argument");
  *n_out = pop_results(s->hyp_done, max_results, out);
  return DSM_OK;
}

int dsm_stream_hypotheses_counts(dsm_stream *s, int *pending_out, int *ready_out) {
  if (!s) return invalid("null stream");
  if (pending_out) *pending_out = (int)s->groups.size();
  if (ready_out) *ready_out = (int)s->hyp_done.size();
  return DSM_OK;
}

int dsm_stream_set_hypothesis_window(dsm_stream *s, int window) {
  if (!s || window < 0) return invalid("dsm_stream_set_hypothesis_window: window >= 1, or 0 for all of a group's tries");
  s->hyp_window = window;
  return DSM_OK;
}

int dsm_stream_submit_scale(dsm_stream *s, int n, dsm_tracker *const *ts, const float *scale0, int coarsest_lvl, uint64_t *tickets_out) {
  if (n && !scale0) return invalid("dsm_stream_submit_scale: null scale");
  int rc = submit_common(s, 1, n, ts, coarsest_lvl, tickets_out);
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
  int r = 0;
  for (const Slot &sl : s->slots) r += sl.state != SLOT_FREE;
  long long on_the_way = 0;
  if (s->engine == 1) { // as of the last read-back: in a slot / in the device's waiting ring
    r = (int)((s->seen[0].admitted - s->seen[0].retired) + (s->seen[1].admitted - s->seen[1].retired));
    on_the_way = (s->handed[0] - s->seen[0].admitted) + (s->handed[1] - s->seen[1].admitted);
  }
  if (resident_out) *resident_out = r;
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
    for (int l = 0; l < DSM_MAX_LEVELS; l++) rounds_out[l] = s->rounds[mode][l];
  if (passes_out) *passes_out = s->passes;
  if (retired_out) *retired_out = s->retired[mode];
  if (carried_out) *carried_out = s->carried_slot_passes;
  return DSM_OK;
}

int dsm_stream_advance(dsm_stream *s) {
  if (!s) return invalid("null stream");
  return s->engine == 1 ? tick_advance(s) : pass_advance(s);
}

} // extern "C"

// ---- tick engine (engine 1) --------------------------------------------------------------------------------------------
static int tick_setup(dsm_stream *s) {
  dsm_context *ctx = s->ctx;
  const int cap0 = s->cap[0], N = s->N;
  s->tsegs = build_segments(ctx->groups.n_streams, cap0, 0, s->cap[1], 1);
  const int nseg = (int)s->tsegs.size();
  tick_free(s); // (an earlier attempt that failed half way left its allocations behind: ADVICE r04)
  int rc = realloc_dev(&s->d_segctl, nseg);
  if (!rc) rc = realloc_pinned(&s->h_segctl, 2 * (size_t)nseg);
  if (!rc) rc = realloc_dev(&s->d_modectl, 2);
  if (!rc) rc = realloc_pinned(&s->h_modectl, 2 * 2);
  if (!rc) rc = realloc_pinned(&s->h_count_word, 4);
  if (!rc) rc = realloc_dev(&s->d_slot_ticket, N);
  if (!rc) rc = realloc_dev(&s->d_admit_idx, N);
  if (rc) return rc;
  // an item list holds at most one evaluation (+ its speculative twin) per slot of the segment
  const int maxpos = 8 * ((max_chunks_upto(s->w * s->h) + 7) / 8);
  if (maxpos >= (1 << kTickChunkBits)) return invalid("dsm_stream (tick engine): a level has too many chunks for the item encoding");
  if (N >= (1 << (30 - kTickChunkBits))) return invalid("dsm_stream (tick engine): too many slots for the item encoding");
  s->d_items.assign(2 * nseg, nullptr);
  s->items_cap.assign(nseg, 0);
  s->last_count.assign(nseg, 0);
  s->last_chain.assign(nseg, 0);
  for (int si = 0; si < nseg; si++) {
    const int ns = s->tsegs[si].i1 - s->tsegs[si].i0;
    const int cap = ns * 2 * maxpos + 64;
    s->items_cap[si] = cap;
    for (int b = 0; b < 2; b++) // item slots [0, cap), then one chain entry per slot of the segment
      if ((rc = realloc_dev(&s->d_items[2 * si + b], (size_t)cap + ns))) return rc;
  }
  DSM_HIP(hipMemsetAsync(s->d_segctl, 0, sizeof(TickSegCtl) * nseg, ctx->stream));
  DSM_HIP(hipMemsetAsync(s->d_slot_ticket, 0, sizeof(unsigned long long) * N, ctx->stream));
  // the waiting ring and the result ring of each kind: the host appends waiting problems and never lets more in than the result
  // ring has room for; the device consumes / produces by monotonic counters
  for (int mode = 0; mode < 2; mode++) {
    int ring = 1024;
    while (ring < 4 * s->cap[mode]) ring <<= 1;
    s->ring[mode] = ring;
    if ((rc = realloc_dev(&s->d_pending[mode], ring)) || (rc = realloc_pinned(&s->h_pending[mode], ring)) || (rc = realloc_dev(&s->d_results[mode], ring)) ||
        (rc = realloc_pinned(&s->h_results[mode], 2 * (size_t)ring)))
      return rc;
    TickModeCtl mc;
    memset(&mc, 0, sizeof mc);
    mc.ring = ring;
    s->h_modectl[mode] = mc;
  }
  DSM_HIP(hipMemcpyAsync(s->d_modectl, s->h_modectl, sizeof(TickModeCtl) * 2, hipMemcpyHostToDevice, ctx->stream));
  for (int k = 0; k < 2; k++) {
    DSM_HIP(hipEventCreate(&s->ev_begin[k]));
    DSM_HIP(hipEventCreate(&s->ev_end[k]));
  }
  DSM_HIP(hipStreamSynchronize(ctx->stream));
  memset(s->seen, 0, sizeof s->seen);
  s->tick_ready = true;
  return DSM_OK;
}

// the read-back of advance `k` (parity k & 1): control blocks and result rings are in the pinned copies once ev_end[k & 1] is reached
static int tick_collect(dsm_stream *s, long long k) {
  dsm_context *ctx = s->ctx;
  const int par = (int)(k & 1), nseg = (int)s->tsegs.size();
  DSM_HIP(hipEventSynchronize(s->ev_end[par]));
  float ms = 0;
  DSM_HIP(hipEventElapsedTime(&ms, s->ev_begin[par], s->ev_end[par]));
  s->stats[0].total_ms += ms, s->stats[1].total_ms += ms; // (the stream's statistics are cumulative)
  s->stats[0].polls += 1;
  if (s->inflight_timed[par]) collect_eval_timing(ctx, s->tm.lvl, 1, s->stats[0]);
  for (int si = 0; si < nseg; si++) {
    const TickSegCtl &sc = s->h_segctl[par * nseg + si];
    if (sc.overflow) {
      set_error("internal: an item list of the tick engine ran over");
      return DSM_ERR_STATE;
    }
    s->last_count[si] = sc.count[s->inflight_parity[par]];
    s->last_chain[si] = sc.chain[s->inflight_parity[par]];
  }
  for (int mode = 0; mode < 2; mode++) {
    const TickModeCtl &mc = s->h_modectl[par * 2 + mode];
    dsm_stream::Seen &sn = s->seen[mode];
    const int ring = s->ring[mode];
    const long long new_ret = mc.retired - sn.retired;
    if (new_ret < 0 || new_ret > ring) {
      set_error("internal: the tick engine's result ring ran over");
      return DSM_ERR_STATE;
    }
    dsm_stats &st = s->stats[mode];
    for (int l = 0; l < s->nlevels; l++) st.launches[l] += s->inflight_ticks[par];
    const TickResult *res = s->h_results[mode] + (size_t)par * ring;
    long long life_sum = 0;
    for (long long i = 0; i < new_ret; i++) {
      const TickResult &R = res[(sn.retired + i) & (ring - 1)];
      life_sum += R.ticks; // (= its LM rounds, less the rounds chains ran inside one tick)
      auto it = s->origin.find(R.ticket);
      if (it == s->origin.end()) {
        set_error("internal: the tick engine returned an unknown ticket");
        return DSM_ERR_STATE;
      }
      const dsm_stream::Origin &og = it->second;
      dsm_stream_result r;
      fill_stream_result(r, R, mode, R.ticket, (int)(k - og.admitted_at + 1), og.pose0, og.aff0);
      // evaluations and SURVEY.md 8d's bytes, booked when the problem retires (exact per problem; a long run's average equals the
      // bytes moved).  Not from the device's count of staged evaluations (TickModeCtl::sched_evals / sched_ro): a speculative
      // candidate that the LM step consumes is an evaluation of the problem's (LMState::evals, as the batch form counts) and is
      // not staged as one -- a drained stream reported fewer residual-only evaluations than the batch calls (15 against 20 on a level).
      for (int l = 0; l < s->nlevels; l++) {
        st.evals[l] += R.evals[l];
        st.evals_residual_only[l] += R.evals_ro[l];
        st.algorithmic_bytes += R.evals[l] * eval_bytes(og.trk, l);
      }
      s->retired[mode]++;
      s->origin.erase(it); // (before route_result: a group's next tries are added to `origin`)
      route_result(s, r);
    }
    if (new_ret > 0 && mode == (s->cap[0] > 0 ? 0 : 1)) { // (a tick = one LM round of every resident problem)
      const double mean = (double)life_sum / (double)new_ret;
      s->life_ticks = s->life_ticks > 0.0 ? 0.75 * s->life_ticks + 0.25 * mean : mean;
    }
    sn.retired = mc.retired;
    sn.admitted = mc.pending_head;
    s->resident[mode] = (int)(sn.admitted - sn.retired);
  }
  return DSM_OK;
}

// the advances before `upto` are read back (default: everything in flight)
static int tick_sync(dsm_stream *s, long long upto) {
  while (s->collected < (upto < 0 ? s->advances : upto)) {
    const int rc = tick_collect(s, s->collected);
    if (rc) return rc;
    s->collected++;
  }
  return DSM_OK;
}

// One advance of the tick engine, PIPELINED: waiting problems are appended to the device's waiting ring, free slots take them,
// then `ticks` ticks -- evaluate every staged item, step every resident problem; finished problems retire into the result ring and
// their slots take the next waiting problem on the spot -- and the control blocks and result rings are copied back behind them.
// The call returns as soon as that is ENQUEUED; what it reads back is the PREVIOUS advance's (its kernels ran while the host
// prepared this one), so results surface one advance late and the device never waits for the host (dsm_stream_sync / drain wait
// for everything).  With dsm_context_set_timing the advance is synchronous (its events are read right away).
struct Advance {
  long long k, par; // its number; its pinned copies are those of parity par = k & 1
  int n_new[2];      // problems handed over, per kind
  bool may_admit[2]; // something may be waiting on the device
  int T, speculate, chain_rounds;
};

// waiting problems -> the device's ring: as many as the waiting ring and the result ring have room for
static int tick_hand_over(dsm_stream *s, Advance &a) {
  dsm_context *ctx = s->ctx;
  std::vector<dsm_tracker *> fresh;
  for (int mode = 0; mode < 2; mode++) {
    const int ring = s->ring[mode];
    const long long room = std::min<long long>(ring - (s->handed[mode] - s->seen[mode].admitted), ring - (s->handed[mode] - s->seen[mode].retired));
    const int n = (int)std::min<long long>((long long)s->waiting[mode].size(), room > 0 ? room : 0);
    a.n_new[mode] = n;
    for (int i = 0; i < n; i++) {
      const Waiting &wt = s->waiting[mode].front();
      TickPending &pd = s->h_pending[mode][(s->handed[mode] + i) & (ring - 1)];
      pd.start = wt.start;
      pd.trk = wt.trk->d_desc;
      pd.ticket = wt.ticket;
      fresh.push_back(wt.trk);
      s->sched_fixed_schedule = wt.trk->params.fixed_schedule, s->sched_speculate = wt.trk->params.speculate, s->have_sched = true;
      auto it = s->origin.find(wt.ticket);
      if (it != s->origin.end()) it->second.admitted_at = a.k;
      s->waiting[mode].pop_front();
    }
  }
  if (!s->have_sched) return invalid("dsm_stream: internal: no problem was ever handed over");
  int rc;
  if (!fresh.empty() && (rc = sync_descs(ctx, fresh.data(), (int)fresh.size()))) return rc;
  DSM_HIP(hipEventRecord(s->ev_begin[a.par], ctx->stream));
  if (ctx->timers.timing) DSM_HIP(hipEventRecord(ctx->timers.ev_total[0], ctx->stream)); // (collect_eval_timing places the dispatches relative to it)
  for (int mode = 0; mode < 2; mode++) {
    if (!a.n_new[mode]) continue;
    const int ring = s->ring[mode];
    const int first = (int)(s->handed[mode] & (ring - 1)), n1 = std::min(a.n_new[mode], ring - first);
    DSM_HIP(hipMemcpyAsync(s->d_pending[mode] + first, s->h_pending[mode] + first, sizeof(TickPending) * n1, hipMemcpyHostToDevice, ctx->stream));
    if (a.n_new[mode] > n1)
      DSM_HIP(hipMemcpyAsync(s->d_pending[mode], s->h_pending[mode], sizeof(TickPending) * (a.n_new[mode] - n1), hipMemcpyHostToDevice, ctx->stream));
    s->handed[mode] += a.n_new[mode];
    s->h_count_word[a.par * 2 + mode] = s->handed[mode];
    DSM_HIP(hipMemcpyAsync(&s->d_modectl[mode].pending_count, &s->h_count_word[a.par * 2 + mode], sizeof(long long), hipMemcpyHostToDevice, ctx->stream));
  }
  for (int mode = 0; mode < 2; mode++) a.may_admit[mode] = s->handed[mode] > s->seen[mode].admitted;
  return DSM_OK;
}

// the advance's ticks and the switches of its launches
static void tick_plan(dsm_stream *s, Advance &a) {
  a.T = s->ticks;
  if (s->auto_ticks && s->life_ticks > 0.0) {
    const int m = s->cap[0] > 0 ? 0 : 1;
    // sized to retire 7/8 of what the advance hands over: the rest stays in the device's waiting ring as the buffer from which a slot
    // freed by a retirement is refilled on the spot (a caller that hands over a full pool every advance builds a backlog of an eighth of
    // a pool per advance; it is worked off at full occupancy when the caller stops).  Nothing handed over: the residents' own life.
    // (With dsm_params.fixed_schedule every problem lives the same number of ticks and a cohort admitted together stays on one level,
    // which evaluates in larger single-level launches: there an advance is one cohort's whole life.)
    const double share = s->sched_fixed_schedule > 0 ? 1.0 : 0.875;
    const double t = a.n_new[m] > 0 ? share * (double)a.n_new[m] * s->life_ticks / (double)s->cap[m] : s->life_ticks;
    a.T = (int)std::ceil(t);
    a.T = a.T < 8 ? 8 : a.T > 256 ? 256 : a.T;
  }
  s->inflight_ticks[a.par] = a.T;
  a.speculate = s->sched_fixed_schedule > 0 ? 0 : s->sched_speculate;
  // (with dsm_params.fixed_schedule a cohort moves in lock step and an advance is its whole life: chains would only unbalance it)
  a.chain_rounds = (s->sched_fixed_schedule > 0 || !s->chain_possible) ? 0 : s->chain_rounds;
}

// the list of segment si that buffer `buf` of its items is
static TickList tick_list(const dsm_stream *s, int si, int buf, int chain_rounds) {
  const Seg &sg = s->tsegs[si];
  return TickList{s->d_items[2 * si + buf], s->d_segctl + si, buf, s->items_cap[si], chain_rounds > 0 ? sg.i1 - sg.i0 : 0, s->chain_max_n0};
}

// which free slot takes which waiting problem (one launch, before the stream groups fork), then every segment's free slots take theirs
static int tick_reserve_and_admit(dsm_stream *s, const Advance &a) {
  dsm_context *ctx = s->ctx;
  const int nseg = (int)s->tsegs.size();
  if (a.may_admit[0] || a.may_admit[1]) {
    TickReserveArgs ra;
    if (nseg > kTickMaxSegs) return invalid("dsm_stream: too many stream groups");
    ra.nseg = nseg;
    for (int si = 0; si < nseg; si++) ra.seg[si] = TickSegDesc{s->tsegs[si].mode, s->tsegs[si].i0, s->tsegs[si].i1 - s->tsegs[si].i0};
    launch_tick_reserve(ctx->stream, ra, s->d_states, s->d_modectl, s->d_admit_idx);
  }
  const int rc = fork_segments(ctx, s->tsegs);
  if (rc) return rc;
  for (int si = nseg - 1; si >= 0; si--) {
    const Seg &sg = s->tsegs[si];
    const int i0 = sg.i0, ns = sg.i1 - sg.i0, mode = sg.mode;
    if (a.may_admit[mode]) // (free slots take what tick_reserve_kernel gave them)
      launch_tick_admit(sg.st, mode, ns, (const TrackerDev **)s->d_tracker_ptrs + i0, s->d_states + i0, tick_list(s, si, s->parity, a.chain_rounds),
                        s->d_modectl + mode, s->d_pending[mode], s->d_slot_ticket + i0, s->d_admit_idx + i0);
  }
  return DSM_OK;
}

// T ticks: per segment one evaluation launch over its item list and one LM launch over its slots
static int tick_ticks(dsm_stream *s, const Advance &a) {
  dsm_context *ctx = s->ctx;
  const int nseg = (int)s->tsegs.size();
  s->tm.used = 0;
  s->tm.lvl.clear();
  for (int t = 0; t < a.T; t++) {
    const int buf = (s->parity + t) & 1;
    for (int si = nseg - 1; si >= 0; si--) {
      const Seg &sg = s->tsegs[si];
      const int i0 = sg.i0, ns = sg.i1 - sg.i0, mode = sg.mode;
      // grid: what the segment's list held at the end of the last advance read back, plus slack (the kernel strides over a longer list)
      long long grid = (long long)(s->last_count[si] + s->last_chain[si]) * 5 / 4 + 256;
      if (s->last_count[si] + s->last_chain[si] == 0) grid = (long long)ns * 16;
      if (grid > s->items_cap[si]) grid = s->items_cap[si];
      float *part = s->d_partials + (size_t)i0 * s->partial_stride;
      hipEvent_t eb = nullptr;
      const int rc = timed_eval_begin(ctx, sg, 0, s->tm, &eb); // (all levels in one launch: booked under index 0)
      if (rc) return rc;
      const TickList next = tick_list(s, si, buf ^ 1, a.chain_rounds);
      const TickChainArgs chain{(const TrackerDev **)s->d_tracker_ptrs + i0, s->d_states + i0, next, s->d_modectl + mode, s->d_pending[mode], s->d_results[mode],
                                s->d_slot_ticket + i0, a.chain_rounds, s->chain_flags};
      launch_tick_eval(sg.st, mode, (int)grid, s->d_states + i0, part, s->partial_stride, s->d_items[2 * si + buf], s->d_segctl + si, buf, s->items_cap[si], chain, s->chain_possible);
      if (eb) DSM_HIP(hipEventRecord(eb, sg.st));
      launch_tick_lm(sg.st, mode, ns, (const TrackerDev **)s->d_tracker_ptrs + i0, s->d_states + i0, part, s->partial_stride, next, s->d_modectl + mode,
                     s->d_pending[mode], s->d_results[mode], s->d_slot_ticket + i0, a.speculate, s->lm_opts);
    }
  }
  s->parity = (s->parity + a.T) & 1;
  s->inflight_parity[a.par] = s->parity;
  s->inflight_timed[a.par] = ctx->timers.timing;
  DSM_HIP(hipGetLastError());
  return DSM_OK;
}

// read-back behind the ticks: control blocks and the result rings, into this advance's pinned copies
static int tick_read_back(dsm_stream *s, const Advance &a) {
  dsm_context *ctx = s->ctx;
  const int nseg = (int)s->tsegs.size(), par = a.par;
  const int rc = join_segments(ctx, s->tsegs);
  if (rc) return rc;
  DSM_HIP(hipMemcpyAsync(s->h_modectl + par * 2, s->d_modectl, sizeof(TickModeCtl) * 2, hipMemcpyDeviceToHost, ctx->stream));
  DSM_HIP(hipMemcpyAsync(s->h_segctl + par * nseg, s->d_segctl, sizeof(TickSegCtl) * nseg, hipMemcpyDeviceToHost, ctx->stream));
  for (int mode = 0; mode < 2; mode++)
    if (s->handed[mode] > s->seen[mode].retired) // (results may appear)
      DSM_HIP(hipMemcpyAsync(s->h_results[mode] + (size_t)par * s->ring[mode], s->d_results[mode], sizeof(TickResult) * s->ring[mode], hipMemcpyDeviceToHost,
                             ctx->stream));
  DSM_HIP(hipEventRecord(s->ev_end[par], ctx->stream));
  return DSM_OK;
}

static int tick_advance(dsm_stream *s) {
  dsm_context *ctx = s->ctx;
  DSM_HIP(hipSetDevice(ctx->device));
  if (!s->partial_stride) return DSM_OK; // nothing was ever submitted
  int rc;
  if (!s->tick_ready && (rc = tick_setup(s))) return rc;
  if (s->collected == s->advances && s->resident[0] + s->resident[1] == 0 && s->waiting[0].empty() && s->waiting[1].empty() &&
      s->handed[0] == s->seen[0].admitted && s->handed[1] == s->seen[1].admitted)
    return DSM_OK; // idle
  if ((rc = bind_streams(ctx, s->tsegs))) return rc;
  if ((s->advances - s->collected >= 2 || ctx->timers.timing) && (rc = tick_sync(s))) return rc; // (at most one advance behind: the pinned copies are two deep;
                                                                                          // a timed advance reads its own events alone)
  Advance a{};
  a.k = s->advances;
  a.par = a.k & 1;
  if ((rc = tick_hand_over(s, a))) return rc;
  tick_plan(s, a);
  if ((rc = tick_reserve_and_admit(s, a)) || (rc = tick_ticks(s, a)) || (rc = tick_read_back(s, a))) return rc;
  s->advances++;
  s->total_ticks += a.T;
  s->passes++;
  // what was in flight before this advance has finished on the device by now, or finishes while the host is busy here
  return tick_sync(s, ctx->timers.timing || !s->pipelined ? s->advances : s->advances - 1);
}

extern "C" {

int dsm_stream_sync(dsm_stream *s) {
  if (!s) return invalid("null stream");
  if (s->engine != 1 || !s->tick_ready) return DSM_OK;
  DSM_HIP(hipSetDevice(s->ctx->device));
  return tick_sync(s);
}

int dsm_stream_set_pipelined(dsm_stream *s, int on) {
  if (!s) return invalid("null stream");
  const int rc = dsm_stream_sync(s);
  if (rc) return rc;
  s->pipelined = on != 0;
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
    if (resident == 0 && waiting == 0 && s->groups.empty()) { // (a group's next tries are queued when the try before them is read back)
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
