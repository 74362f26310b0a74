// stream_tick.hip -- the TICK engine of a dsm_stream (engine 1, the default; the two engines are set side by side in stream_capi.hip's
// header).  Owns dsm_stream::tick -- everything tick_setup allocates, the rings' counters and the state of the advances in flight -- and
// works on the slot arrays both engines share.
#include <algorithm>
#include <cmath>

#include "stream_internal.hpp"

using namespace dsm;

void dsm_stream::TickEngine::release() {
  release_dev(d_segctl), release_pinned(h_segctl), release_dev(d_modectl), release_pinned(h_modectl);
  for (unsigned *&p : d_items) release_dev(p);
  d_items.clear();
  for (int m = 0; m < 2; m++) release_dev(d_pending[m]), release_pinned(h_pending[m]), release_dev(d_results[m]), release_pinned(h_results[m]);
  release_dev(d_slot_ticket), release_dev(d_admit_idx), release_pinned(h_count_word);
  for (int k = 0; k < 2; k++) {
    if (ev_begin[k]) hipEventDestroy(ev_begin[k]);
    if (ev_end[k]) hipEventDestroy(ev_end[k]);
    ev_begin[k] = ev_end[k] = nullptr;
  }
  ready = false;
}

static int tick_setup(dsm_stream *s) {
  dsm_context *ctx = s->ctx;
  const int cap0 = s->cap[0], N = s->N;
  s->tick.segs = build_segments(ctx->groups.n_streams, cap0, 0, s->cap[1], 1);
  const int nseg = (int)s->tick.segs.size();
  s->tick.release(); // (an earlier attempt that failed half way left its allocations behind: ADVICE r04)
  int rc = realloc_dev(&s->tick.d_segctl, nseg);
  if (!rc) rc = realloc_pinned(&s->tick.h_segctl, 2 * (size_t)nseg);
  if (!rc) rc = realloc_dev(&s->tick.d_modectl, 2);
  if (!rc) rc = realloc_pinned(&s->tick.h_modectl, 2 * 2);
  if (!rc) rc = realloc_pinned(&s->tick.h_count_word, 4);
  if (!rc) rc = realloc_dev(&s->tick.d_slot_ticket, N);
  if (!rc) rc = realloc_dev(&s->tick.d_admit_idx, N);
  if (rc) return rc;
  // an item list holds at most one evaluation (+ its speculative twin) per slot of the segment
  const int maxpos = 8 * ((max_chunks_upto(s->w * s->h) + 7) / 8);
  if (maxpos >= (1 << kTickChunkBits)) return invalid("dsm_stream (tick engine): a level has too many chunks for the item encoding");
  if (N >= (1 << (30 - kTickChunkBits))) return invalid("dsm_stream (tick engine): too many slots for the item encoding");
  s->tick.d_items.assign(2 * nseg, nullptr);
  s->tick.items_cap.assign(nseg, 0);
  s->tick.last_count.assign(nseg, 0);
  s->tick.last_chain.assign(nseg, 0);
  for (int si = 0; si < nseg; si++) {
    const int ns = s->tick.segs[si].i1 - s->tick.segs[si].i0;
    const int cap = ns * 2 * maxpos + 64;
    s->tick.items_cap[si] = cap;
    for (int b = 0; b < 2; b++) // item slots [0, cap), then one chain entry per slot of the segment
      if ((rc = realloc_dev(&s->tick.d_items[2 * si + b], (size_t)cap + ns))) return rc;
  }
  DSM_HIP(hipMemsetAsync(s->tick.d_segctl, 0, sizeof(TickSegCtl) * nseg, ctx->stream));
  DSM_HIP(hipMemsetAsync(s->tick.d_slot_ticket, 0, sizeof(unsigned long long) * N, ctx->stream));
  // the waiting ring and the result ring of each kind: the host appends waiting problems and never lets more in than the result
  // ring has room for; the device consumes / produces by monotonic counters
  for (int mode = 0; mode < 2; mode++) {
    int ring = 1024;
    while (ring < 4 * s->cap[mode]) ring <<= 1;
    s->tick.ring[mode] = ring;
    if ((rc = realloc_dev(&s->tick.d_pending[mode], ring)) || (rc = realloc_pinned(&s->tick.h_pending[mode], ring)) ||
        (rc = realloc_dev(&s->tick.d_results[mode], ring)) || (rc = realloc_pinned(&s->tick.h_results[mode], 2 * (size_t)ring)))
      return rc;
    TickModeCtl mc;
    memset(&mc, 0, sizeof mc);
    mc.ring = ring;
    s->tick.h_modectl[mode] = mc;
  }
  DSM_HIP(hipMemcpyAsync(s->tick.d_modectl, s->tick.h_modectl, sizeof(TickModeCtl) * 2, hipMemcpyHostToDevice, ctx->stream));
  for (int k = 0; k < 2; k++) {
    DSM_HIP(hipEventCreate(&s->tick.ev_begin[k]));
    DSM_HIP(hipEventCreate(&s->tick.ev_end[k]));
  }
  DSM_HIP(hipStreamSynchronize(ctx->stream));
  memset(s->tick.seen, 0, sizeof s->tick.seen);
  s->tick.ready = true;
  return DSM_OK;
}

// the read-back of advance `k` (parity k & 1): control blocks and result rings are in the pinned copies once ev_end[k & 1] is reached
static int tick_collect(dsm_stream *s, long long k) {
  dsm_context *ctx = s->ctx;
  const int par = (int)(k & 1), nseg = (int)s->tick.segs.size();
  DSM_HIP(hipEventSynchronize(s->tick.ev_end[par]));
  float ms = 0;
  DSM_HIP(hipEventElapsedTime(&ms, s->tick.ev_begin[par], s->tick.ev_end[par]));
  s->stats[0].total_ms += ms, s->stats[1].total_ms += ms; // (the stream's statistics are cumulative)
  s->stats[0].polls += 1;
  if (s->tick.inflight_timed[par]) collect_eval_timing(ctx, s->tick.tm.lvl, 1, s->stats[0]);
  for (int si = 0; si < nseg; si++) {
    const TickSegCtl &sc = s->tick.h_segctl[par * nseg + si];
    if (sc.overflow) {
      set_error("internal: an item list of the tick engine ran over");
      return DSM_ERR_STATE;
    }
    s->tick.last_count[si] = sc.count[s->tick.inflight_parity[par]];
    s->tick.last_chain[si] = sc.chain[s->tick.inflight_parity[par]];
  }
  for (int mode = 0; mode < 2; mode++) {
    const TickModeCtl &mc = s->tick.h_modectl[par * 2 + mode];
    dsm_stream::TickEngine::Seen &sn = s->tick.seen[mode];
    const int ring = s->tick.ring[mode];
    const long long new_ret = mc.retired - sn.retired;
    if (new_ret < 0 || new_ret > ring) {
      set_error("internal: the tick engine's result ring ran over");
      return DSM_ERR_STATE;
    }
    dsm_stats &st = s->stats[mode];
    for (int l = 0; l < s->nlevels; l++) st.launches[l] += s->tick.inflight_ticks[par];
    const TickResult *res = s->tick.h_results[mode] + (size_t)par * ring;
    long long life_sum = 0;
    for (long long i = 0; i < new_ret; i++) {
      const TickResult &R = res[(sn.retired + i) & (ring - 1)];
      life_sum += R.ticks; // (= its LM rounds, less the rounds chains ran inside one tick)
      auto it = origin_of(s, R.ticket);
      if (it == s->origin.end()) return DSM_ERR_STATE;
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
      s->tick.life_ticks = s->tick.life_ticks > 0.0 ? 0.75 * s->tick.life_ticks + 0.25 * mean : mean;
    }
    sn.retired = mc.retired;
    sn.admitted = mc.pending_head;
    s->tick.resident[mode] = (int)(sn.admitted - sn.retired);
  }
  return DSM_OK;
}

int dsm::tick_sync(dsm_stream *s, long long upto) {
  while (s->tick.collected < (upto < 0 ? s->tick.advances : upto)) {
    const int rc = tick_collect(s, s->tick.collected);
    if (rc) return rc;
    s->tick.collected++;
  }
  return DSM_OK;
}

int dsm::tick_resident(const dsm_stream *s) {
  return (int)((s->tick.seen[0].admitted - s->tick.seen[0].retired) + (s->tick.seen[1].admitted - s->tick.seen[1].retired));
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
    const int ring = s->tick.ring[mode];
    // room in BOTH rings of this kind, each of `ring` entries: the waiting ring holds what is handed over and not admitted, the result ring
    // must take everything handed over and not yet read back as retired (its two pinned copies are read one advance late)
    const long long room = std::min<long long>(ring - (s->tick.handed[mode] - s->tick.seen[mode].admitted), ring - (s->tick.handed[mode] - s->tick.seen[mode].retired));
    const int n = (int)std::min<long long>((long long)s->waiting[mode].size(), room > 0 ? room : 0);
    a.n_new[mode] = n;
    for (int i = 0; i < n; i++) {
      const Waiting &wt = s->waiting[mode].front();
      TickPending &pd = s->tick.h_pending[mode][(s->tick.handed[mode] + i) & (ring - 1)];
      pd.start = wt.start;
      pd.trk = wt.trk->d_desc;
      pd.ticket = wt.ticket;
      fresh.push_back(wt.trk);
      s->tick.sched_fixed_schedule = wt.trk->params.fixed_schedule, s->tick.sched_speculate = wt.trk->params.speculate, s->tick.have_sched = true;
      auto it = s->origin.find(wt.ticket);
      if (it != s->origin.end()) it->second.admitted_at = a.k;
      s->waiting[mode].pop_front();
    }
  }
  if (!s->tick.have_sched) return invalid("dsm_stream: internal: no problem was ever handed over");
  int rc;
  if (!fresh.empty() && (rc = sync_descs(ctx, fresh.data(), (int)fresh.size()))) return rc;
  DSM_HIP(hipEventRecord(s->tick.ev_begin[a.par], ctx->stream));
  if (ctx->timers.timing) DSM_HIP(hipEventRecord(ctx->timers.ev_total[0], ctx->stream)); // (collect_eval_timing places the dispatches relative to it)
  for (int mode = 0; mode < 2; mode++) {
    if (!a.n_new[mode]) continue;
    const int ring = s->tick.ring[mode];
    const int first = (int)(s->tick.handed[mode] & (ring - 1)), n1 = std::min(a.n_new[mode], ring - first);
    DSM_HIP(hipMemcpyAsync(s->tick.d_pending[mode] + first, s->tick.h_pending[mode] + first, sizeof(TickPending) * n1, hipMemcpyHostToDevice, ctx->stream));
    if (a.n_new[mode] > n1)
      DSM_HIP(hipMemcpyAsync(s->tick.d_pending[mode], s->tick.h_pending[mode], sizeof(TickPending) * (a.n_new[mode] - n1), hipMemcpyHostToDevice, ctx->stream));
    s->tick.handed[mode] += a.n_new[mode];
    s->tick.h_count_word[a.par * 2 + mode] = s->tick.handed[mode];
    DSM_HIP(hipMemcpyAsync(&s->tick.d_modectl[mode].pending_count, &s->tick.h_count_word[a.par * 2 + mode], sizeof(long long), hipMemcpyHostToDevice, ctx->stream));
  }
  for (int mode = 0; mode < 2; mode++) a.may_admit[mode] = s->tick.on_the_way(mode) > 0;
  return DSM_OK;
}

// the advance's ticks and the switches of its launches
static void tick_plan(dsm_stream *s, Advance &a) {
  a.T = s->tick.ticks;
  if (s->tick.auto_ticks && s->tick.life_ticks > 0.0) {
    const int m = s->cap[0] > 0 ? 0 : 1;
    // sized to retire 7/8 of what the advance hands over: the rest stays in the device's waiting ring as the buffer from which a slot
    // freed by a retirement is refilled on the spot (a caller that hands over a full pool every advance builds a backlog of an eighth of
    // a pool per advance; it is worked off at full occupancy when the caller stops).  Nothing handed over: the residents' own life.
    // (With dsm_params.fixed_schedule every problem lives the same number of ticks and a cohort admitted together stays on one level,
    // which evaluates in larger single-level launches: there an advance is one cohort's whole life.)
    const double share = s->tick.sched_fixed_schedule > 0 ? 1.0 : 0.875;
    const double t = a.n_new[m] > 0 ? share * (double)a.n_new[m] * s->tick.life_ticks / (double)s->cap[m] : s->tick.life_ticks;
    a.T = (int)std::ceil(t);
    a.T = a.T < 8 ? 8 : a.T > 256 ? 256 : a.T;
  }
  s->tick.inflight_ticks[a.par] = a.T;
  a.speculate = s->tick.sched_fixed_schedule > 0 ? 0 : s->tick.sched_speculate;
  // (with dsm_params.fixed_schedule a cohort moves in lock step and an advance is its whole life: chains would only unbalance it)
  a.chain_rounds = (s->tick.sched_fixed_schedule > 0 || !s->tick.chain_possible) ? 0 : s->tick.chain_rounds;
}

// the list of segment si that buffer `buf` of its items is
static TickList tick_list(const dsm_stream *s, int si, int buf, int chain_rounds) {
  const Seg &sg = s->tick.segs[si];
  return TickList{s->tick.d_items[2 * si + buf], s->tick.d_segctl + si, buf, s->tick.items_cap[si], chain_rounds > 0 ? sg.i1 - sg.i0 : 0, s->tick.chain_max_n0};
}

// which free slot takes which waiting problem (one launch, before the stream groups fork), then every segment's free slots take theirs
static int tick_reserve_and_admit(dsm_stream *s, const Advance &a) {
  dsm_context *ctx = s->ctx;
  const int nseg = (int)s->tick.segs.size();
  if (a.may_admit[0] || a.may_admit[1]) {
    TickReserveArgs ra;
    if (nseg > kTickMaxSegs) return invalid("dsm_stream: too many stream groups");
    ra.nseg = nseg;
    for (int si = 0; si < nseg; si++) ra.seg[si] = TickSegDesc{s->tick.segs[si].mode, s->tick.segs[si].i0, s->tick.segs[si].i1 - s->tick.segs[si].i0};
    launch_tick_reserve(ctx->stream, ra, s->arr.d_states, s->tick.d_modectl, s->tick.d_admit_idx);
  }
  const int rc = fork_segments(ctx, s->tick.segs);
  if (rc) return rc;
  for (int si = nseg - 1; si >= 0; si--) {
    const Seg &sg = s->tick.segs[si];
    const int i0 = sg.i0, ns = sg.i1 - sg.i0, mode = sg.mode;
    if (a.may_admit[mode]) // (free slots take what tick_reserve_kernel gave them)
      launch_tick_admit(sg.st, mode, ns, (const TrackerDev **)s->arr.d_tracker_ptrs + i0, s->arr.d_states + i0, tick_list(s, si, s->tick.parity, a.chain_rounds),
                        s->tick.d_modectl + mode, s->tick.d_pending[mode], s->tick.d_slot_ticket + i0, s->tick.d_admit_idx + i0);
  }
  return DSM_OK;
}

// T ticks: per segment one evaluation launch over its item list and one LM launch over its slots
static int tick_ticks(dsm_stream *s, const Advance &a) {
  dsm_context *ctx = s->ctx;
  const int nseg = (int)s->tick.segs.size();
  s->tick.tm.used = 0;
  s->tick.tm.lvl.clear();
  for (int t = 0; t < a.T; t++) {
    const int buf = (s->tick.parity + t) & 1;
    for (int si = nseg - 1; si >= 0; si--) {
      const Seg &sg = s->tick.segs[si];
      const int i0 = sg.i0, ns = sg.i1 - sg.i0, mode = sg.mode;
      // grid: what the segment's list held at the end of the last advance read back, plus slack (the kernel strides over a longer list)
      long long grid = (long long)(s->tick.last_count[si] + s->tick.last_chain[si]) * 5 / 4 + 256;
      if (s->tick.last_count[si] + s->tick.last_chain[si] == 0) grid = (long long)ns * 16;
      if (grid > s->tick.items_cap[si]) grid = s->tick.items_cap[si];
      float *part = s->arr.d_partials + (size_t)i0 * s->arr.partial_stride;
      hipEvent_t eb = nullptr;
      const int rc = timed_eval_begin(ctx, sg, 0, s->tick.tm, &eb); // (all levels in one launch: booked under index 0)
      if (rc) return rc;
      const TickList next = tick_list(s, si, buf ^ 1, a.chain_rounds);
      const TickChainArgs chain{(const TrackerDev **)s->arr.d_tracker_ptrs + i0, s->arr.d_states + i0, next, s->tick.d_modectl + mode, s->tick.d_pending[mode],
                                s->tick.d_results[mode], s->tick.d_slot_ticket + i0, a.chain_rounds, s->tick.chain_flags};
      launch_tick_eval(sg.st, mode, (int)grid, s->arr.d_states + i0, part, s->arr.partial_stride, tick_list(s, si, buf, a.chain_rounds), chain, s->tick.chain_possible);
      if (eb) DSM_HIP(hipEventRecord(eb, sg.st));
      launch_tick_lm(sg.st, mode, ns, (const TrackerDev **)s->arr.d_tracker_ptrs + i0, s->arr.d_states + i0, part, s->arr.partial_stride, next, s->tick.d_modectl + mode,
                     s->tick.d_pending[mode], s->tick.d_results[mode], s->tick.d_slot_ticket + i0, a.speculate, s->tick.lm_opts);
    }
  }
  s->tick.parity = (s->tick.parity + a.T) & 1;
  s->tick.inflight_parity[a.par] = s->tick.parity;
  s->tick.inflight_timed[a.par] = ctx->timers.timing;
  DSM_HIP(hipGetLastError());
  return DSM_OK;
}

// read-back behind the ticks: control blocks and the result rings, into this advance's pinned copies
static int tick_read_back(dsm_stream *s, const Advance &a) {
  dsm_context *ctx = s->ctx;
  const int nseg = (int)s->tick.segs.size(), par = a.par;
  const int rc = join_segments(ctx, s->tick.segs);
  if (rc) return rc;
  DSM_HIP(hipMemcpyAsync(s->tick.h_modectl + par * 2, s->tick.d_modectl, sizeof(TickModeCtl) * 2, hipMemcpyDeviceToHost, ctx->stream));
  DSM_HIP(hipMemcpyAsync(s->tick.h_segctl + par * nseg, s->tick.d_segctl, sizeof(TickSegCtl) * nseg, hipMemcpyDeviceToHost, ctx->stream));
  for (int mode = 0; mode < 2; mode++)
    if (s->tick.handed[mode] > s->tick.seen[mode].retired) // (results may appear)
      DSM_HIP(hipMemcpyAsync(s->tick.h_results[mode] + (size_t)par * s->tick.ring[mode], s->tick.d_results[mode], sizeof(TickResult) * s->tick.ring[mode],
                             hipMemcpyDeviceToHost, ctx->stream));
  DSM_HIP(hipEventRecord(s->tick.ev_end[par], ctx->stream));
  return DSM_OK;
}

int dsm::tick_advance(dsm_stream *s) {
  dsm_context *ctx = s->ctx;
  DSM_HIP(hipSetDevice(ctx->device));
  if (!s->arr.partial_stride) return DSM_OK; // nothing was ever submitted
  int rc;
  if (!s->tick.ready && (rc = tick_setup(s))) return rc;
  if (!s->tick.in_transit() && s->tick.resident[0] + s->tick.resident[1] == 0 && s->waiting[0].empty() && s->waiting[1].empty()) return DSM_OK; // idle
  if ((rc = bind_streams(ctx, s->tick.segs))) return rc;
  if ((s->tick.advances - s->tick.collected >= 2 || ctx->timers.timing) && (rc = tick_sync(s))) return rc; // (at most one advance behind: the pinned copies are two deep;
                                                                                                    // a timed advance reads its own events alone)
  Advance a{};
  a.k = s->tick.advances;
  a.par = a.k & 1;
  if ((rc = tick_hand_over(s, a))) return rc;
  tick_plan(s, a);
  if ((rc = tick_reserve_and_admit(s, a)) || (rc = tick_ticks(s, a)) || (rc = tick_read_back(s, a))) return rc;
  s->tick.advances++;
  s->tick.total_ticks += a.T;
  s->advances_done++;
  // what was in flight before this advance has finished on the device by now, or finishes while the host is busy here
  return tick_sync(s, ctx->timers.timing || !s->tick.pipelined ? s->tick.advances : s->tick.advances - 1);
}
