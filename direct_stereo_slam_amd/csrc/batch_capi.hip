// batch_capi.hip -- the batch form of the LM scheduler (run_lm_batch: work queue, chain prefix, passes; what it shares with the
// streaming form is lm_schedule.hip's) and its entry points, dsm_track* and dsm_optimize_scale*.
#include <algorithm>
#include <cstring>
#include <vector>

#include "dsm_internal.hpp"

namespace dsm {

static int ensure_batch_capacity(dsm_context *ctx, int nprob, int partial_stride) {
  if (nprob <= ctx->lm.cap_prob && partial_stride <= ctx->lm.partial_stride) return DSM_OK;
  const int cap = nprob > ctx->lm.cap_prob ? nprob : ctx->lm.cap_prob;
  const int ps = partial_stride > ctx->lm.partial_stride ? partial_stride : ctx->lm.partial_stride;
  int rc;
  if ((rc = realloc_dev(&ctx->lm.d_tracker_ptrs, cap))) return rc;
  if ((rc = realloc_pinned(&ctx->lm.h_tracker_ptrs, cap))) return rc;
  if ((rc = realloc_dev(&ctx->lm.d_states, cap))) return rc;
  if ((rc = realloc_pinned(&ctx->lm.h_states, cap))) return rc;
  if ((rc = realloc_dev(&ctx->lm.d_partials, (size_t)cap * ps))) return rc;
  if ((rc = realloc_dev(&ctx->lm.d_start, cap))) return rc;
  if ((rc = realloc_pinned(&ctx->lm.h_start, cap))) return rc;
  if ((rc = realloc_dev(&ctx->lm.d_single, cap))) return rc;
  if ((rc = realloc_pinned(&ctx->lm.h_single, cap))) return rc;
  if ((rc = realloc_dev(&ctx->lm.d_status, 2 * (size_t)cap))) return rc;
  if ((rc = realloc_pinned(&ctx->lm.h_status, 2 * (size_t)cap))) return rc;
  if ((rc = realloc_dev(&ctx->lm.d_rowmap, cap))) return rc;
  if ((rc = realloc_pinned(&ctx->lm.h_rowmap, cap))) return rc;
  if ((rc = realloc_dev(&ctx->lm.d_tickets, cap))) return rc;
  DSM_HIP(hipMemsetAsync(ctx->lm.d_tickets, 0, sizeof(int) * cap, ctx->stream));
  DSM_HIP(hipMemsetAsync(ctx->lm.d_states, 0, sizeof(LMState) * cap, ctx->stream));
  ctx->lm.cap_prob = cap;
  ctx->lm.partial_stride = ps;
  return DSM_OK;
}

int round8(int x) { return (x + 7) & ~7; }

// ts: n trackers of a call in mode `mode`, followed by n2 trackers of the companion segment in mode `mode2`
int prepare_batch(dsm_context *ctx, int n, dsm_tracker *const *ts, int mode, int n2, int mode2) {
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
  for (int i = 0; i < n + n2; i++) ctx->lm.h_tracker_ptrs[i] = ts[i]->d_desc;
  DSM_HIP(hipMemcpyAsync(ctx->lm.d_tracker_ptrs, ctx->lm.h_tracker_ptrs, sizeof(TrackerDev *) * (n + n2), hipMemcpyHostToDevice, ctx->stream));
  return DSM_OK;
}

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
  if (qcap > ctx->lm.qcap) {
    ctx->lm.qcap = 0;
    const int rc = realloc_dev(&ctx->lm.d_qitems, qcap);
    if (rc) return rc;
    ctx->lm.qcap = qcap;
  }
  if (!ctx->lm.d_queue) DSM_HIP(hipMalloc(&ctx->lm.d_queue, sizeof(WorkQueue)));
  if (!ctx->lm.h_queue) DSM_HIP(hipHostMalloc(&ctx->lm.h_queue, sizeof(WorkQueue), hipHostMallocDefault));
  DSM_HIP(hipMemsetAsync(ctx->lm.d_queue, 0, sizeof(WorkQueue), ctx->stream));
  DSM_HIP(hipMemsetAsync(ctx->lm.d_qitems, 0, ctx->lm.qcap * sizeof(unsigned long long), ctx->stream)); // stale publication tags
  if (ctx->lm.queue_blocks[mode] == 0) {
    hipDeviceProp_t prop;
    DSM_HIP(hipGetDeviceProperties(&prop, ctx->device));
    const int per_cu = queue_kernel_blocks_per_cu(mode);
    if (per_cu < 1) return invalid("work queue: kernel does not fit the device");
    ctx->lm.queue_blocks[mode] = per_cu * prop.multiProcessorCount; // all workgroups must be co-resident
  }
  hipEvent_t qa = ctx->timers.timing ? get_event(ctx, 0) : nullptr, qb = ctx->timers.timing ? get_event(ctx, 1) : nullptr;
  if (qa) DSM_HIP(hipEventRecord(qa, ctx->stream));
  launch_queue(ctx->stream, mode, ctx->lm.queue_blocks[mode], n, ctx->lm.d_tracker_ptrs, ctx->lm.d_states, ctx->lm.d_partials,
               ctx->lm.partial_stride, ctx->lm.d_tickets, ctx->lm.d_queue, ctx->lm.d_qitems, (unsigned)(ctx->lm.qcap - 1));
  if (qb) DSM_HIP(hipEventRecord(qb, ctx->stream));
  DSM_HIP(hipGetLastError());
  DSM_HIP(hipMemcpyAsync(ctx->lm.h_queue, ctx->lm.d_queue, sizeof(WorkQueue), hipMemcpyDeviceToHost, ctx->stream));
  ctx->timers.stats.queue_blocks = ctx->lm.queue_blocks[mode];
  return DSM_OK;
}
// after the call's read-back: the queue kernel's verdict and statistics
static int queue_outcome(dsm_context *ctx) {
  if (ctx->lm.h_queue->error) {
    // leave the arrival counters clean for the next call
    DSM_HIP(hipMemsetAsync(ctx->lm.d_tickets, 0, sizeof(int) * ctx->lm.cap_prob, ctx->stream));
    DSM_HIP(hipStreamSynchronize(ctx->stream));
    set_error("internal: work-queue kernel gave up waiting (bounded wait expired)");
    return DSM_ERR_STATE;
  }
  ctx->timers.stats.queue_items = ctx->lm.h_queue->tail;
  if (ctx->timers.timing && ctx->timers.ev_pool.size() >= 2) {
    float qm = 0;
    if (hipEventElapsedTime(&qm, ctx->timers.ev_pool[0], ctx->timers.ev_pool[1]) == hipSuccess) ctx->timers.stats.queue_kernel_ms = qm;
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
  for (const Seg &sg : segs) launch_chain(sg.st, sg.mode, sg.i1 - sg.i0, ctx->lm.d_tracker_ptrs + sg.i0, ctx->lm.d_states + sg.i0, ctx->lm.d_status + 2 * sg.i0);
  ctx->timers.stats.coarse_launches = 1;
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
    int groups = ctx->groups.n_streams < 1 ? 1 : ctx->groups.n_streams;
    if (groups > N) groups = N;
    run.shape[L] = RoundShape{max_chunks < 8 ? max_chunks : round8(max_chunks), max_n, (long long)((N + groups - 1) / groups) * max_n, 0, false};
  }
}

// one (evaluate, step) round of a segment at level L: the fused step for segments of few problems and for compact launches
static int batch_round(PassRun &run, const Seg &sg, int L, int k) {
  RoundShape R = run.shape[L];
  R.fuse_count = sg.i1 - sg.i0;
  R.fuse_also = sg.rows[L] >= 0;
  return launch_round(run.ctx, run.B, run.P, sg, L, k, run.ctx->lm.d_rowmap + sg.i0, R, run.tm);
}

// row map of a segment: the problems (relative to its first) for which `keep(status, level)` holds, from h_status
template <typename Keep>
static int build_rowmap(dsm_context *ctx, const Seg &sg, Keep keep, int *rows) {
  int r = 0;
  for (int i = sg.i0; i < sg.i1; i++)
    if (keep(ctx->lm.h_status[2 * i], ctx->lm.h_status[2 * i + 1])) ctx->lm.h_rowmap[sg.i0 + r++] = i - sg.i0;
  *rows = r;
  if (r > 0) DSM_HIP(hipMemcpyAsync(ctx->lm.d_rowmap + sg.i0, ctx->lm.h_rowmap + sg.i0, sizeof(int) * r, hipMemcpyHostToDevice, sg.st));
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
    const int st = seg_steps(sg), bk = ctx->learnt.sched_bulk[sg.companion ? run.mode2 : run.mode][L];
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
      DSM_HIP(hipMemcpyAsync(ctx->lm.h_status + 2 * sg.i0, ctx->lm.d_status + 2 * sg.i0, sizeof(int) * 2 * (sg.i1 - sg.i0), hipMemcpyDeviceToHost, sg.st));
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
  ctx->timers.stats.polls++;
  return DSM_OK;
}

// top / top2: the first level of the main / companion segment (-1: nothing to run)
static int run_passes(PassRun &run, dsm_tracker *const *ts, int n, int n2, int top, int top2) {
  dsm_context *ctx = run.ctx;
  const dsm_params &P = run.P;
  const int N = n + n2;
  plan_levels(run, ts, N, ts[0]->nlevels);
  const int *sched = ctx->learnt.sched[run.mode], *sched2 = ctx->learnt.sched[run.mode2];
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
      ctx->timers.stats.launches[L] += steps;
      ctx->timers.stats2.launches[L] += steps2;
    }
    DSM_HIP(hipGetLastError()); // launch-configuration errors of the kernels enqueued above
    if ((rc = join_segments(ctx, run.segs, top2 >= 0))) return rc;
    DSM_HIP(hipMemcpyAsync(ctx->lm.h_status, ctx->lm.d_status, sizeof(int) * 2 * N, hipMemcpyDeviceToHost, ctx->stream));
    DSM_HIP(hipStreamSynchronize(ctx->stream));
    ctx->timers.stats.polls++;
    top = top2 = -1;
    for (int i = 0; i < n; i++)
      if (ctx->lm.h_status[2 * i] == ST_RUNNING && ctx->lm.h_status[2 * i + 1] > top) top = ctx->lm.h_status[2 * i + 1];
    for (int i = n; i < N; i++)
      if (ctx->lm.h_status[2 * i] == ST_RUNNING && ctx->lm.h_status[2 * i + 1] > top2) top2 = ctx->lm.h_status[2 * i + 1];
    if (top < 0 && top2 < 0) break;
    if (pass > 64) {
      set_error("internal: LM state machine did not terminate within the launch bound");
      return DSM_ERR_STATE;
    }
  }
  return DSM_OK;
}

// after the call's read-back: every problem must have terminated; the statistics of the call (ctx->timers.stats, the companion's ctx->timers.stats2)
// and the schedule the next call starts from
static int account_and_learn(dsm_context *ctx, dsm_tracker *const *ts, int n, int n2, int mode, int mode2) {
  const int nlevels = ts[0]->nlevels;
  const int N = n + n2;
  int *sched = ctx->learnt.sched[mode], *sched2 = ctx->learnt.sched[mode2];
  int need[DSM_MAX_LEVELS] = {0}, need2[DSM_MAX_LEVELS] = {0};
  for (int i = 0; i < N; i++) {
    const LMState &S = ctx->lm.h_states[i];
    if (S.status == ST_RUNNING) {
      set_error("internal: LM state machine did not terminate within the launch bound");
      return DSM_ERR_STATE;
    }
    dsm_stats &st = i < n ? ctx->timers.stats : ctx->timers.stats2;
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
    int *dst = ctx->learnt.sched_bulk[seg ? mode2 : mode];
    for (int l = 0; l < nlevels; l++) {
      r.clear();
      for (int i = i0; i < i1; i++) r.push_back((int)ctx->lm.h_states[i].rounds[l]);
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
// them.  Launch-per-step form only.  Statistics of the companion: ctx->timers.stats2.
int run_lm_batch(dsm_context *ctx, int n, dsm_tracker *const *ts, int mode, int coarsest, int n2, int mode2) {
  const int nlevels = ts[0]->nlevels;
  if (coarsest < 0 || coarsest >= nlevels) return invalid("coarsest level out of range"); // :457 / :856
  const dsm_params &P = ts[0]->params;
  const int N = n + n2;
  memset(&ctx->timers.stats, 0, sizeof ctx->timers.stats);
  memset(&ctx->timers.stats2, 0, sizeof ctx->timers.stats2);
  DSM_HIP(hipEventRecord(ctx->timers.ev_total[0], ctx->stream));
  DSM_HIP(hipMemcpyAsync(ctx->lm.d_start, ctx->lm.h_start, sizeof(StartInfo) * N, hipMemcpyHostToDevice, ctx->stream));
  launch_lm(ctx->stream, mode, LM_OP_START, coarsest, n, ctx->lm.d_tracker_ptrs, ctx->lm.d_states, ctx->lm.d_partials,
            ctx->lm.partial_stride, ctx->lm.d_start, nullptr, ctx->lm.d_status);
  if (n2 > 0)
    launch_lm(ctx->stream, mode2, LM_OP_START, coarsest, n2, ctx->lm.d_tracker_ptrs + n, ctx->lm.d_states + n,
              ctx->lm.d_partials + (size_t)n * ctx->lm.partial_stride, ctx->lm.partial_stride, ctx->lm.d_start + n, nullptr, ctx->lm.d_status + 2 * n);
  const bool use_queue = queue_wanted(P, n, n2, ts);
  int rc;
  if (use_queue && (rc = run_queue(ctx, ts, n, mode, coarsest))) return rc;
  // the learnt "rounds most problems need" belong to calls of this size and form: another batch-size bucket (powers of four)
  // or form must not inherit them (a batch of hundreds following a single-frame call would switch to compact launches after
  // one round, covering almost every problem)
  int bucket = 0;
  for (int v = N; v >= 4; v >>= 2) bucket++;
  const int key = bucket * 4 + (use_queue ? 2 : 0) + (P.persistent_coarse < 0 ? 1 : 0);
  if (key != ctx->learnt.sched_bulk_key) {
    for (int m = 0; m < 3; m++)
      for (int l = 0; l < DSM_MAX_LEVELS; l++) ctx->learnt.sched_bulk[m][l] = 1 << 30;
    ctx->learnt.sched_bulk_key = key;
  }
  std::vector<Seg> segs = build_segments(ctx->groups.n_streams, n, mode, n2, mode2);
  if ((rc = bind_streams(ctx, segs))) return rc;
  PassRun run{ctx, P, segs, mode, mode2,
              LMBuffers{ctx->lm.d_tracker_ptrs, ctx->lm.d_states, ctx->lm.d_partials, ctx->lm.partial_stride, ctx->lm.d_tickets, ctx->lm.d_status}, EvalTimer{}, {}, {}};
  if (!use_queue) {
    int top = coarsest, top2 = n2 > 0 ? coarsest : -1;
    rc = P.persistent_coarse < 0 ? run_chain_prefix(ctx, ts, n, n2, segs, coarsest, top, top2) : DSM_OK;
    if (!rc) rc = run_passes(run, ts, n, n2, top, top2);
    if (rc) return rc;
  }
  DSM_HIP(hipMemcpyAsync(ctx->lm.h_states, ctx->lm.d_states, sizeof(LMState) * N, hipMemcpyDeviceToHost, ctx->stream));
  DSM_HIP(hipEventRecord(ctx->timers.ev_total[1], ctx->stream));
  DSM_HIP(hipStreamSynchronize(ctx->stream));
  if (use_queue && (rc = queue_outcome(ctx))) return rc;
  float ms = 0;
  DSM_HIP(hipEventElapsedTime(&ms, ctx->timers.ev_total[0], ctx->timers.ev_total[1]));
  ctx->timers.stats.total_ms = ms;
  ctx->timers.stats2.total_ms = ms;
  if (ctx->timers.timing) collect_eval_timing(ctx, run.tm.lvl, nlevels, ctx->timers.stats);
  return account_and_learn(ctx, ts, n, n2, mode, mode2);
}

} // namespace dsm

using namespace dsm;

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
  fill_track_starts(ctx->lm.h_start, n, pose_io, aff_io, min_res_for_abort, coarsest_lvl);
  rc = run_lm_batch(ctx, n, ts, 0, coarsest_lvl);
  if (rc) return rc;
  read_track_batch(ctx->lm.h_states, n, pose_io, aff_io, last_residuals, flow_out, good);
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
  fill_scale_starts(ctx->lm.h_start, n, scale_io, coarsest_lvl);
  rc = run_lm_batch(ctx, n, ts, 1, coarsest_lvl);
  if (rc) return rc;
  read_scale_batch(ctx->lm.h_states, n, scale_io, err_out);
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
  fill_track_starts(ctx->lm.h_start, n, pose_io, aff_io, min_res_for_abort, coarsest_lvl);
  fill_scale_starts(ctx->lm.h_start + n, n_scale, scale_io, coarsest_lvl);
  rc = run_lm_batch(ctx, n, all.data(), 0, coarsest_lvl, n_scale, 1);
  if (rc) return rc;
  read_track_batch(ctx->lm.h_states, n, pose_io, aff_io, last_residuals, flow_out, good);
  read_scale_batch(ctx->lm.h_states + n, n_scale, scale_io, err_out);
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

} // extern "C"
