// stream_pass.hip -- the PASS engine of a dsm_stream (engine 0; the two engines are set side by side in stream_capi.hip's header).
// Owns dsm_stream::pass (the slots' host states and the learnt schedule) and works on the slot arrays both engines share.
//
// One pass.  (i) waiting problems are admitted into free slots, (ii) their state machines are started, (iii) every level
// from the coarsest a resident problem stands on down to level 0 gets its rounds -- compact launches over the slots that
// can be at that level in this pass: the new ones and the carried ones standing at or above it -- (iv) the states are read
// back once; problems that terminated retire (dsm_stream_results), the others are carried.
#include <algorithm>

#include "stream_internal.hpp"

using namespace dsm;

namespace {

constexpr size_t kHistCap = 4096; // retired problems whose round counts the schedule looks at

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

} // namespace

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
      for (int i = segs[si].i0; i < segs[si].i1; i++) live[si] += s->pass.slots[i].state != SLOT_FREE;
    }
    while (!wq.empty()) {
      int best = -1;
      for (int si = sg0; si < sg1; si++)
        if (live[si] < segs[si].i1 - segs[si].i0 && (best < 0 || live[si] < live[best])) best = si;
      if (best < 0) break; // every slot of this kind is taken
      int &c = cursor[best];
      while (s->pass.slots[c].state != SLOT_FREE) c++;
      const Waiting &wt = wq.front();
      Slot &sl = s->pass.slots[c];
      sl = Slot();
      sl.state = SLOT_NEW;
      sl.ticket = wt.ticket;
      sl.trk = wt.trk;
      sl.lvl = wt.start.coarsest;
      s->arr.h_start[c] = wt.start;
      s->arr.h_tracker_ptrs[c] = wt.trk->d_desc;
      s->arr.h_rowmap[(size_t)DSM_MAX_LEVELS * N + (mode == 0 ? 0 : cap0) + p.n_new[mode]] = c - (mode == 0 ? 0 : cap0);
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
    const Slot &sl = s->pass.slots[i];
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
      const Slot &sl = s->pass.slots[i];
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
        if (s->pass.slots[i].state != SLOT_FREE && s->pass.slots[i].lvl >= L) s->arr.h_rowmap[(size_t)L * N + sg.i0 + r++] = i - sg.i0;
      sg.rows[L] = r;
    }
  }
  DSM_HIP(hipMemcpyAsync(s->arr.d_rowmap, s->arr.h_rowmap, sizeof(int) * (size_t)(DSM_MAX_LEVELS + 1) * N, hipMemcpyHostToDevice, s->ctx->stream));
  return DSM_OK;
}

// (ii) start the admitted problems (LM_OP_START over the list of new slots of each kind)
static int pass_start_admitted(dsm_stream *s, const Pass &p) {
  dsm_context *ctx = s->ctx;
  const int N = s->N;
  if (p.n_new[0] + p.n_new[1] == 0) return DSM_OK;
  DSM_HIP(hipMemcpyAsync(s->arr.d_tracker_ptrs, s->arr.h_tracker_ptrs, sizeof(TrackerDev *) * N, hipMemcpyHostToDevice, ctx->stream));
  DSM_HIP(hipMemcpyAsync(s->arr.d_start, s->arr.h_start, sizeof(StartInfo) * N, hipMemcpyHostToDevice, ctx->stream));
  for (int mode = 0; mode < 2; mode++) {
    if (!p.n_new[mode]) continue;
    const int base = mode == 0 ? 0 : s->cap[0];
    launch_lm(ctx->stream, mode, LM_OP_START, 0, p.n_new[mode], s->arr.d_tracker_ptrs + base, s->arr.d_states + base,
              s->arr.d_partials + (size_t)base * s->arr.partial_stride, s->arr.partial_stride, s->arr.d_start + base, nullptr, s->arr.d_status + 2 * base, false,
              s->arr.d_rowmap + (size_t)DSM_MAX_LEVELS * N + base);
  }
  return DSM_OK;
}

// (iii) the pass: the other segments' streams start behind the uploads and the START launches
static int pass_rounds(dsm_stream *s, Pass &p) {
  dsm_context *ctx = s->ctx;
  const LMBuffers B = s->arr.lm_buffers();
  int rc = fork_segments(ctx, p.segs);
  if (rc) return rc;
  for (int L = p.top > p.top2 ? p.top : p.top2; L >= 0; L--) {
    auto seg_rounds = [&](const Seg &sg) {
      int r = s->pass.fixed_rounds[sg.mode][L] > 0 ? s->pass.fixed_rounds[sg.mode][L] : p.draining ? s->pass.rounds_max[sg.mode][L] : s->pass.rounds[sg.mode][L];
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
        if ((rc = launch_round(ctx, B, *p.P, sg, L, k, s->arr.d_rowmap + (size_t)L * s->N + sg.i0, R, p.tm))) return rc;
      }
    for (const Seg &sg : p.segs)
      if (sg.rows[L] > 0) s->stats[sg.mode].launches[L] += seg_rounds(sg);
  }
  DSM_HIP(hipGetLastError());
  return join_segments(ctx, p.segs);
}

// a resident problem has terminated: its result, its rounds into the schedule's history, its slot free
static int pass_retire(dsm_stream *s, Slot &sl, const LMState &S, int mode) {
  dsm_stream_result r;
  const auto og = origin_of(s, sl.ticket);
  if (og == s->origin.end()) return DSM_ERR_STATE;
  fill_stream_result(r, S, mode, sl.ticket, sl.passes, og->second.pose0, og->second.aff0);
  s->origin.erase(og);
  route_result(s, r);
  s->retired[mode]++;
  for (int l = 0; l < s->nlevels; l++) {
    std::vector<int> &hv = s->pass.hist[mode][l];
    if (hv.size() < kHistCap)
      hv.push_back((int)S.rounds[l]);
    else
      hv[s->pass.hist_pos[mode] % kHistCap] = (int)S.rounds[l];
  }
  s->pass.hist_pos[mode]++;
  sl = Slot();
  return DSM_OK;
}

// (iv) one read-back; what THIS pass evaluated goes into the statistics; terminated problems retire, the others are carried
static int pass_read_back(dsm_stream *s, Pass &p) {
  dsm_context *ctx = s->ctx;
  const int N = s->N, nlevels = s->nlevels;
  DSM_HIP(hipMemcpyAsync(s->arr.h_states, s->arr.d_states, sizeof(LMState) * N, hipMemcpyDeviceToHost, ctx->stream));
  DSM_HIP(hipEventRecord(ctx->timers.ev_total[1], ctx->stream));
  DSM_HIP(hipStreamSynchronize(ctx->stream));
  s->advances_done++;
  float ms = 0;
  DSM_HIP(hipEventElapsedTime(&ms, ctx->timers.ev_total[0], ctx->timers.ev_total[1]));
  s->stats[0].total_ms += ms, s->stats[1].total_ms += ms;
  s->stats[0].polls += 1;
  if (ctx->timers.timing) collect_eval_timing(ctx, p.tm.lvl, nlevels, s->stats[0]);
  for (int i = 0; i < N; i++) {
    Slot &sl = s->pass.slots[i];
    if (sl.state == SLOT_FREE) continue;
    const int mode = i < s->cap[0] ? 0 : 1;
    const LMState &S = s->arr.h_states[i];
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
      if (pass_retire(s, sl, S, mode)) return DSM_ERR_STATE;
      continue;
    }
    if (sl.passes > 4096) {
      set_error("internal: a resident problem did not terminate within 4096 passes");
      return DSM_ERR_STATE;
    }
    sl.state = SLOT_RUNNING;
    sl.lvl = S.lvl;
    s->pass.carried_slot_passes++;
  }
  return DSM_OK;
}

// the next pass's rounds per level: the quantile of what the recently retired problems needed
static void pass_learn(dsm_stream *s) {
  for (int mode = 0; mode < 2; mode++) {
    if (s->pass.hist[mode][0].size() < 16) continue;
    std::vector<int> r;
    for (int l = 0; l < s->nlevels; l++) {
      r = s->pass.hist[mode][l];
      size_t k = (size_t)(s->pass.quantile[l] * (double)(r.size() - 1) + 0.5);
      if (k >= r.size()) k = r.size() - 1;
      std::nth_element(r.begin(), r.begin() + k, r.end());
      s->pass.rounds[mode][l] = r[k] < 1 ? 1 : r[k];
      s->pass.rounds_max[mode][l] = *std::max_element(r.begin(), r.end()) + 1;
    }
  }
}

int dsm::pass_resident(const dsm_stream *s) {
  int r = 0;
  for (const Slot &sl : s->pass.slots) r += sl.state != SLOT_FREE;
  return r;
}

int dsm::pass_advance(dsm_stream *s) {
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
