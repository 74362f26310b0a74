// stream_groups.hip -- hypothesis groups of a dsm_stream (dsm_stream_submit_hypotheses): FrontEnd::trackNewCoarse's list of tries as one
// submission.  Its tries are ordinary track problems without abort thresholds; their results go to the group (route_result, called by
// either engine for every retired problem) instead of `done`, and the loop is replayed on the host by dsm_hypotheses_resolve
// (host_capi.cpp).
//
// Host bookkeeping only: this file issues NO HIP call -- no launch, no copy, no allocation -- and no launch or copy of the engines changes,
// with or without groups.  Keep it that way.
#include <algorithm>
#include <cstring>

#include "stream_internal.hpp"

using namespace dsm;

static void group_queue_try(dsm_stream *s, uint64_t gt, HypGroup &g, int i) {
  const uint64_t tk = enqueue_track(s, g.trk, &g.tries[7 * (size_t)i], g.aff_last, g.coarsest, nullptr); // no abort: replayed by the resolver
  s->hyp.member[tk] = std::make_pair(gt, i);
  g.in_flight++;
}

// the group's tries that still wait on the host leave the queue (those on the device run to their end)
static void group_drop_waiting(dsm_stream *s, uint64_t gt, HypGroup &g) {
  std::deque<Waiting> &wq = s->waiting[0];
  auto keep_end = std::remove_if(wq.begin(), wq.end(), [&](const Waiting &w) {
    auto it = s->hyp.member.find(w.ticket);
    if (it == s->hyp.member.end() || it->second.first != gt) return false;
    s->hyp.member.erase(it);
    s->origin.erase(w.ticket);
    g.in_flight--;
    return true;
  });
  wq.erase(keep_end, wq.end());
}

void dsm::route_result(dsm_stream *s, const dsm_stream_result &r) {
  auto mit = s->hyp.member.empty() ? s->hyp.member.end() : s->hyp.member.find(r.ticket);
  if (mit == s->hyp.member.end()) {
    s->done.push_back(r);
    return;
  }
  const uint64_t gt = mit->second.first;
  const int i = mit->second.second;
  s->hyp.member.erase(mit);
  HypGroup &g = s->hyp.groups.at(gt);
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
      const int w = s->hyp.hyp_window > 0 ? s->hyp.hyp_window : g.n;
      while (g.next < g.n && g.in_flight < w) group_queue_try(s, gt, g, g.next++);
    }
  }
  if (g.decided && g.in_flight == 0) { // nothing of the group is on the device any more: its result is handed back
    g.res.ticket = gt;
    g.res.tries_run = g.run;
    g.res.advances = (int)(s->advances_done - g.born);
    s->hyp.hyp_done.push_back(g.res);
    s->hyp.groups.erase(gt);
  }
}

extern "C" {

int dsm_stream_submit_hypotheses(dsm_stream *s, dsm_tracker *tracker, int n_tries, const double *tries, const double aff_last[2], int coarsest_lvl,
                                 double last_coarse_rmse0, double retrack_threshold, uint64_t *ticket_out) {
  if (!s || !tracker || n_tries < 1 || !tries || !aff_last || !ticket_out)
    return invalid("dsm_stream_submit_hypotheses: null stream / tracker / tries / aff_last / ticket_out, or n_tries < 1");
  if (s->cap[0] == 0) return invalid("dsm_stream_submit_hypotheses: the stream has no track slots");
  int rc = submit_common(s, 0, 1, &tracker, coarsest_lvl);
  if (rc) return rc;
  const uint64_t gt = s->next_ticket++;
  HypGroup &g = s->hyp.groups[gt];
  g.trk = tracker, g.n = n_tries, g.coarsest = coarsest_lvl;
  g.aff_last[0] = aff_last[0], g.aff_last[1] = aff_last[1];
  g.rmse0 = last_coarse_rmse0, g.thr = retrack_threshold;
  g.tries.assign(tries, tries + 7 * (size_t)n_tries);
  g.pose.assign(7 * (size_t)n_tries, 0.0), g.aff.assign(2 * (size_t)n_tries, 0.0);
  g.last.assign(DSM_MAX_LEVELS * (size_t)n_tries, 0.0), g.flow.assign(3 * (size_t)n_tries, 0.0);
  g.good.assign(n_tries, 0), g.back.assign(n_tries, 0);
  g.born = s->advances_done;
  group_queue_try(s, gt, g, 0); // try 0 (the constant-motion guess): nothing achieved yet, so no abort threshold either
  *ticket_out = gt;
  return DSM_OK;
}

int dsm_stream_hypotheses_results(dsm_stream *s, int max_results, dsm_stream_hyp_result *out, int *n_out) {
  if (!s || max_results < 0 || (max_results && !out) || !n_out) return invalid("dsm_stream_hypotheses_results: bad argument");
  *n_out = pop_results(s->hyp.hyp_done, max_results, out);
  return DSM_OK;
}

int dsm_stream_hypotheses_counts(dsm_stream *s, int *pending_out, int *ready_out) {
  if (!s) return invalid("null stream");
  if (pending_out) *pending_out = (int)s->hyp.groups.size();
  if (ready_out) *ready_out = (int)s->hyp.hyp_done.size();
  return DSM_OK;
}

int dsm_stream_set_hypothesis_window(dsm_stream *s, int window) {
  if (!s || window < 0) return invalid("dsm_stream_set_hypothesis_window: window >= 1, or 0 for all of a group's tries");
  s->hyp.hyp_window = window;
  return DSM_OK;
}

} // extern "C"
