// stream_internal.hpp -- the object behind a dsm_stream handle, for the four files that implement it: stream_capi.hip (the pool and the
// exports around it), stream_pass.hip (engine 0), stream_tick.hip (engine 1) and stream_groups.hip (hypothesis groups).  No other file
// needs it.
//
// Everything a stream holds beyond its queues and counters belongs to one of four owners, as in dsm_context: a plain aggregate whose
// release(), where it holds resources, gives back exactly what it holds and leaves it null.  Who may touch what:
//   arr  (SlotArrays)  both engines index it; allocated by dsm_stream_create, the partials by the first submission
//   pass (PassEngine)  stream_pass.hip alone, and the setters / getters of its schedule in stream_capi.hip
//   tick (TickEngine)  stream_tick.hip alone, and the setters of its switches in stream_capi.hip
//   hyp  (HypGroups)   stream_groups.hip alone; dsm_stream_drain asks whether a group is open
#pragma once
#include <deque>
#include <unordered_map>
#include <utility>
#include <vector>

#include "dsm_internal.hpp"

namespace dsm {

enum { SLOT_FREE = 0, SLOT_NEW = 1, SLOT_RUNNING = 2 };

struct Slot { // the pass engine's host view of a slot
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

} // namespace dsm

struct dsm_stream {
  dsm_context *ctx = nullptr;
  int cap[2] = {0, 0}; // slots of mode 0 (trackNewestCoarse) / mode 1 (optimizeScale); track slots come first
  int N = 0;
  int w = 0, h = 0, nlevels = 0; // geometry of the first tracker submitted; every tracker of the stream must share it
  // the per-slot device arrays and their pinned mirrors
  struct SlotArrays {
    int partial_stride = 0;
    dsm::TrackerDev **d_tracker_ptrs = nullptr, **h_tracker_ptrs = nullptr;
    dsm::LMState *d_states = nullptr, *h_states = nullptr;
    float *d_partials = nullptr;
    dsm::StartInfo *d_start = nullptr, *h_start = nullptr;
    int *d_status = nullptr;
    int *d_tickets = nullptr;
    int *d_rowmap = nullptr, *h_rowmap = nullptr; // [DSM_MAX_LEVELS + 1][N]: rows per level (relative to their segment), then the new slots (relative to their mode's base)
    dsm::LMBuffers lm_buffers() const { return dsm::LMBuffers{d_tracker_ptrs, d_states, d_partials, partial_stride, d_tickets, d_status}; }
    void release();
  } arr;
  std::deque<dsm::Waiting> waiting[2];
  std::deque<dsm_stream_result> done;
  uint64_t next_ticket = 1;
  struct Origin {
    dsm_tracker *trk;
    double pose0[7], aff0[2];
    long long admitted_at; // advance in which the problem was handed to the device (-1: still waiting)
  };
  std::unordered_map<uint64_t, Origin> origin;
  dsm_stats stats[2]{};
  long long retired[2] = {0, 0};
  // advances of EITHER engine that moved something: passes read back plus tick advances enqueued.  The groups' clock (HypGroup::born,
  // dsm_stream_hyp_result::advances) and dsm_stream_get_schedule's passes_out.
  long long advances_done = 0;
  int engine = 1;
  // ---- pass engine (engine 0): the slots' host states and the learnt schedule; holds no resource ----
  struct PassEngine {
    std::vector<dsm::Slot> slots;
    double quantile[DSM_MAX_LEVELS] = {0.75, 0.75, 0.75, 0.75, 0.75, 0.75};
    int fixed_rounds[2][DSM_MAX_LEVELS] = {{0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0}}; // > 0: overrides the learnt schedule
    std::vector<int> hist[2][DSM_MAX_LEVELS];
    size_t hist_pos[2] = {0, 0};
    int rounds[2][DSM_MAX_LEVELS] = {{6, 8, 10, 12, 16, 16}, {4, 4, 4, 4, 4, 4}};
    int rounds_max[2][DSM_MAX_LEVELS] = {{12, 22, 52, 52, 52, 52}, {8, 8, 8, 8, 8, 8}}; // the most any retired problem needed (+ 1)
    long long carried_slot_passes = 0;
  } pass;
  // ---- tick engine (engine 1): every resident problem advances one LM round per tick, admission and retirement on the device ----
  struct TickEngine {
    int ticks = 32; // ticks per advance (one host read-back per advance)
    bool ready = false;
    std::vector<dsm::Seg> segs;
    dsm::TickSegCtl *d_segctl = nullptr, *h_segctl = nullptr;
    dsm::TickModeCtl *d_modectl = nullptr, *h_modectl = nullptr;
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
    dsm::TickPending *d_pending[2] = {nullptr, nullptr}, *h_pending[2] = {nullptr, nullptr}; // waiting rings (device / pinned staging)
    dsm::TickResult *d_results[2] = {nullptr, nullptr}, *h_results[2] = {nullptr, nullptr};   // result rings (device / two pinned copies)
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
    dsm::EvalTimer tm; // per-dispatch events of the advance in flight
    // scheduling switches of the problems in flight, BY VALUE (a tracker may be destroyed as soon as its own result is back -- ADVICE r04:
    // the stream used to keep a pointer into the first submitted tracker's params for its whole life); refreshed at every hand-over
    bool have_sched = false;
    int sched_fixed_schedule = 0, sched_speculate = 0;
    unsigned long long *d_slot_ticket = nullptr;
    long long *d_admit_idx = nullptr; // per slot: the waiting-ring entry it takes at the start of this advance, or -1 (tick_reserve_kernel)
    int parity = 0;
    int resident[2] = {0, 0};
    long long advances = 0, total_ticks = 0;
    // problems of kind m in the device's waiting ring: handed over and, as of the last read-back, not admitted
    long long on_the_way(int m) const { return handed[m] - seen[m].admitted; }
    // something is on its way to the device or back: a problem of either kind handed over and not admitted, or an advance not read back
    bool in_transit() const { return on_the_way(0) != 0 || on_the_way(1) != 0 || collected != advances; }
    // everything tick_setup allocates, the events included; safe on a partially set-up engine, leaves every pointer null and `ready` false
    void release();
  } tick;
  // ---- hypothesis groups ----
  struct HypGroups {
    std::unordered_map<uint64_t, dsm::HypGroup> groups;            // group ticket -> group, until its result is handed back
    std::unordered_map<uint64_t, std::pair<uint64_t, int>> member; // a group try's internal ticket -> (group ticket, try)
    std::deque<dsm_stream_hyp_result> hyp_done;
    int hyp_window = 0; // tries of a group waiting or resident at once after try 0; 0 = all
  } hyp;
};

namespace dsm {
// ---- stream_capi.hip ----
// what every submission checks (and binds the stream's geometry on the first)
int submit_common(dsm_stream *s, int mode, int n, dsm_tracker *const *ts, int coarsest);
// one trackNewestCoarse problem (min_res: DSM_MAX_LEVELS thresholds, NULL = no abort) into the host's waiting queue; returns its ticket
uint64_t enqueue_track(dsm_stream *s, dsm_tracker *t, const double *pose0, const double *aff0, int coarsest_lvl, const double *min_res);
// what a retiring problem started from (kept since its submission); origin.end(): an internal error, reported
std::unordered_map<uint64_t, dsm_stream::Origin>::iterator origin_of(dsm_stream *s, uint64_t ticket);
template <typename T>
int pop_results(std::deque<T> &q, int max_results, T *out) {
  int k = 0;
  for (; k < max_results && !q.empty(); q.pop_front()) out[k++] = q.front();
  return k;
}
// ---- stream_groups.hip ----
// a retired track problem: a group try's result goes to its group, every other result to dsm_stream_results
void route_result(dsm_stream *s, const dsm_stream_result &r);
// ---- stream_pass.hip ----
int pass_advance(dsm_stream *s);
int pass_resident(const dsm_stream *s); // slots taken
// ---- stream_tick.hip ----
int tick_advance(dsm_stream *s);
int tick_sync(dsm_stream *s, long long upto = -1); // the advances before `upto` are read back (default: everything in flight)
int tick_resident(const dsm_stream *s); // slots taken as of the last read-back
} // namespace dsm
