// lm_schedule.hip -- what the host schedulers of the LM kernels share: the batch form (run_lm_batch, batch_capi.hip), the pass engine
// and the tick engine of a dsm_stream (stream_pass.hip, stream_tick.hip).  Segments and their HIP streams, fork and join, the (evaluate, step)
// round with its launch rules, the per-dispatch timing, and the rules of what a problem starts from, what it costs and what it
// writes back.  Host code only; each rule is stated here once.
#include <algorithm>
#include <limits>
#include <utility>

#include "dsm_internal.hpp"

namespace dsm {

// ---- segments and their streams ----
std::vector<Seg> build_segments(int n_streams, int n, int mode, int n2, int mode2) {
  int ng = n_streams < 1 ? 1 : n_streams;
  if (ng > n) ng = n;
  std::vector<Seg> segs;
  for (int g = 0; g < ng; g++) {
    const int g0 = (int)((long long)n * g / ng), g1 = (int)((long long)n * (g + 1) / ng);
    segs.push_back(Seg{nullptr, g0, g1, mode, false, {}});
  }
  if (n2 > 0) segs.push_back(Seg{nullptr, n, n + n2, mode2, true, {}});
  for (Seg &sg : segs) std::fill(sg.rows, sg.rows + DSM_MAX_LEVELS, -1);
  return segs;
}

// Do kernels of streams a and b run at the same time?  (The runtime maps streams onto a few hardware queues -- four by default --
// round robin, together with every other stream of the process; two streams that share a queue serialise.  Measured in round 5: a
// hipMemset on the null stream in dsm_tracker_create shifted the assignment, two of the three stream groups of dsm_stream_* landed on
// one queue, and the bench lost 6 % on 512 frames, 15 % on 256 and 30 % on the sparse template -- profiles/r05_ab_bisect.log.)
// A kernel that stays resident for 400 us on a, an empty one on b behind it in host order: b's finishes early only on another queue.
static int streams_overlap(dsm_context *ctx, hipStream_t a, hipStream_t b, bool *overlap) {
  int khz = 0;
  if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, ctx->device) != hipSuccess || khz <= 0) khz = 100000;
  const double wait_ms = 0.4;
  hipEvent_t e0, e1;
  DSM_HIP(hipEventCreate(&e0));
  DSM_HIP(hipEventCreate(&e1));
  int rc = DSM_OK;
  float ms = 0.f;
  hipError_t e = hipSuccess;
  for (int pass = 0; pass < 2 && e == hipSuccess; pass++) { // (pass 0 loads the two kernels)
    e = hipEventRecord(e0, a);
    launch_queue_probe_wait(a, pass == 0 ? 1 : (long long)(wait_ms * khz));
    launch_queue_probe_empty(b);
    if (e == hipSuccess) e = hipEventRecord(e1, b);
    if (e == hipSuccess) e = hipStreamSynchronize(a);
    if (e == hipSuccess) e = hipStreamSynchronize(b);
  }
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
  hipEventDestroy(e0);
  hipEventDestroy(e1);
  if (e != hipSuccess) rc = hip_fail(e, "queue probe", __FILE__, __LINE__);
  *overlap = ms < 0.5 * wait_ms;
  return rc;
}
// a new stream whose kernels run concurrently with those of every stream in `with` (up to 12 candidates: the runtime hands out its
// queues round robin, so a few rejected candidates later one on a free queue comes up); none found -- fewer hardware queues than
// streams wanted (GPU_MAX_HW_QUEUES) --: the last candidate, counted in ctx->groups.streams_sharing_a_queue
static int create_concurrent_stream(dsm_context *ctx, const std::vector<hipStream_t> &with, hipStream_t *out) {
  std::vector<hipStream_t> rejected;
  hipStream_t found = nullptr;
  int rc = DSM_OK;
  for (int attempt = 0; attempt < 12 && !found && rc == DSM_OK; attempt++) {
    hipStream_t st;
    const hipError_t e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
    if (e != hipSuccess) {
      rc = hip_fail(e, "hipStreamCreateWithFlags", __FILE__, __LINE__);
      break;
    }
    bool ok = true;
    for (size_t i = 0; i < with.size() && ok && rc == DSM_OK; i++) rc = streams_overlap(ctx, with[i], st, &ok);
    if (ok && rc == DSM_OK)
      found = st;
    else
      rejected.push_back(st);
  }
  if (!found && rc == DSM_OK && !rejected.empty()) {
    found = rejected.back();
    rejected.pop_back();
    ctx->groups.streams_sharing_a_queue++;
  }
  for (hipStream_t st : rejected) hipStreamDestroy(st);
  *out = found;
  return rc;
}

// streams of the segments of a launch schedule: `ng` stream groups (the context's stream + ng - 1 extra ones) and, on
// request, the companion stream
static int ensure_streams(dsm_context *ctx, int ng, bool companion) {
  auto in_use = [&]() {
    std::vector<hipStream_t> v{ctx->stream};
    v.insert(v.end(), ctx->groups.extra_streams.begin(), ctx->groups.extra_streams.end());
    if (ctx->groups.companion_stream) v.push_back(ctx->groups.companion_stream);
    return v;
  };
  while ((int)ctx->groups.extra_streams.size() < ng - 1) { // (the groups first: they carry the large kernels)
    hipStream_t st;
    const int rc = create_concurrent_stream(ctx, in_use(), &st);
    if (rc) return rc;
    ctx->groups.extra_streams.push_back(st);
    hipEvent_t ev;
    DSM_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    ctx->groups.join_events.push_back(ev);
  }
  if (companion && !ctx->groups.companion_stream) {
    const int rc = create_concurrent_stream(ctx, in_use(), &ctx->groups.companion_stream);
    if (rc) return rc;
    DSM_HIP(hipEventCreateWithFlags(&ctx->groups.companion_event, hipEventDisableTiming));
  }
  return DSM_OK;
}

int bind_streams(dsm_context *ctx, std::vector<Seg> &segs) {
  int ng = 0;
  for (const Seg &sg : segs) ng += sg.companion ? 0 : 1;
  // (a stream without track slots runs its scale segment, the only one, on the context's stream)
  const int rc = ensure_streams(ctx, ng, !segs.empty() && segs.back().companion && segs.size() > 1);
  if (rc) return rc;
  for (size_t si = 0; si < segs.size(); si++)
    segs[si].st = si == 0 ? ctx->stream : segs[si].companion ? ctx->groups.companion_stream : ctx->groups.extra_streams[si - 1];
  return DSM_OK;
}

int fork_segments(dsm_context *ctx, const std::vector<Seg> &segs, bool with_companion) {
  bool recorded = false;
  for (size_t si = 1; si < segs.size(); si++) {
    if (segs[si].companion && !with_companion) continue;
    if (!recorded) DSM_HIP(hipEventRecord(ctx->groups.fork_event, ctx->stream));
    recorded = true;
    DSM_HIP(hipStreamWaitEvent(segs[si].st, ctx->groups.fork_event, 0));
  }
  return DSM_OK;
}

int join_segments(dsm_context *ctx, const std::vector<Seg> &segs, bool with_companion) {
  for (size_t si = 1; si < segs.size(); si++) {
    if (segs[si].companion && !with_companion) continue;
    hipEvent_t ev = segs[si].companion ? ctx->groups.companion_event : ctx->groups.join_events[si - 1];
    DSM_HIP(hipEventRecord(ev, segs[si].st));
    DSM_HIP(hipStreamWaitEvent(ctx->stream, ev, 0));
  }
  return DSM_OK;
}

// ---- per-dispatch timing ----
hipEvent_t get_event(dsm_context *ctx, size_t idx) {
  while (ctx->timers.ev_pool.size() <= idx) {
    hipEvent_t ev;
    if (hipEventCreate(&ev) != hipSuccess) return nullptr;
    ctx->timers.ev_pool.push_back(ev);
  }
  return ctx->timers.ev_pool[idx];
}

int timed_eval_begin(dsm_context *ctx, const Seg &sg, int L, EvalTimer &tm, hipEvent_t *end) {
  *end = nullptr;
  if (!ctx->timers.timing || sg.companion) return DSM_OK;
  hipEvent_t begin = get_event(ctx, tm.used++);
  *end = get_event(ctx, tm.used++);
  tm.lvl.push_back(L);
  if (begin) DSM_HIP(hipEventRecord(begin, sg.st));
  return DSM_OK;
}

// timing enabled: per-level sums and interval unions of the eval dispatches bracketed by ev_pool[2 i], ev_pool[2 i + 1]
// (level ev_lvl[i]), relative to ev_total[0] (the stream groups' dispatches overlap; the union is the time during which the
// level's kernel ran at all)
void collect_eval_timing(dsm_context *ctx, const std::vector<int> &ev_lvl, int nlevels, dsm_stats &st) {
  std::vector<std::pair<float, float>> iv[DSM_MAX_LEVELS];
  for (size_t i = 0; i < ev_lvl.size(); i++) {
    float m = 0, a = 0;
    if (hipEventElapsedTime(&m, ctx->timers.ev_pool[2 * i], ctx->timers.ev_pool[2 * i + 1]) == hipSuccess &&
        hipEventElapsedTime(&a, ctx->timers.ev_total[0], ctx->timers.ev_pool[2 * i]) == hipSuccess) {
      st.eval_kernel_ms[ev_lvl[i]] += m;
      st.eval_dispatches[ev_lvl[i]]++;
      iv[ev_lvl[i]].push_back(std::make_pair(a, a + m));
    }
  }
  for (int l = 0; l < nlevels; l++) {
    std::sort(iv[l].begin(), iv[l].end());
    double busy = 0, cs = 0, ce = -1;
    for (auto &p : iv[l]) {
      if (ce < 0) {
        cs = p.first, ce = p.second;
      } else if (p.first > ce) {
        busy += ce - cs;
        cs = p.first, ce = p.second;
      } else if (p.second > ce)
        ce = p.second;
    }
    if (ce >= 0) busy += ce - cs;
    st.eval_kernel_union_ms[l] += busy; // (+=: a stream's statistics are cumulative; the batch calls clear theirs per call)
  }
}

// ---- the round ----
int launch_round(dsm_context *ctx, const LMBuffers &B, const dsm_params &P, const Seg &sg, int L, int k, const int *rowmap, const RoundShape &R,
                 EvalTimer &tm) {
  const bool compact = sg.rows[L] >= 0;
  const int rows = compact ? sg.rows[L] : sg.i1 - sg.i0;
  if (rows == 0) return DSM_OK;
  if (!compact) rowmap = nullptr;
  // Speculative second candidate (dsm_device.hpp): doubles the evaluation work of a step to save the launches of
  // rejected steps.  It pays where a launch is latency- and not bandwidth-bound and rejections come in runs: the
  // small levels (a few thousand points).  Measured (S2 dense, launch form): 64 frames +12 %, 512 frames +-0 %, one
  // frame -1 % when applied to every level (the fine levels end on their first rejection), DESIGN.md section 4.3.
  // "Latency-bound" is a property of the launch, not of the level alone: a stream group's launch over G problems of n points
  // evaluates G * n points, and above about a million of them the doubled work costs more than the saved launches give back
  // (S2 dense, 512 + 103 problems in two groups, level 3 = 2.3 M points per launch: 51.3-51.8 k frames/s with the second
  // candidate there, 52.3-52.6 k without; levels 4 and 5, 0.58 M and 0.14 M points, make no measurable difference).
  const bool spec = P.fixed_schedule <= 0 && (P.speculate >= 2 || (P.speculate == 1 && R.level_pts <= 8192 && R.launch_points <= 1000000ll));
  // levels >= 1: the eval kernel's last-arriving workgroup per problem can perform the LM step itself (one launch per
  // round instead of two): for launches of few problems -- small batches (measured: -6 % latency for one frame in flight,
  // -11 % throughput at 256) and compact launches over a handful of stragglers.
  // (Measured on 512 all-distinct S2 frames, same box: fused compact rounds 39.7-40.2 k frames/s, pairs above 8 rows
  // 38.6-38.8 k, the speculative candidate on every level of the compact rounds 38.9 k: the pair's second launch and the
  // doubled rows cost what they save.)
  const bool fused = L > 0 && (P.fuse_lm >= 2 || (P.fuse_lm == 1 && (R.fuse_count <= 8 || R.fuse_also)));
  // Large levels: the residual-only evaluations (the level's last ones; eval_kernel's ROSEL, form_launch.hpp) get a launch of their own
  // behind the full ones -- an instantiation without the 45 accumulators, 30-41 VGPRs = eight waves per SIMD instead
  // of four or five.  Never in a level's first round (its evaluation is the level's first).  Measured (S2 dense, 512
  // frames): level-0 evaluations 4.62 -> 4.40 ms per step, 54.3 -> 55.7 k frames/s with levels 0 and 1 split; with
  // level 2 as well 53.7-55.3 k (the extra launch costs more than it gives there); one frame in flight 0.70 -> 0.74 ms
  // (three more launches), hence the floor on the points per launch.
  const bool split_ro = !sg.companion && !fused && k > 0 && R.level_pts >= 100000 && (long long)rows * R.level_pts >= 8000000ll;
  hipEvent_t eb = nullptr;
  const int rc = timed_eval_begin(ctx, sg, L, tm, &eb);
  if (rc) return rc;
  float *part = B.partials + (size_t)sg.i0 * B.partial_stride;
  launch_eval(sg.st, sg.mode, L, R.grid_x, rows, B.trackers + sg.i0, B.states + sg.i0, part, B.partial_stride, fused ? B.tickets + sg.i0 : nullptr,
              B.status + 2 * sg.i0, spec, split_ro, rowmap);
  if (eb) DSM_HIP(hipEventRecord(eb, sg.st));
  if (!fused)
    launch_lm(sg.st, sg.mode, LM_OP_STEP, L, rows, B.trackers + sg.i0, B.states + sg.i0, part, B.partial_stride, nullptr, nullptr,
              B.status + 2 * sg.i0, spec, rowmap);
  return DSM_OK;
}

// ---- what a problem costs, starts from and writes back ----
// compulsory bytes of one evaluation (what calcRes* reads): the template once + the target image once,
// or, for a sparse template, the four 12-byte taps of every point if that is less
long long eval_bytes(const dsm_tracker *t, int lvl) {
  const long long nl = t->desc.lv[lvl].n, img = 12ll * (t->w >> lvl) * (t->h >> lvl);
  return 16ll * nl + std::min(48ll * nl, img);
}

void fill_track_start(StartInfo &I, const double pose[7], const double aff[2], const double *min_res, int coarsest) {
  memset(&I, 0, sizeof I);
  memcpy(I.pose, pose, sizeof I.pose);
  memcpy(I.aff, aff, sizeof I.aff);
  for (int l = 0; l < DSM_MAX_LEVELS; l++) I.min_res[l] = min_res ? min_res[l] : std::numeric_limits<double>::quiet_NaN();
  I.scale = 1.0f;
  I.coarsest = coarsest;
}

void fill_scale_start(StartInfo &I, float scale, int coarsest) {
  const double identity[7] = {0, 0, 0, 1, 0, 0, 0}, no_aff[2] = {0, 0};
  fill_track_start(I, identity, no_aff, nullptr, coarsest);
  I.scale = scale;
}

// the reference writes lastToNew_out / aff_g2l_out at TrackerAndScaler.cpp:612-613, i.e. also when the later affine
// plausibility checks (:615-626) fail, but not when a level aborts (:598)
bool wrote_pose(int status) { return status == ST_GOOD || status == ST_BAD_AFFINE; }

} // namespace dsm
