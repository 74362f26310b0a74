// dsm_internal.hpp -- host-side objects behind the opaque C handles of include/dsm_hotpath.h
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/dsm_hotpath.h"
#include "dsm_kernels.hpp"

namespace dsm {
void set_error(const std::string &msg);
int hip_fail(hipError_t e, const char *what, const char *file, int line);
} // namespace dsm

#define DSM_HIP(expr)                                                     \
  do {                                                                    \
    hipError_t e__ = (expr);                                              \
    if (e__ != hipSuccess) return dsm::hip_fail(e__, #expr, __FILE__, __LINE__); \
  } while (0)

// Everything the context holds beyond its device and its stream belongs to one of the owners below: a plain aggregate whose release()
// gives back exactly what it holds and leaves it null (context_capi.hip; the arena's in call_arena.hip).  dsm_context_destroy selects
// the device, drains the streams, calls every owner's release() and destroys the stream; whoever grows a buffer is named at its owner.
struct dsm_context {
  int device = 0;
  hipStream_t stream = nullptr;
  // batched calls may split the batch over several streams so that one group's small kernels overlap
  // another group's (dsm_context_set_streams); single calls always use `stream`.  Grown by lm_schedule.hip (bind_streams)
  struct StreamGroups {
    int n_streams = 1;
    std::vector<hipStream_t> extra_streams;
    std::vector<hipEvent_t> join_events;
    hipEvent_t fork_event = nullptr;
    int streams_sharing_a_queue = 0;        // streams of ensure_streams that could not be given a hardware queue of their own
    hipStream_t companion_stream = nullptr; // the companion segment of dsm_track_and_scale_batch
    hipEvent_t companion_event = nullptr;
    void release();
  } groups;
  // descriptor updates of a batch in one copy (sync_descs, tracker_capi.hip): [n descriptors][n destination pointers], pinned + device
  struct DescStaging {
    unsigned char *h_desc_stage = nullptr, *d_desc_stage = nullptr;
    int desc_stage_cap = 0;
    hipEvent_t desc_event = nullptr;
    bool desc_stage_busy = false;
    void release();
  } descs;
  // image hand-over (handover_capi.hip; dsm_tracker_upload_image records copy_event too)
  struct HandOver {
    hipEvent_t copy_event = nullptr; // end of a host->device hand-over (dsm_tracker_upload_image)
    // batched hand-over (dsm_upload_images): copies on a stream of their own, one event per group of images
    hipStream_t copy_stream = nullptr;
    // asynchronous hand-over (dsm_upload_images_async): its own work stream; copies_event = the caller's buffers are
    // free, done_event = the pyramids are built
    hipStream_t upload_stream = nullptr;
    hipEvent_t upload_copies_event = nullptr, upload_done_event = nullptr;
    bool upload_pending = false;
    bool enqueue_pending = false; // dsm_upload_images_enqueue: copy_event not yet waited for
    int async_copy_blocks = 48;  // workgroups of the host-read kernel of the asynchronous hand-over (measured: DESIGN.md section 2)
    std::vector<hipEvent_t> upload_events;
    dsm::PyrJob *d_pyr_jobs = nullptr, *h_pyr_jobs = nullptr; // h: pinned
    int pyr_jobs_cap = 0;
    // before something a hand-over may still touch is freed (a tracker's buffers, an undistorter's tables): the context's stream
    // `main`, the upload stream and the copy stream are idle
    int drain(hipStream_t main);
    // the copies of a pending asynchronous or enqueued hand-over are through: its job table and the caller's buffers are free
    int wait_copies();
    void release();
  } handover;
  // workspaces of the LM batch form (batch_capi.hip: ensure_batch_capacity, run_queue; read by diag_capi.hip and pose_capi.hip; a dsm_stream has
  // slot arrays of its own, stream_internal.hpp)
  struct LmWorkspace {
    int cap_prob = 0;
    int partial_stride = 0; // floats per problem
    dsm::TrackerDev **d_tracker_ptrs = nullptr;
    dsm::TrackerDev **h_tracker_ptrs = nullptr; // pinned
    dsm::LMState *d_states = nullptr;
    dsm::LMState *h_states = nullptr; // pinned
    float *d_partials = nullptr;
    dsm::StartInfo *d_start = nullptr;
    dsm::StartInfo *h_start = nullptr; // pinned
    dsm::SingleOut *d_single = nullptr;
    dsm::SingleOut *h_single = nullptr; // pinned
    int *d_status = nullptr;
    int *h_status = nullptr; // pinned
    dsm::WorkQueue *d_queue = nullptr, *h_queue = nullptr; // work-queue kernel: header (device / pinned copy)
    unsigned long long *d_qitems = nullptr;
    size_t qcap = 0;
    int queue_blocks[3] = {0, 0, 0}; // co-resident grid size per mode
    int *d_rowmap = nullptr, *h_rowmap = nullptr; // compact launches: row -> problem (relative to the segment), device / pinned
    int *d_tickets = nullptr; // per-problem arrival counters of the fused eval+LM kernels (zero between launches)
    void release();
  } lm;
  // the staging arena of every call that stages its inputs, runs its kernels and reads its results back once (the users are listed in
  // call_arena.hpp): device buffer and page-locked mirror, grown and laid out by CallArena alone
  struct ArenaBuffers {
    void *arena_dev = nullptr, *arena_pin = nullptr;
    size_t arena_dev_bytes = 0, arena_pin_bytes = 0;
    void release();
  } arena;
  // the learnt launch schedule of the batch form (batch_capi.hip: account_and_learn); holds no resource
  struct LearntSchedule {
    // speculative launch schedule per mode (0 = track, 1 = scale, 2 = loop-closure pose) and level, adapted after every call
    int sched[3][DSM_MAX_LEVELS] = {{6, 8, 10, 12, 16, 16}, {4, 4, 4, 4, 4, 4}, {6, 8, 10, 12, 16, 16}};
    // ... and the number of launches after which only a level's stragglers are still at work (the third quartile of the
    // rounds the problems of recent calls needed): from there on a round is ONE fused evaluate + step launch (dsm_params.fuse_lm = 1)
    int sched_bulk[3][DSM_MAX_LEVELS] = {{1 << 30, 1 << 30, 1 << 30, 1 << 30, 1 << 30, 1 << 30}, {1 << 30, 1 << 30, 1 << 30, 1 << 30, 1 << 30, 1 << 30},
                                         {1 << 30, 1 << 30, 1 << 30, 1 << 30, 1 << 30, 1 << 30}};
    int sched_bulk_key = -1; // batch-size bucket and launch form the sched_bulk figures were learnt on
  } learnt;
  // stats / timing (ev_pool grown by lm_schedule.hip: get_event)
  struct Timing {
    bool timing = false;
    dsm_stats stats{};
    dsm_stats stats2{}; // companion segment of the last dsm_track_and_scale_batch
    std::vector<hipEvent_t> ev_pool;
    hipEvent_t ev_total[2] = {nullptr, nullptr};
    void release();
  } timers;
};

struct dsm_tracker {
  dsm_context *ctx = nullptr;
  int w = 0, h = 0, nlevels = 0;
  dsm_params params{};
  dsm::TrackerDev desc{}; // host copy of the device descriptor
  dsm::TrackerDev *d_desc = nullptr;
  float4 *d_pts[DSM_MAX_LEVELS] = {};
  int pts_cap[DSM_MAX_LEVELS] = {}; // template capacity per level (w_l*h_l; w*h on every level for the pose estimator)
  float *d_img[2][DSM_MAX_LEVELS] = {};
  float *d_raw[2] = {nullptr, nullptr}; // raw level-0 images of dsm_tracker_upload_image, per slot
  // back buffers of the two frame slots (DSM_SLOT_NEXT_*), swapped in by dsm_frames_advance
  float *d_img_back[2][DSM_MAX_LEVELS] = {};
  float *d_raw_back[2] = {nullptr, nullptr};
  // size of d_raw / d_raw_back once grown past the 4 w h bytes they are allocated with (raw camera images larger than
  // that: dsm_upload_images_undistorted), 0 = not grown; swapped along with the buffers
  size_t raw_bytes[2] = {0, 0}, raw_back_bytes[2] = {0, 0};
  bool have_back[2] = {false, false};
  float back_exposure[2] = {1.f, 1.f};
  bool have_k = false, have_ref = false, have_frame[2] = {false, false};
  int ref_frame_id = -1;
  bool desc_dirty = true;
  // The facts of the template lists and frame buffers above (eval_facts.hpp): device words the kernels that produce a list or a plane
  // write, read by the LM step when a level begins.  A stale 1 is the one way they can make a result wrong, so every path that writes
  // a list or a plane -- a kernel, a copy, whatever comes later -- announces it HERE first, on the stream its writes are ordered on:
  //   kFactClear  the fact is 0 from there on (the general per-point code);
  //   kFactArm    for the producers named in eval_facts.hpp, whose kernels look at every value they write and store 0 on failure.
  // Nothing else writes the words (dsm_diag_tracker_force_general writes its own).
  struct Facts {
    dsm::TrackerFacts *d = nullptr; // zeroed at creation: nothing established
    int set[2] = {0, 1};            // the buffer set behind each frame slot ...
    int back_set[2] = {2, 3};       // ... and behind its back buffers; swapped with the buffers (swap_frames)
    int set_of(int slot) const { return slot >= 2 ? back_set[slot & 1] : set[slot & 1]; } // slot: 0, 1 or DSM_SLOT_NEXT_*
  } facts;
  enum FactUse { kFactClear = 0, kFactArm = 1 };
  // before the lists of every level are written on stream s
  int announce_template_write(hipStream_t s, FactUse use);
  // before the planes of every level behind `slot` (0, 1 or DSM_SLOT_NEXT_*) are written on stream s
  int announce_plane_write(int slot, hipStream_t s, FactUse use);
  // the same for a batched producer whose own first launch arms the words of all its jobs (launch_pyr_facts_arm): no launch here
  int *plane_fact_words(int slot) const { return facts.d ? facts.d->img_plain[facts.set_of(slot)] : nullptr; }
  dsm::LevelFacts *template_fact_words() const { return facts.d ? facts.d->lv : nullptr; }
  // dsm_frames_advance: the facts follow the buffers
  void swap_frame_facts(int s) {
    const int f = facts.set[s];
    facts.set[s] = facts.back_set[s], facts.back_set[s] = f;
    desc.img_set[s] = facts.set[s];
  }
};

// dsm_undistorter_create: the device copy of one camera's undistortion
struct dsm_undistorter {
  dsm_context *ctx = nullptr;
  dsm::UndistortTables tab{}; // device pointers + sizes (dsm_kernels.hpp)
};

// dsm_pose_estimator_create (pose_capi.hip): a tracker whose every level has the level-0 capacity, and the points narrowed to float
struct dsm_pose_estimator {
  dsm_tracker *t = nullptr;
  std::vector<float> x, y, z;
};

// dsm_window_create (immature_kernels.hip): the level-0 intensity planes of a window's keyframes; also a target of trace_kernels.hip and the images of linearize_kernels.hip
struct dsm_window {
  dsm_context *ctx = nullptr;
  int w = 0, h = 0, capacity = 0;
  float *d_planes = nullptr; // capacity planes of w * h floats
  int ids[DSM_WINDOW_MAX_FRAMES] = {};
  bool used[DSM_WINDOW_MAX_FRAMES] = {};
  int find(int id) const {
    for (int i = 0; i < capacity; i++)
      if (used[i] && ids[i] == id) return i;
    return -1;
  }
  float *plane(int i) const { return d_planes + (size_t)i * w * h; }
};

namespace dsm {
int invalid(const char *msg); // set_error + DSM_ERR_INVALID
// points_host.cpp: what both forms of a point call (dsm_*_batch and dsm_*_host) refuse in the settings / in the arrays of a job (NULL: nothing)
const char *activation_job_error(const dsm_activation_job &J, bool with_cand);
const char *immature_settings_error(float huber_th, float min_idepth_h_act, int gn_iterations);
const char *immature_job_error(const dsm_immature_job &J);
const char *trace_params_error(const dsm_trace_params *p);
const char *trace_job_error(const dsm_trace_job &J);
const char *select_params_error(const dsm_select_params *p);
const char *select_geometry_error(int w, int h); // of the level-0 frame
const char *select_job_error(const dsm_select_job &J);
const char *linearize_params_error(const dsm_linearize_params *p);
const char *linearize_job_error(const dsm_linearize_job &J);
// points_host.cpp: B1 and B2 of DESIGN.md section 16 from the job's filled new_energy / new_energy_with_outlier arrays, for both forms
void linearize_job_summary(const dsm_linearize_job &J, const dsm_linearize_params &S);
// points_host.cpp: what both forms of the Hessian call refuse beyond linearize_job_error
// (stitched_required false: the solve call, where H_A, b_A, H_sc and b_sc are optional)
const char *hessian_job_error(const dsm_hessian_job &J, bool stitched_required = true);
// solve_host.cpp: what both forms of the solve call refuse beyond that
const char *solve_job_error(const dsm_solve_job &J);
// step_host.cpp: what both forms of the step call refuse on top of that, before the solve call's rules see the completed job
// 
const char *step_params_error(const dsm_step_params *p);
const char *step_job_error(const dsm_step_job &J);
// optimize_host.cpp: what both forms of the optimize call refuse on top of that, and the job of pass 0 as
// the step call's rules and pieces see it: zeros (n_frames * 8, 4 and n_pts of them) for the three steps, zero factors, `lambda`
const char *optimize_params_error(const dsm_optimize_params *p);
const char *optimize_job_error(const dsm_optimize_job &J);
dsm_step_job optimize_first_pass(const dsm_optimize_job &J, const double *zeros, double lambda);
// finish_host.cpp: what both forms of the finish call refuse on top of that
const char *finish_job_error(const dsm_finish_job &J);
// points_host.cpp: the copies of the optional raw accumulators alone
void hessian_copy_raw(const dsm_hessian_job &J, const double *top, const double *D, const double *E, const double *EB, const double *Hcc,
                      const double *bc);
// points_host.cpp: T1 of section 17 -- H_A, b_A, H_sc, b_sc of the job from its raw accumulators, for both forms; then the copies of
// the optional raw accumulators
void hessian_stitch(const dsm_hessian_job &J, const double *top, const double *D, const double *E, const double *EB, const double *Hcc,
                    const double *bc);
// points_host.cpp: dsm_window_hessian_host with a hook between the linearisation and the accumulation: after_lin (or null) sees the
// linearised job (its J_out holds the rows, the host form's own room where the caller gave none) and may rewrite the rows
int hessian_host_run(int w, int h, const dsm_hessian_job *job, const float *const *frame_I, const dsm_linearize_params *params,
                     void (*after_lin)(void *user, const dsm_linearize_job &L, float *rows), void *user);
// context_capi.hip: the device-visible address of a caller's array if it lies in page-locked memory, else null
const void *pinned_device_pointer(const void *p);
int take_params(const dsm_params *params, dsm_params *out); // the caller's parameters, checked, or the defaults
// tracker_capi.hip: the bytes of one intensity plane; the small host math and the pieces of a tracker's device descriptor
// (dsm_pose_estimate_batch builds its jobs' descriptors from the same pieces)
size_t plane_bytes(int w, int h);
void se3_from_matrix(const double T[16], double pose[7]);
void desc_init(TrackerDev &D, int nlevels, const dsm_params &P);
void desc_cam1(TrackerDev &D, int nlevels, const float K1[4]);
void desc_make_k(TrackerDev &D, int nlevels, float fx, float fy, float cx, float cy);
int sync_desc(dsm_tracker *t);
int sync_descs(dsm_context *ctx, dsm_tracker *const *ts, int n);
int check_ready(dsm_tracker *t, int mode);
// batch_capi.hip: the batch form of the LM scheduler, as the pose estimators and the diagnostic calls run it
int round8(int x);
int prepare_batch(dsm_context *ctx, int n, dsm_tracker *const *ts, int mode, int n2 = 0, int mode2 = 1);
int run_lm_batch(dsm_context *ctx, int n, dsm_tracker *const *ts, int mode, int coarsest, int n2 = 0, int mode2 = 1);
// pose_capi.hip: the loading half of PoseEstimator::estimate (dsm_diag_pose_estimator_eval loads the same way)
int pose_estimator_load(dsm_pose_estimator *pe, int n_pts, const double *xyz, const float *const *ref_colors, float ref_ab_exposure,
                        const float *const *new_dIp, float new_ab_exposure, const float new_cam[4]);

// a device / pinned array of n elements into *p, which is null or holds an earlier allocation (freed first)
template <typename T>
int realloc_dev(T **p, size_t n) {
  if (*p) DSM_HIP(hipFree(*p));
  *p = nullptr;
  DSM_HIP(hipMalloc(p, n * sizeof(T)));
  return DSM_OK;
}
template <typename T>
int realloc_pinned(T **p, size_t n) {
  if (*p) DSM_HIP(hipHostFree(*p));
  *p = nullptr;
  DSM_HIP(hipHostMalloc(p, n * sizeof(T), hipHostMallocDefault));
  return DSM_OK;
}

// an owner's release(): the array goes (null: nothing to do) and the pointer is left null
template <typename T>
void release_dev(T *&p) {
  if (p) (void)hipFree(p);
  p = nullptr;
}
template <typename T>
void release_pinned(T *&p) {
  if (p) (void)hipHostFree(p);
  p = nullptr;
}

// ---- lm_schedule.hip: what the schedulers of the LM kernels share (the batch form, run_lm_batch in batch_capi.hip; the pass
// engine of stream_pass.hip and the tick engine of stream_tick.hip) ----

// A segment of a launch schedule: problems (or slots) [i0, i1) of one mode on one HIP stream.  The main batch is split into
// contiguous stream groups, each with its own HIP stream: a group's lm_kernel -- one small workgroup per problem -- and its
// small-level eval kernels leave most of the chip idle; another group's kernels fill it.  The companion segment (the scale
// problems next to the track problems) follows the groups.  Per-problem results do not depend on the split.
struct Seg {
  hipStream_t st;
  int i0, i1, mode;
  bool companion;
  int rows[DSM_MAX_LEVELS]; // per level, >= 0: compact launches over the first `rows` entries of the segment's row map; -1: one row per problem
};
// n problems of `mode` in min(n_streams, n) contiguous groups, then n2 companion problems of `mode2`
std::vector<Seg> build_segments(int n_streams, int n, int mode, int n2, int mode2);
// segment 0 on the context's stream, the other groups on the extra streams, the companion on its own (created on first use)
int bind_streams(dsm_context *ctx, std::vector<Seg> &segs);
// fork: the other segments' streams start after everything enqueued on the main stream so far; join: the main stream waits for them
int fork_segments(dsm_context *ctx, const std::vector<Seg> &segs, bool with_companion = true);
int join_segments(dsm_context *ctx, const std::vector<Seg> &segs, bool with_companion = true);

struct LMBuffers { // the arrays a scheduler's launches index by problem or slot (dsm_context's batch workspaces, dsm_stream's slot arrays)
  TrackerDev **trackers;
  LMState *states;
  float *partials;
  int partial_stride;
  int *tickets, *status;
};
struct EvalTimer { // a timed call (dsm_context_set_timing): ev_pool[2 i], ev_pool[2 i + 1] bracket evaluation dispatch i, of level lvl[i]
  size_t used = 0;
  std::vector<int> lvl;
};
hipEvent_t get_event(dsm_context *ctx, size_t idx);
// timing on and a main segment: the next pair of events, the first recorded here, *end to be recorded behind the dispatch
int timed_eval_begin(dsm_context *ctx, const Seg &sg, int L, EvalTimer &tm, hipEvent_t *end);
void collect_eval_timing(dsm_context *ctx, const std::vector<int> &ev_lvl, int nlevels, dsm_stats &st);
struct RoundShape { // what differs between the schedulers in one (evaluate, step) round; the rules are launch_round's
  int grid_x, level_pts;   // of the level: chunks per row of the launch, points of the largest template
  long long launch_points; // points one launch evaluates, as the scheduler counts them
  int fuse_count;          // the fused step is for launches of few problems: this count is few ...
  bool fuse_also;          // ... or this holds
};
// round k of level L of a segment; rowmap: the segment's row map for this level (read when sg.rows[L] >= 0)
int launch_round(dsm_context *ctx, const LMBuffers &B, const dsm_params &P, const Seg &sg, int L, int k, const int *rowmap, const RoundShape &R,
                 EvalTimer &tm);

long long eval_bytes(const dsm_tracker *t, int lvl); // compulsory bytes of one evaluation (dsm_stats.algorithmic_bytes)
void fill_track_start(StartInfo &I, const double pose[7], const double aff[2], const double *min_res, int coarsest); // min_res: NULL = no abort
void fill_scale_start(StartInfo &I, float scale, int coarsest);
bool wrote_pose(int status);

// Outputs of a terminated problem; S: its LMState or its TickResult (the same field names).  pose / aff hold what the problem
// started from and keep it unless the problem wrote them (wrote_pose).
template <typename R>
void read_track(const R &S, double pose[7], double aff[2], int *good) {
  if (wrote_pose(S.status)) {
    memcpy(pose, S.cur, sizeof(double) * 7);
    memcpy(aff, S.aff_cur, sizeof(double) * 2);
  }
  if (good) *good = S.status == ST_GOOD ? 1 : 0;
}
template <typename R>
void read_scale(const R &S, float *scale, float *err) {
  *scale = S.scale_cur;                       // TrackerAndScaler.cpp:954
  if (err) *err = (float)S.last_residuals[0]; // :963
}
template <typename R>
void fill_stream_result(dsm_stream_result &r, const R &S, int mode, uint64_t ticket, int passes, const double *pose0, const double *aff0) {
  memset(&r, 0, sizeof r);
  r.ticket = ticket;
  r.kind = mode;
  r.status = S.status;
  r.passes = passes;
  if (mode == 0) {
    memcpy(r.pose, pose0, sizeof r.pose);
    memcpy(r.aff, aff0, sizeof r.aff);
    read_track(S, r.pose, r.aff, &r.good);
    memcpy(r.flow, S.flow, sizeof r.flow);
    r.scale = 1.0f;
  } else {
    r.good = 1;
    read_scale(S, &r.scale, &r.err);
    r.pose[3] = 1.0;
  }
  memcpy(r.last_residuals, S.last_residuals, sizeof r.last_residuals);
  for (int l = 0; l < DSM_MAX_LEVELS; l++) r.evals[l] = S.evals[l];
}
} // namespace dsm
