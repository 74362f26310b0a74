// dsm_kernels.hpp -- host-side launch interface of the HIP kernels, grouped by the file that defines them: tracker_kernels.hip,
// template_kernels.hip, frame_kernels.hip, pose_batch_kernels.hip, diag_kernels.hip, ringkey_kernels.hip.  Internal to the shared
// library; the public boundary is include/dsm_hotpath.h.
#pragma once
#include "dsm_device.hpp"

struct dsm_lm_propose_in; // include/dsm_hotpath.h
struct dsm_lm_propose_out;
struct dsm_lm_step_state;
struct dsm_tick_slot;
struct dsm_tick_slot_out;

namespace dsm {

// Reduction geometry (part of the documented numerics): a workgroup of 256 threads owns a chunk of 256*P
// consecutive template points, thread t handles points chunk*256*P + k*256 + t for k = 0..P-1.  P is chosen per level from its point
// count by one of two tables (dsm_params.chunk_geometry):
//   throughput (0, the default): long chunks -- the per-chunk prologue (three dependent memory round trips before the first point's
//     arithmetic) and epilogue (52 row sums, a barrier, the partial) are paid once per 16 points per thread, and a level of at most 4096
//     points is ONE chunk (the smallest P of 1 / 2 / 4 / 8 / 16 whose 256 P points hold it).  Many problems in flight: the stream, the
//     batched calls.  Round 5's table (16 points per thread from 16 k points up, 8 / 4 / 2 from 4 k / 1 k / 512) measured + 7 % on the
//     streamed bench against the latency table (profiles/r05_ab_geometry.log); round 6's shader-clock stamps inside the tick engine's
//     kernel (profiles/r06_tick_stamps.json) showed its small levels still paying the fixed cost several times over -- a
//     chunk costs about 12 k cycles plus 2 k per point per thread: level 5 of the metric's pyramid (280 points) ran as two workgroups of
//     14.6 k cycles, level 4 (1480) as two of 20 k, level 3 (6688) as four of 28 k; 8.6 % of the kernel's workgroup time for 2.2 % of its bytes
//   latency (1): short chunks -- more workgroups per evaluation, each through sooner: ONE problem in flight (the replay adaptors):
//     0.53 instead of 0.61 ms per frame there
// Results differ between the tables in the last bits of the float sums only (another summation tree); integer outputs are identical.
//   chain (2, round 6): the latency table above 4096 points, ONE chunk up to 4096 (as the throughput table) -- one frame in flight whose
//     small levels run as a chain (an LM loop inside one workgroup: chain_kernel, dsm_params.persistent_coarse < 0; the tick engine's chains)
enum { kGeomThroughput = 0, kGeomLatency = 1, kGeomChain = 2 };
__host__ __device__ inline int pts_per_thread(int n, int geom) {
  if (geom == kGeomLatency || (geom == kGeomChain && n > 4096)) return n >= 256 * 1024 ? 16 : n >= 64 * 1024 ? 8 : n >= 16 * 1024 ? 4 : n >= 4 * 1024 ? 2 : 1;
  return n > 2048 ? 16 : n > 1024 ? 8 : n > 512 ? 4 : n > 256 ? 2 : 1;
}
// chunks of a list of n points at P points per thread
__host__ __device__ inline int chunks_of(int n, int ppt) {
  const int per = kThreads * ppt;
  return (n + per - 1) / per;
}
__host__ __device__ inline int num_chunks(int n, int geom) { return chunks_of(n, pts_per_thread(n, geom)); }

// largest chunk count any n <= cap can produce under either table (P grows with n, so num_chunks is not monotone)
inline int max_chunks_upto(int cap) {
  int best = 0;
  const int edges[8] = {cap, 256 * 1024 - 1, 64 * 1024 - 1, 16 * 1024 - 1, 4 * 1024 - 1, 1023, 511, 255}; // (the latency table's edges; the throughput table's count grows with n)
  for (int g = 0; g < 3; g++)
    for (int e : edges)
      if (e <= cap && num_chunks(e, g) > best) best = num_chunks(e, g);
  return best;
}

enum LMOp {
  LM_OP_STEP = 0,          // consume the evaluation of level `lvl`, advance the LM state machine
  LM_OP_START = 1,         // initialise the state machine at the coarsest level
  LM_OP_SINGLE_PREP = 2,   // dsm_tracker_calc_res_*: build EvalIn from a host supplied pose/scale
  LM_OP_SINGLE_FINISH = 3  // ... and reduce the partials into a SingleOut
};

struct StartInfo { // host -> device, one per problem
  double pose[7];
  double aff[2];
  double min_res[DSM_MAX_LEVELS];
  float scale;
  float cutoff; // single evaluation only
  int coarsest;
  int lvl;      // single evaluation only
  int residual_only; // single evaluation only (dsm_diag_single_eval): EvalIn::residual_only
};

// ---- tracker_kernels.hip (one translation unit; grouped by the part that defines each launcher, in its include order) ----
// -- lm_step.hpp: the LM state machine --
// bounded waits of the LM steps' wave hand-shakes that expired since the library was loaded (0 unless something is badly wrong)
int lm_spin_expired();

// -- form_launch.hpp: launch-per-step form --
// mode: 0 = pose (calcResPose + calcGSSSEPose), 1 = scale (calcResScale + calcGSSSEScale)
// rowmap != nullptr: compact launch over nprob rows, row r = problem rowmap[r] (indices relative to trackers / states)
void launch_eval(hipStream_t s, int mode, int lvl, int grid_x, int nprob,
                 const TrackerDev *const *trackers, const LMState *states, float *partials,
                 int partial_stride, int *tickets, int *status_out, bool spec = false, bool split_ro = false,
                 const int *rowmap = nullptr);
void launch_lm(hipStream_t s, int mode, int op, int lvl, int nprob, const TrackerDev *const *trackers,
               LMState *states, const float *partials, int partial_stride, const StartInfo *start,
               SingleOut *single_out, int *status_out, bool spec = false, const int *rowmap = nullptr);

// -- form_queue.hpp: work-queue form --
// work-queue kernel (queue_kernel): header of the device-side queue, zeroed before every launch; counters on their
// own 128-byte lines.  Items: (index + 1) << 32 | problem << kQueueChunkBits | chunk.
struct WorkQueue {
  unsigned head, pad0[31];
  unsigned tail, pad1[31];
  unsigned done, pad2[31]; // problems that have terminated
  int error, pad3[31];     // a bounded wait expired
};
constexpr int kQueueChunkBits = 12;
int queue_kernel_blocks_per_cu(int mode);
void launch_queue(hipStream_t s, int mode, int nblocks, int nprob, const TrackerDev *const *trackers, LMState *states,
                  float *partials, int partial_stride, int *tickets, WorkQueue *q, unsigned long long *items, unsigned qmask);

// -- form_chain.hpp: chain form --
// persistent LM loop of the levels whose evaluation is ONE chunk (chain_kernel: the tick engine's chain as a launch of its own, one
// workgroup per problem, until the problem reaches a level of several chunks or terminates; no speculative candidates)
void launch_chain(hipStream_t s, int mode, int nprob, const TrackerDev *const *trackers, LMState *states, int *status_out);

// -- form_tick.hpp: tick engine of the streaming form (dsm_stream_*, stream_capi.hip) --
// One TICK advances every resident problem by one LM round, whatever level it stands on: ONE evaluation launch over a
// device-built list of (problem, chunk) items of all levels mixed, then ONE LM launch (a workgroup per slot) that steps the
// problems, builds the next tick's list, retires finished problems into a result array and refills their slots from the
// waiting list -- no host round trip inside an advance of many ticks.
constexpr unsigned kTickNoop = 0x80000000u, kTickCand = 0x40000000u; // item = flags | problem << 12 | chunk
constexpr int kTickChunkBits = 12;
struct TickSegCtl { // one per segment (stream group / companion): item counts of the two lists (tick parity)
  int count[2];
  int overflow; // an item list ran over (cannot happen by construction: checked by the host)
  int chain[2]; // chain entries of the two lists (problems whose pending evaluation is ONE chunk: see tick_eval_kernel), kept behind
                // the list's `cap` item slots
  int pad[27];
};
struct TickModeCtl { // one per problem kind, shared by the kind's segments; every counter is monotonic over the stream's life (64 bits:
                     // 2^31 problems are nine hours at the benchmarked rate)
  long long pending_head, pending_count; // waiting problems: admitted so far (device) / handed over so far (host: the only word it writes)
  long long retired;                     // results written so far
  int ring, pad;                         // entries of the waiting and result rings (a power of two)
  long long sched_evals[DSM_MAX_LEVELS], sched_ro[DSM_MAX_LEVELS]; // evaluations staged (they run in the next tick)
  long long sched_items[DSM_MAX_LEVELS];
};
struct TickPending { // a waiting problem (host -> device)
  StartInfo start;
  const TrackerDev *trk;
  unsigned long long ticket;
};
struct TickResult { // a retired problem (device -> host)
  unsigned long long ticket;
  int status, ticks; // ticks the problem lived (the stream sizes its advances by their mean)
  double cur[7], aff_cur[2];
  double last_residuals[DSM_MAX_LEVELS];
  double flow[3];
  float scale_cur, pad1;
  long long evals[DSM_MAX_LEVELS], evals_ro[DSM_MAX_LEVELS], rounds[DSM_MAX_LEVELS];
};
// start of an advance, before the stream groups fork: which free slot takes which entry of the waiting ring (tick_reserve_kernel)
constexpr int kTickMaxSegs = 20;
struct TickSegDesc {
  int mode, i0, ns;
};
struct TickReserveArgs {
  int nseg;
  TickSegDesc seg[kTickMaxSegs];
};
void launch_tick_reserve(hipStream_t s, const TickReserveArgs &a, const LMState *states, TickModeCtl *mcs, long long *admit_idx);
// the list a tick's LM work appends to (the next tick's evaluations): item slots [0, cap), chain entries [cap, cap + chain_cap)
struct TickList {
  unsigned *items;
  TickSegCtl *seg;
  int buf, cap;
  int chain_cap; // 0: chains off -- every pending evaluation becomes items
  int chain_max_n0; // > 0: only problems whose level-0 template has at most this many points chain (0: all)
};
// what a chain (an evaluation workgroup that also steps its problem, see tick_eval_kernel) needs beyond the evaluation's own arguments
struct TickChainArgs {
  const TrackerDev **trackers;
  LMState *states;
  TickList next;
  TickModeCtl *mc;
  const TickPending *pending;
  TickResult *results;
  unsigned long long *slot_ticket;
  int max_rounds; // LM rounds a chain may run inside one tick
  int flags;      // bit 0: helper wave in the chain's LM step
};
void launch_tick_admit(hipStream_t s, int mode, int nslots, const TrackerDev **trackers, LMState *states, const TickList &list, TickModeCtl *mc,
                       const TickPending *pending, unsigned long long *slot_ticket, const long long *admit_idx);
void launch_tick_eval(hipStream_t s, int mode, int grid, const LMState *states, float *partials, int partial_stride, const unsigned *items,
                      TickSegCtl *seg, int buf, int cap, const TickChainArgs &chain,
                      bool with_chains /* the list may hold chain entries (now or from an earlier setting): the launch must look at them, if only
                                          to turn them into items (chain.max_rounds 0) */);
// the same launch, the list it evaluates given as the TickList it was built as (its chain_cap and chain_max_n0 are not read)
inline void launch_tick_eval(hipStream_t s, int mode, int grid, const LMState *states, float *partials, int partial_stride, const TickList &list,
                             const TickChainArgs &chain, bool with_chains) {
  launch_tick_eval(s, mode, grid, states, partials, partial_stride, list.items, list.seg, list.buf, list.cap, chain, with_chains);
}
void launch_tick_lm(hipStream_t s, int mode, int nslots, const TrackerDev **trackers, LMState *states, const float *partials, int partial_stride,
                    const TickList &next, TickModeCtl *mc, const TickPending *pending, TickResult *results, unsigned long long *slot_ticket,
                    int speculate, int opts /* bit 0: helper waves in the LM step, bit 1: the next items' place in the list asked for early */);

// -- form_diag.hpp: the diagnostic kernels --
// dsm_diag_single_eval: problem 0's staged evaluation (one chunk) in the chains' form, its partial into partials[0 .. 52)
void launch_diag_chain_eval(hipStream_t s, int mode, const LMState *states, float *partials);

// dsm_diag_lm_propose: propose_pose / propose_scale (and the raw solve) on n caller-supplied systems, one workgroup per problem; the
// structures are the public ones of include/dsm_hotpath.h
void launch_diag_lm_propose(hipStream_t s, int mode, int lvl, const TrackerDev *tracker, int n, const ::dsm_lm_propose_in *in,
                            ::dsm_lm_propose_out *out, bool spec, bool helper);

// dsm_diag_lm_step: one production LM step (lm_step_block) per problem on caller-supplied states and partials, one workgroup per
// problem; `states`: n LMState of device scratch the kernel builds the problems in; partials: problem p's at p * partial_stride floats,
// the speculative evaluation's spec_off floats behind (the caller has checked that they fit)
void launch_diag_lm_step(hipStream_t s, int mode, int lvl, const TrackerDev *tracker, int n, const ::dsm_lm_step_state *in,
                         ::dsm_lm_step_state *out, LMState *states, const float *partials, long long partial_stride, bool spec, int spec_off,
                         bool helper, bool coherent);

// dsm_diag_tick_stage: tick_after_step (behind the slot's reservation) on n host-built slot states, one wave per slot in one launch
void launch_diag_tick_stage(hipStream_t s, int mode, int n, const ::dsm_tick_slot *slots, const TrackerDev **trackers, LMState *states,
                            const TickList &list, TickModeCtl *mc, const TickPending *pending, TickResult *results,
                            unsigned long long *slot_ticket, int stepped);
// dsm_diag_tick_step: n slot states built as launch_diag_lm_step builds its problems (slots: the stepped flag, an idle status)
void launch_diag_tick_fill(hipStream_t s, int mode, int lvl, const TrackerDev *tracker, int n, const ::dsm_lm_step_state *in,
                           const ::dsm_tick_slot *slots, LMState *states);
// both: the states as dsm_lm_step_state records, and status / level / flags, ticket and "the tracker pointer is `tracker`" per slot
void launch_diag_tick_unpack(hipStream_t s, int n, const LMState *states, const TrackerDev *const *trackers, const TrackerDev *tracker,
                             const unsigned long long *slot_ticket, ::dsm_lm_step_state *state_out, ::dsm_tick_slot_out *slot_out);

// dsm_diag_eval_facts: {template fact, image fact, pose fact, fast, the bits of the five bounds} of a pose evaluation of level lvl at
// d_pose (7 doubles) into d_out (9 ints)
void launch_diag_eval_facts(hipStream_t s, const TrackerDev *tracker, int lvl, const double *d_pose, int *d_out);

// -- tracker_kernels.hip itself --
// descriptors of many trackers in one launch (sync_descs): d_dst[i] <- d_src[i]
void launch_desc_scatter(hipStream_t s, int n, const TrackerDev *d_src, TrackerDev *const *d_dst);
// Template lists are allocated with this many entries of slack (zeroed).  The evaluation loop prefetches template entries up to three
// trips (3 x 256 points) past the end of a chunk; its buffer loads are range-checked against the list (an entry beyond it reads as
// zeros, never used: masked), so the slack is only a second line of defence for the paths that read the list with plain loads
constexpr int kTemplatePad = 1024;
// chunks of an evaluation of level L of a tracker
inline int level_chunks(const TrackerDev &d, int L) { return num_chunks(d.lv[L].n, d.p.geometry); }

// ---- template_kernels.hip ----
// row A4 / N3: makeCoarseDepthL0 on the device, batched over the keyframes of a call
struct TplJob {
  int npts, pad;
  const float *pt; // [pu | pv | pidepth | pweight], npts each
  float *ws;       // make_coarse_depth_workspace_floats() floats
  const float *ref[DSM_MAX_LEVELS];
  float4 *pts[DSM_MAX_LEVELS];
  int *d_n; // nlevels + 1 ints: template points per level, then the out-of-bounds flag
  LevelFacts *facts; // the armed template-fact words of pts[] (eval_facts.hpp), one per level; null: none kept
};
size_t make_coarse_depth_workspace_floats(int w, int h, int nlevels, int npts);
void launch_make_coarse_depth(hipStream_t s, int w, int h, int nlevels, const TplJob *jobs, int njobs, int max_npts, int texel_floats);

// facts (eval_facts.hpp): the level's armed words, cleared / tightened from the entries as they are written; null: none kept
void launch_interleave_template(hipStream_t s, int n, const float *u, const float *v, const float *id,
                                const float *c, float4 *out, LevelFacts *facts = nullptr);
// the words behind dsm_tracker::announce_*: value 0 clears, 1 arms (flag 1, bounds empty); level bit masks; img_set < 0: no plane
void launch_facts_set(hipStream_t s, TrackerFacts *f, int tpl_levels, int img_set, int img_levels, int value);
void launch_deinterleave_template(hipStream_t s, int n, const float4 *in, float *u, float *v, float *id,
                                  float *c);
void launch_scale_depth(hipStream_t s, int n, float4 *pts, float scale);
struct ScaleDepthArgs { // every level of one template in one launch (blockIdx.y = level)
  int nlevels;
  int n[DSM_MAX_LEVELS];
  float4 *pts[DSM_MAX_LEVELS];
};
void launch_scale_depth_levels(hipStream_t s, const ScaleDepthArgs &a, int max_n, float scale);

// ---- frame_kernels.hip ----
// makeImages (upstream DSO): the intensity plane of level 0 from the float image, of level l from level l-1
// plain (eval_facts.hpp): the armed image-fact words of the levels, cleared where a written pixel fails; null: none kept
void launch_pyramid(hipStream_t s, int w, int h, int nlevels, const float *raw, float *const *img, int *plain = nullptr);
// the reference's (I, dx, dy) texels out of / into an intensity plane; with d_bad != nullptr import counts the texels whose
// gradient channels are not makeImages' central differences of channel 0 (bitwise, or beyond tol) into d_bad[0] and keeps
// the first such index in d_bad[1]
void launch_dip_export(hipStream_t s, int w, int h, const float *plane, float *out3);
void launch_dip_import(hipStream_t s, int w, int h, const float *in3, float *plane, int *d_bad, float tol);
// one image of a batched hand-over (dsm_upload_images): staged level-0 pixels (float or u8) and the pyramid levels
struct PyrJob {
  const void *raw;
  float *img[DSM_MAX_LEVELS];
  const void *src; // device-visible address of the caller's pinned image (kernel copy path), else null
  int *plain;      // the image-fact words of img[] (eval_facts.hpp), armed by launch_pyr_facts_arm; null: none kept
};
// arms the words of every job: the first launch of a batched pyramid build
void launch_pyr_facts_arm(hipStream_t s, const PyrJob *d_jobs, int njobs, int nlevels);
// raw <- src for every job, rows of row_bytes at pitch `pitch` in src (tight in raw); unit: 16, 4 or 1 bytes per access
void launch_host_rows_copy(hipStream_t s, const PyrJob *d_jobs, int njobs, int row_bytes, int rows, size_t pitch, int unit, int max_blocks);
void launch_pyramid_batched(hipStream_t s, int w, int h, int nlevels, const PyrJob *d_jobs, int njobs, bool u8);
// dsm_undistorter: remap = w_out * h_out (x, y) source coordinates (x < 0: outside; null: passthrough), G = 256 floats,
// vig = w_in * h_in inverse vignette (each null when absent)
struct UndistortTables {
  int w_in, h_in, w_out, h_out;
  const float2 *remap;
  const float *G, *vig;
};
// the batched pyramids of dsm_upload_images_undistorted: level 0 (and 1) from the staged camera bytes of every job, the
// other levels as launch_pyramid_batched builds them -- as many launches as that
void launch_undistort_pyramid_batched(hipStream_t s, const UndistortTables &u, int nlevels, const PyrJob *d_jobs, int njobs);

// ---- pose_batch_kernels.hip ----
// dsm_pose_estimate_batch: one job's template pack and one job's pyramid import
struct PosePackJob {
  const double *xyz;                // n x 3 (the staged arena, or the caller's page-locked array)
  const float *col[DSM_MAX_LEVELS]; // n each
  float4 *pts[DSM_MAX_LEVELS];      // n + kTemplatePad entries each
  int n, pad;
};
struct PoseImportJob {
  const float *in3[DSM_MAX_LEVELS]; // staged (I, dx, dy) texels, 16-byte aligned
  float *plane[DSM_MAX_LEVELS];     // intensity planes, 16-byte aligned
  int *bad;                         // [level]{count, smallest index} of the gradient check
};
// every level of every job in one launch; max_n: the largest n of the table
void launch_pose_pack(hipStream_t s, const PosePackJob *d_jobs, int njobs, int nlevels, int max_n);
// every level of a wave of jobs in one launch; check: count the texels whose gradient channels are not makeImages' (as launch_dip_import)
void launch_pose_import(hipStream_t s, const PoseImportJob *d_jobs, int njobs, int w, int h, int nlevels, bool check, float tol);

// ---- diag_kernels.hip ----
// queue probe of ensure_streams: a kernel resident for `ticks` of the wall clock, and an empty one
void launch_queue_probe_wait(hipStream_t s, long long ticks);
void launch_queue_probe_empty(hipStream_t s);

// ---- ringkey_kernels.hip ----
void launch_ringkey_knn(hipStream_t s, const float *keysT, int64_t cap, int64_t n_local, int dim,
                        int k, float thres, int shard_rank, int shard_count, const float *d_queries,
                        int nq, unsigned long long *d_scratch, int n_slices,
                        unsigned long long *d_packed_out);
int ringkey_num_slices(int64_t n_local, int nq, int dim);
// the form (DSM_RINGKEY_FORM_*, include/dsm_hotpath.h) that launch_ringkey_knn takes for nq queries, and the keys of one slice of a form
int ringkey_scan_form(int dim, int nq);
long long ringkey_slice_keys(int64_t n_local, int n_slices, int form);
void launch_ringkey_insert(hipStream_t s, float *keysT, int64_t cap, int64_t pos, int dim,
                           const float *d_key, int nkeys);
// many indexes in one call (dsm_ringdb_query_then_enqueue_many, dsm_loop_detect_batch_many): query q scans its own index
struct RingKeyScanDesc {
  const float *keysT; // the index's dimension-major planes
  long long cap, n_local;
  float thres;
  int n_slices; // ringkey_many_slices(n_local)
};
// matured key i of the call goes to slot pos of its index's planes
struct RingKeyInsertDesc {
  float *keysT;
  long long cap, pos;
};
int ringkey_many_slices(int64_t n_local);
// the form that launch_ringkey_knn_many takes (four: every capacity of the call is a multiple of four)
int ringkey_many_form(int dim, bool four);
// one scan over all nq queries (each over its own index, d_queries nq x dim) into d_scratch (n_slices = the largest count of the call),
// then ringkey_merge_kernel into d_packed_out (nq x k).  four: every capacity a multiple of four (16-byte plane loads; ringkey_many_form)
void launch_ringkey_knn_many(hipStream_t s, const RingKeyScanDesc *d_descs, int dim, int k, bool four, const float *d_queries, int nq,
                             int n_slices, unsigned long long *d_scratch, unsigned long long *d_packed_out);
// one launch appending nkeys keys (nkeys x dim) to their indexes
void launch_ringkey_insert_many(hipStream_t s, const RingKeyInsertDesc *d_descs, int dim, const float *d_keys, int nkeys);

} // namespace dsm
