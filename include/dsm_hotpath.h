/*
 * dsm_hotpath.h -- C ABI of the MI355X-native direct photometric hot path.
 *
 * Drop-in boundary for the hot path of IRVLab/direct_stereo_slam.
 * The reference has no FFI layer: the seam is the C++ class `dso::TrackerAndScaler`
 * (src/scale_optimization/TrackerAndScaler.h:34-137) and the free functions
 * `search_ringkey` / `search_sc` (src/loop_closure/loop_detection/search_place.h:25-84).
 * Every entry point below names the reference interface it replaces (file:line,
 * relative to the reference tree).  The host adaptor that keeps the reference's C++
 * surface on top of this ABI is direct_stereo_slam_amd/host/TrackerAndScaler.hpp; the
 * reference-side binding is shown in INTEGRATION.md.
 *
 * Conventions
 *  - plain C, POD only, no exceptions; every function returns DSM_OK (0) or a negative
 *    dsm_status.  dsm_last_error() gives a thread-local human readable message.
 *  - all image / template data is IEEE float32; poses and affine brightness are float64
 *    exactly as the reference keeps them (Sophus SE3d, AffLight{double a,b}).
 *  - pose layout: double[7] = {qx, qy, qz, qw, tx, ty, tz} (Eigen quaternion coefficient
 *    order, then translation) for the transform refToNew / lastToNew.
 *  - host pointers are read during the call and never retained after it returns.
 *  - one HIP stream per context; one call in flight per context (the reference calls
 *    this path under track_mutex_ / coarse_tracker_swap_mutex_, FrontEnd.cpp:589,628).
 *  - there is NO CPU fallback: every entry point fails with DSM_ERR_NO_DEVICE when no
 *    gfx950 device is usable.
 */
#ifndef DSM_HOTPATH_H
#define DSM_HOTPATH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSM_ABI_VERSION 4 /* 2: dsm_params.struct_size / fixed_schedule / frame_check / frame_grad_tol, dsm_stats.evals_residual_only;
                             3: dsm_params_default_sized / DSM_PARAMS_INIT, dsm_stream_* (streaming form of the batched calls);
                             4: dsm_params.chunk_geometry takes the slot of version 3's tile_l0 -- same layout, another meaning: 0 now
                                selects the THROUGHPUT chunk table (float sums differ in their last bits from versions <= 3, whose only
                                table is today's 1 = LATENCY), and a version-3 caller's tile_l0 = 1 would silently select the latency
                                table -- hence the bump; dsm_set_refs_from_points requires one geometry per call */
#define DSM_MAX_LEVELS 6 /* DSO PYR_LEVELS; the reference tracker uses <= 5 (TrackerAndScaler.cpp:457,463) */

typedef enum dsm_status {
  DSM_OK = 0,
  DSM_ERR_INVALID = -1,   /* bad argument */
  DSM_ERR_NO_DEVICE = -2, /* no usable HIP device */
  DSM_ERR_HIP = -3,       /* HIP runtime error, see dsm_last_error() */
  DSM_ERR_STATE = -4,     /* call order violated (e.g. track before set_ref) */
  DSM_ERR_NOMEM = -5
} dsm_status;

typedef struct dsm_context dsm_context; /* device + stream + workspaces */
typedef struct dsm_tracker dsm_tracker; /* one TrackerAndScaler instance */
typedef struct dsm_ringdb dsm_ringdb;   /* ring-key database + delay queue */
typedef struct dsm_comm dsm_comm;       /* communicator of the sharded ring-key database: one rank per GPU (RCCL) */
typedef struct dsm_pose_estimator dsm_pose_estimator; /* loop-closure direct alignment (PoseEstimator) */
typedef struct dsm_distmap dsm_distmap; /* one CoarseDistanceMap: the level-1 distance map of a window */
typedef struct dsm_window dsm_window;   /* the level-0 intensity planes of the keyframes of one window (frame_hessians_) */
typedef struct dsm_pixel_selector dsm_pixel_selector; /* PixelSelector: the random pattern and all scratch of dsm_select_pixels_batch */

/* Runtime parameters.  These are DSO globals / literals in the reference; the values
 * written by dsm_params_default() are the upstream DSO defaults as used by the
 * reference's default `mode=1` (src/main.cpp:117-121). */
typedef struct dsm_params {
  size_t struct_size;                 /* sizeof(dsm_params) of the header the CALLER was built with: set by DSM_PARAMS_INIT /
                                         dsm_params_default_sized from the size the caller's compiler sees; every entry point
                                         that takes parameters returns DSM_ERR_INVALID on a mismatch, so a host built against
                                         another version of this header fails loudly instead of handing over a shorter
                                         struct.  Hosts should also compare dsm_abi_version() with DSM_ABI_VERSION once (the
                                         Python and C++ adaptors in this repository do). */
  float huber_th;                     /* setting_huberTH            (TrackerAndScaler.cpp:727,795)   9    */
  float coarse_cutoff_th;             /* setting_coarseCutoffTH     (TrackerAndScaler.cpp:476)       20   */
  float scale_xi_rot;                 /* SCALE_XI_ROT               (TrackerAndScaler.cpp:542,685)   1    */
  float scale_xi_trans;               /* SCALE_XI_TRANS             (TrackerAndScaler.cpp:543,686)   0.5  */
  float scale_a;                      /* SCALE_A                    (TrackerAndScaler.cpp:544,687)   10   */
  float scale_b;                      /* SCALE_B                    (TrackerAndScaler.cpp:545,688)   1000 */
  float affine_opt_mode_a;            /* setting_affineOptModeA     (TrackerAndScaler.cpp:511-534)   0    */
  float affine_opt_mode_b;            /* setting_affineOptModeB                                      0    */
  float lambda_extrapolation_limit;   /* literal                    (TrackerAndScaler.cpp:464,863)   0.001*/
  int max_iterations[DSM_MAX_LEVELS]; /* literal {10,20,50,50,50}   (TrackerAndScaler.cpp:463,862); [5]=50 is an extension */
  int adaptive_schedule;              /* 1 (default): speculative per-level launch counts learnt from previous calls, one
                                         host read-back per pass (plus, with compact_tail, one per level and stream group in the
                                         first pass); 0: enqueue the worst case (2*(7+max_iterations) launch
                                         pairs per level) and never poll.  Scheduling only -- results are identical. */
  int persistent_coarse;              /* N < 0: the CHAIN form for single calls -- every level whose evaluation is ONE chunk
                                         (chunk_geometry) runs its LM loop in one launch per problem (evaluate, reduce, step on an LDS
                                         copy of the state; global gathers, no speculative candidates), down to the first level of
                                         several chunks, where the launch-per-step schedule takes over: one frame in flight saves a
                                         launch per LM round of its coarse levels (with chunk_geometry 2: what the replay adaptors
                                         set).  Scheduling only -- bit-identical under the same chunk table.
                                         0 (default): one (evaluate, step) launch pair per LM evaluation at every level.
                                         N > 0: accepted and run as 0 (it selected an LDS-resident small-level kernel, since
                                         retired: DESIGN_HISTORY.md section 4.2). */
  int fuse_lm;                        /* at pyramid levels >= 1 the evaluation kernel's last-arriving workgroup of a
                                         problem can perform the LM step itself (one launch per evaluation instead of
                                         two): 0 never, 1 (default) for batches of at most 8 problems (where it shortens
                                         the latency chain), 2 always.  Scheduling only -- results are bit-identical. */
  int work_queue;                     /* the whole call as ONE launch of persistent workgroups that pull (problem, chunk)
                                         items from a device-side queue; the workgroup completing an evaluation performs
                                         the LM step and enqueues the problem's next evaluation, so problems advance
                                         independently instead of in lock-step launches: 0 never, 1 (default) for batches
                                         of at least 32 problems with at most 24576 finest-level chunks in all (beyond
                                         that the lock-step launches are faster), 2 always.  Scheduling only -- results
                                         are bit-identical. */
  int speculate;                      /* launch-per-step form: next to the LM proposal being evaluated, the proposal that
                                         FOLLOWS IF IT IS REJECTED (same H, b, pose; lambda x 4, TrackerAndScaler.cpp:583-585)
                                         is evaluated in the same launch, so a rejected step -- about half of all steps on
                                         the coarse levels -- costs no launch of its own.  Same evaluations, decisions and
                                         per-level evaluation counts as the sequential loop; the speculative evaluation of
                                         an ACCEPTED step is discarded (not counted).  0 never, 1 (default) on levels of at most
                                         8192 template points whose launches evaluate at most a million points per stream
                                         group (where launches are latency-bound and rejections come in runs),
                                         2 on every level.  Scheduling only -- results are bit-identical. */
  int compact_tail;                   /* launch-per-step form, batches: 1 (default) after the rounds most problems of a level
                                         need (learnt from previous calls) the host reads the level's status back ONCE and
                                         runs the remaining rounds -- needed by a few stragglers -- as compact launches over
                                         those problems only, and every later pass over the problems still running; 0 every
                                         launch covers every problem (idle workgroups cost ~1.6 ns each: 100 us for a level-0
                                         launch over 512 problems).  Scheduling only -- results are bit-identical. */
  int fixed_schedule;                 /* K > 0: BENCHMARK schedule of SURVEY.md section 8d -- every level runs exactly one
                                         initial evaluation + K LM iterations whose steps are ALL taken (no accept test, no
                                         cut-off repeat, no small-step break, no abort), so that the evaluations and bytes
                                         per frame do not depend on the input.  Not the reference's algorithm: 0 (default)
                                         runs trackNewestCoarse / optimizeScale as written. */
  int chunk_geometry;                 /* Reduction geometry: which table gives a chunk's points per thread from the level's point count
                                         (a chunk = one workgroup's share of an evaluation = one partial).
                                         0 (default) THROUGHPUT: 16 points per thread; a level of at most 4096 points is ONE chunk (the smallest
                                           of 1 / 2 / 4 / 8 / 16 points per thread that holds it) --
                                           long chunks, their fixed cost (three dependent memory round trips before the first
                                           point, the 52-sum reduction after the last) amortised: many problems in flight.
                                           (ABI version 3's table 0 -- 16 from 16 k points up, 8 / 4 / 2 from 4 k / 1 k / 512 -- gave the
                                           small levels several short chunks; version 4's float sums there differ in their last bits.)
                                         1 LATENCY: 16 / 8 / 4 / 2 from 256 k / 64 k / 16 k / 4 k points, else 1 -- short chunks, more
                                           workgroups per evaluation, a single evaluation through sooner: ONE problem in flight
                                           Rounds 1-4 used this table for everything.
                                         2 CHAIN (round 6): table 1 above 4096 points, ONE chunk up to 4096 points (as table 0): one problem
                                           in flight whose small levels run as a chain (persistent_coarse < 0; the tick engine's chains):
                                           what the replay adaptors set.
                                         Every form (single, batch, stream) follows the tracker's table: results of one tracker are
                                         bit-identical across forms; between the tables only the summation tree of the float sums
                                         differs (last bits), integer outputs are equal.  dsm_reduction_geometry reports the choice.
                                         (This slot was round 4's tile_l0, RESERVED = 0 since: a caller that leaves it 0 gets the default.) */
  int frame_check;                    /* dsm_tracker_upload_frame: 1 (default) verify that the caller's gradient channels
                                         are makeImages' central differences of channel 0 (the device stores channel 0 only);
                                         0 trust the caller (channels 1, 2 are ignored) */
  float frame_grad_tol;               /* with frame_check = 1: 0 (default) bitwise equality; t > 0 accepts
                                         |g - g'| <= t * max(1, |g'|) per texel and channel (a host whose makeImages was built
                                         with other floating-point flags) */
} dsm_params;

/* Statistics of the last track / optimize_scale (batch) call on a context. */
typedef struct dsm_stats {
  int64_t evals[DSM_MAX_LEVELS];        /* evaluations executed, summed over the batch: fused residual + Jacobian (calcRes* +
                                           calcGSSSE*), except the evals_residual_only below */
  int64_t launches[DSM_MAX_LEVELS];     /* eval kernel launches per level */
  int64_t algorithmic_bytes;            /* sum over evals of 16*n_l + min(12*w_l*h_l, 48*n_l)   */
  double eval_kernel_ms[DSM_MAX_LEVELS];/* summed HIP-event durations of the eval kernel dispatches per level (timing enabled) */
  double eval_kernel_union_ms[DSM_MAX_LEVELS]; /* time during which at least one of them ran (stream groups overlap) */
  int64_t eval_dispatches[DSM_MAX_LEVELS];     /* timed dispatches per level (launches x stream groups) */
  double total_ms;                      /* HIP-event time of the whole call */
  int64_t polls;                        /* host read-backs of the device LM state (passes) */
  int64_t coarse_launches;              /* 1 when the call ran its small levels in chain_kernel (persistent_coarse < 0), else 0 */
  int64_t queue_blocks;                 /* work-queue kernel: persistent workgroups launched (0: launch-per-step form) */
  int64_t queue_items;                  /* work-queue kernel: (problem, chunk) items processed */
  double queue_kernel_ms;               /* work-queue kernel: HIP-event duration of the launch (timing enabled) */
  int64_t evals_residual_only[DSM_MAX_LEVELS]; /* of evals[]: the last evaluation of a level's LM loop when the loop is known
                                           to end after it (increment below 1e-3, TrackerAndScaler.cpp:588 / :937, or the
                                           iteration bound): the reference runs calcGSSSE* on it and never reads the result;
                                           here only calcRes* is executed for it */
} dsm_stats;

const char *dsm_last_error(void);
int dsm_abi_version(void);
/* Defaults into the CALLER's struct: caller_size = sizeof(dsm_params) as the caller's compiler sees it.  The library
 * writes min(caller_size, its own sizeof) bytes -- never past the end of the caller's struct -- records caller_size in
 * struct_size, and returns DSM_ERR_INVALID when the two sizes differ (the caller was built against another header; every
 * entry point taking the struct would refuse it too).  Use the macro. */
int dsm_params_default_sized(dsm_params *p, size_t caller_size);
#define DSM_PARAMS_INIT(p) dsm_params_default_sized((p), sizeof(dsm_params))
/* the same without the size: ONLY for callers known to be built with this very header (the Python binding checks
 * dsm_abi_version() first): it writes the library's sizeof(dsm_params) bytes */
void dsm_params_default(dsm_params *p);

/* ---- context ------------------------------------------------------------------------- */
int dsm_context_create(int device_ordinal, dsm_context **out);
int dsm_context_destroy(dsm_context *ctx);
int dsm_context_sync(dsm_context *ctx);
/* enable per-level HIP-event timing of the eval kernels (off by default) */
int dsm_context_set_timing(dsm_context *ctx, int enable);
int dsm_context_get_stats(dsm_context *ctx, dsm_stats *out);
/* batched calls: split the batch into n_streams groups on separate HIP streams so that the small
 * (latency-bound) kernels of one group overlap the kernels of another; results are unchanged.  Default 1. */
int dsm_context_set_streams(dsm_context *ctx, int n_streams);
/* raw hipStream_t of the context (for callers that order their own device work) */
void *dsm_context_stream(dsm_context *ctx);
/* The stream groups (dsm_context_set_streams, dsm_stream_*) only overlap if their HIP streams sit on different HARDWARE queues; the
 * runtime hands its few queues (GPU_MAX_HW_QUEUES, 4 by default) out round robin to every stream of the process.  The library therefore
 * probes each stream it creates for a group (a resident kernel on one, an empty kernel on the other: docs in csrc/lm_schedule.hip, ensure_streams) and keeps
 * only streams that run concurrently with the groups it already has.  streams_out: group streams in use (the context's own included),
 * sharing_out: how many of them had to share a queue with another group after 12 candidates (0 on a default runtime). */
int dsm_context_stream_queues(dsm_context *ctx, int *streams_out, int *sharing_out);

/* measurement aid (no reference counterpart): read-only streaming bandwidth of the device in GB/s,
 * `bytes` per pass (choose > 256 MiB to defeat the Infinity Cache), `iters` timed passes */
int dsm_diag_read_bandwidth(dsm_context *ctx, size_t bytes, int iters, double *gbps_out);
/* same, but each workgroup streams its own contiguous chunk of `chunk_bytes` (the access pattern of the
 * evaluation kernels) instead of all workgroups advancing through memory side by side */
int dsm_diag_read_bandwidth_chunked(dsm_context *ctx, size_t bytes, size_t chunk_bytes, int iters, double *gbps_out);
/* test aid: message-passing litmus of the hand-off protocol the kernels use between workgroups (device-scope stores,
 * drained store queue, ticket; device-scope loads on the other side): `pairs` producer / consumer workgroup pairs on
 * different XCDs exchange `iters` 256-byte blocks each under uneven load; *stale_words_out = words read that were not the
 * announced hand-off's (must be 0). */
int dsm_diag_xwg_litmus(dsm_context *ctx, int pairs, int iters, long long *handoffs_out, long long *stale_words_out);

/* ---- TrackerAndScaler ---------------------------------------------------------------- */
/* replaces TrackerAndScaler::TrackerAndScaler(w,h,tfm_vec,K1)  (TrackerAndScaler.cpp:47-109).
 * T_f1_f0: row-major 4x4 stereo extrinsic (cams/<set>/T_stereo.yaml); K1 = {fx,fy,cx,cy} of camera 1. */
int dsm_tracker_create(dsm_context *ctx, int w, int h, int nlevels, const double T_f1_f0[16],
                       const float K1[4], const dsm_params *params, dsm_tracker **out);
/* replaces ~TrackerAndScaler (TrackerAndScaler.cpp:111-115) */
int dsm_tracker_destroy(dsm_tracker *t);
/* replaces TrackerAndScaler::makeK(CalibHessian*) (TrackerAndScaler.cpp:117-141) */
int dsm_tracker_make_k(dsm_tracker *t, float fx, float fy, float cx, float cy);
/* replaces the OUTPUT of TrackerAndScaler::setCoarseTrackingRef (TrackerAndScaler.cpp:317-327):
 * the per-level template lists pc_u/pc_v/pc_idepth/pc_color with pc_n (built by
 * makeCoarseDepthL0 :143-315, or by dsm_make_coarse_depth_l0 below), plus refFrameID,
 * lastRef_aff_g2l and lastRef->ab_exposure. */
int dsm_tracker_set_ref(dsm_tracker *t, int ref_frame_id, double ref_aff_a, double ref_aff_b,
                        float ref_exposure, const int *n, const float *const *pc_u,
                        const float *const *pc_v, const float *const *pc_idepth,
                        const float *const *pc_color);
/* "next" row N3: makeCoarseDepthL0 + setCoarseTrackingRef (TrackerAndScaler.cpp:143-327) on the device.
 * The window's active points as flat arrays -- (pu,pv) = centerProjectedTo[0..1], pidepth =
 * centerProjectedTo[2], pweight = sqrtf(1e-3/(HdiF+1e-12)) (:155-158) -- are splatted, pyramided, dilated
 * and emitted (row-major, the reference's order) straight into this tracker's template; the keyframe's
 * (I,dx,dy) pyramid is the one already resident in `frame_owner`'s `slot` (the tracker that tracked the frame
 * which became the keyframe; may be `t` itself).  Result identical to dsm_make_coarse_depth_l0 +
 * dsm_tracker_set_ref, without the host loops and the template upload.  n_out (may be NULL): pc_n per level.
 * COORDINATES: a point is accepted exactly when pu + 0.5f and pv + 0.5f (float) are finite and truncate toward zero into
 * [0, w) x [0, h), i.e. -1 < pu + 0.5f < w and -1 < pv + 0.5f < h; so -1.4 lands on pixel 0, and NaN, +-inf, 1e20, -1.6 and w - 0.5
 * are refused.  One refused point fails the whole call with DSM_ERR_INVALID (the reference would write out of bounds, :160) and
 * leaves the tracker without a reference. */
int dsm_tracker_set_ref_from_points(dsm_tracker *t, dsm_tracker *frame_owner, int slot, int ref_frame_id,
                                    double ref_aff_a, double ref_aff_b, float ref_exposure, int npts,
                                    const float *pu, const float *pv, const float *pidepth, const float *pweight,
                                    int *n_out);
/* The same for the new keyframes of several sequences in ONE call (a node serving many sequences, dsm_stream_*): every job's
 * splat / pyramid / dilate / emit launches are enqueued back to back and the host waits ONCE for all the per-level counts.
 * A tracker may appear as `t` in one job only; results per job as dsm_tracker_set_ref_from_points.  On an error no tracker of
 * the batch has a valid reference any more.
 * ONE GEOMETRY PER CALL: every job's tracker must share image width, height and level count (the launches are batched over the
 * jobs: blockIdx.y = job); a call that mixes geometries returns DSM_ERR_INVALID before anything is enqueued -- callers with
 * trackers of several sizes issue one call per size (the per-job loop of ABI versions <= 3 accepted mixed sizes). */
typedef struct dsm_ref_job {
  dsm_tracker *t, *frame_owner;
  int slot, ref_frame_id;
  double ref_aff_a, ref_aff_b;
  float ref_exposure;
  int npts;
  const float *pu, *pv, *pidepth, *pweight;
  int *n_out; /* may be NULL */
} dsm_ref_job;
int dsm_set_refs_from_points(dsm_context *ctx, int n_jobs, const dsm_ref_job *jobs);
/* replaces TrackerAndScaler::scaleCoarseDepthL0(scale) (TrackerAndScaler.cpp:329-336) */
int dsm_tracker_scale_depth(dsm_tracker *t, float scale);
/* read back the device template of one level (tests; debugPlotIDepthMap replacement) */
int dsm_tracker_get_template(dsm_tracker *t, int lvl, int *n, float *pc_u, float *pc_v,
                             float *pc_idepth, float *pc_color);

enum { DSM_SLOT_NEW_LEFT = 0, DSM_SLOT_NEW_RIGHT = 1 };
/* replaces the consumption of FrameHessian::dIp[lvl] (TrackerAndScaler.cpp:709,1016):
 * dIp[lvl] is the reference's AoS Eigen::Vector3f (I,dx,dy) array of w_l*h_l texels.  The device keeps channel 0 only
 * and forms the gradients where they are interpolated, from the neighbouring intensities, exactly as
 * FrameHessian::makeImages (upstream DSO) defines them -- dx = 0.5 (I[idx+1] - I[idx-1]), dy = 0.5 (I[idx+w] - I[idx-w]),
 * zero where not finite -- which is the only way the reference ever fills channels 1 and 2.  The call verifies that
 * (rows 1 .. h_l-2; makeImages leaves the first and last row unset and the tracker never reads them; bitwise, or to
 * dsm_params.frame_grad_tol) and returns DSM_ERR_INVALID -- naming the first offending level and texel -- for texels that
 * were built any other way; dsm_params.frame_check = 0 skips the check. */
int dsm_tracker_upload_frame(dsm_tracker *t, int slot, const float *const *dIp, float ab_exposure);
/* the same hand-over without the gradient channels: I[lvl] = the w_l*h_l intensities of level lvl (channel 0 of dIp[lvl]),
 * 4 bytes per texel over the link instead of 12 and nothing to verify */
int dsm_tracker_upload_intensity(dsm_tracker *t, int slot, const float *const *I, float ab_exposure);
/* "next" row N1: build the pyramid on the device from the level-0 float image (upstream DSO FrameHessian::makeImages,
 * call sites FrontEnd.cpp:605,680): the intensity plane of every level; see dsm_tracker_upload_frame. */
int dsm_tracker_upload_image(dsm_tracker *t, int slot, const float *image, float ab_exposure);
/* the same hand-over for many frames in ONE call (the frames of a batched track / scale call): host->device copies
 * back to back on a copy stream, pyramids of a group of images built under the copies of the next group, five batched
 * launches per group instead of five per image.  images[i]: level-0 pixels of trackers[i]'s geometry (all trackers of one
 * call share w, h, levels), DSM_PIXEL_F32 (the undistorted float image FrontEnd.cpp:605,680 consume) or DSM_PIXEL_U8
 * (camera bytes, main.cpp:216-217 "mono8"; converted exactly on the device -- valid when no photometric calibration is
 * applied, i.e. float(pixel) is what the reference's undistorter hands on; otherwise see dsm_upload_images_undistorted).
 * row_pitch_bytes: distance between image rows in the caller's buffers, 0 = tight; with a pointer to the crop origin this
 * approximates the calibration file's crop (cams/kitti/0_2/camera0.txt:2-4) by a window -- upstream's crop rescales the
 * whole valid image instead.  Returns when every copy has completed. */
enum { DSM_PIXEL_F32 = 0, DSM_PIXEL_U8 = 1 };
int dsm_upload_images(dsm_context *ctx, int n, dsm_tracker *const *trackers, const int *slots, const void *const *images,
                      const float *ab_exposures, int pixel_type, size_t row_pitch_bytes);
/* Double-buffered hand-over, so that the images of step i+1 travel while step i is being tracked:
 *   slots DSM_SLOT_NEXT_LEFT / DSM_SLOT_NEXT_RIGHT name the BACK buffers of the two frame slots (allocated on first
 *   use); dsm_frames_advance swaps back and front of the given (tracker, slot in {0,1}) pairs -- a host-side pointer
 *   swap -- and orders the context's stream after the pyramids of the last asynchronous hand-over.
 *   dsm_upload_images_async enqueues copies and pyramid kernels on a stream of its own and returns at once; the caller's
 *   buffers must stay untouched until dsm_upload_wait returns (pinned buffers are read by the GPU itself).  Track /
 *   scale calls issued meanwhile read the front buffers only.  No reference counterpart: the reference processes one
 *   frame at a time on one thread (FrontEnd.cpp:589). */
enum { DSM_SLOT_NEXT_LEFT = 2, DSM_SLOT_NEXT_RIGHT = 3 };
int dsm_upload_images_async(dsm_context *ctx, int n, dsm_tracker *const *trackers, const int *slots, const void *const *images,
                            const float *ab_exposures, int pixel_type, size_t row_pitch_bytes);
int dsm_upload_wait(dsm_context *ctx);
/* dsm_upload_images into the FRONT buffers, stream-ordered: copies and pyramid kernels are enqueued on the context's stream -- every
 * track / scale call and every dsm_stream_advance issued afterwards finds the frames in place -- and the call returns WITHOUT waiting
 * for the copies.  For page-locked capture buffers that outlive the hand-over (a node's frame ring): the caller's buffers must stay
 * untouched until dsm_upload_wait, the next dsm_upload_images* call on the context or any call that synchronises its stream.
 * Pageable buffers are handed over as dsm_upload_images does (the call then waits for their copies).  No reference counterpart. */
int dsm_upload_images_enqueue(dsm_context *ctx, int n, dsm_tracker *const *trackers, const int *slots, const void *const *images,
                              const float *ab_exposures, int pixel_type, size_t row_pitch_bytes);
int dsm_frames_advance(dsm_context *ctx, int n, dsm_tracker *const *trackers, const int *slots);

/* ---- undistortion and photometric calibration at the hand-over (main.cpp:246-256) ---------------------------------------
 * The reference undistorts both camera images of every frame on the host before addActiveStereoFrame
 * (undistorterN_->undistort<unsigned char>(&img, 1, 0, 1.0f), UPSTREAM-DSO Undistort::undistort): photometric correction
 * (response G[256], vignette) followed by a bilinear remap to the output camera.  The calls below do the same on the device
 * from the raw mono8 camera bytes.  DESIGN.md section 9 lists every upstream quirk that is kept and the one deviation. */
enum { DSM_UNDISTORT_CROP = 0, DSM_UNDISTORT_NONE = 1, DSM_UNDISTORT_EXPLICIT = 2 };
/* The remap of UPSTREAM-DSO's Pinhole model (Undistort::readFromFile + makeOptimalK_crop + UndistortPinhole::distortCoordinates),
 * host code.  calib = fx fy cx cy of the camera file's first line, as read there (double; relative when cx < 1 && cy < 1);
 * out_mode: CROP (line 3 "crop"), NONE ("none": w_out, h_out must equal w_in, h_in) or EXPLICIT (line 3 = "fx fy cx cy 0",
 * relative to the output size, out_calib = its first four numbers; ignored otherwise).  Writes the output camera K_out
 * (fx, fy, cx, cy; what Undistort::getK() returns, i.e. what makeK gets), *passthrough (1 for NONE) and, unless
 * passthrough, remap_x / remap_y (w_out * h_out source coordinates each, -1 = outside).  All float32, fixed evaluation
 * order.  DSM_ERR_INVALID when makeOptimalK_crop does not converge in 500 iterations (upstream aborts the process). */
int dsm_pinhole_undistort_map(const double calib[4], int w_in, int h_in, int out_mode, const float out_calib[4], int w_out, int h_out,
                              float K_out[4], int *passthrough, float *remap_x, float *remap_y);
/* Device copy of one camera's undistortion (UPSTREAM-DSO Undistort + PhotometricUndistorter): remap_x / remap_y as
 * dsm_pinhole_undistort_map writes them (or any caller-made table, e.g. of another camera model); both NULL =
 * passthrough (w_out, h_out must equal w_in, h_in).  G: 256 floats, the response already rescaled as
 * PhotometricUndistorter keeps it; vignette_inv: w_in * h_in floats, the inverse vignette.  Each may be NULL
 * (setting_photometricCalibration 0: neither, 1: G only, 2: both).  The tables are copied once.  Every table entry must
 * be outside (x < 0) or have its whole bilinear 2x2 footprint inside the source image; anything else returns
 * DSM_ERR_INVALID naming the first such entry, so the device never reads outside the staged camera image. */
typedef struct dsm_undistorter dsm_undistorter;
int dsm_undistorter_create(dsm_context *ctx, int w_in, int h_in, int w_out, int h_out, const float *remap_x, const float *remap_y,
                           const float *G, const float *vignette_inv, dsm_undistorter **out);
int dsm_undistorter_destroy(dsm_undistorter *u);
/* The batched hand-over (dsm_upload_images) from RAW camera bytes: images[i] = w_in x h_in mono8 pixels (row_pitch_bytes
 * between rows, 0 = tight), pinned or pageable.  Every tracker must have the undistorter's output size.  Level 0 is, bit
 * for bit, what Undistort::undistort<unsigned char>(img, 1, 0, 1.0f) hands on (photometric value G[byte] or float(byte),
 * times vignette_inv; bilinear remap in upstream's order; 0 outside); the other levels follow as makeImages builds them.
 * form: DSM_UPLOAD_SYNC / _ASYNC / _ENQUEUE, with exactly the semantics of dsm_upload_images / dsm_upload_images_async
 * (DSM_SLOT_NEXT_* + dsm_frames_advance) / dsm_upload_images_enqueue.  ab_exposures as there: the reference passes
 * exposure 1. */
enum { DSM_UPLOAD_SYNC = 0, DSM_UPLOAD_ASYNC = 1, DSM_UPLOAD_ENQUEUE = 2 };
int dsm_upload_images_undistorted(dsm_context *ctx, const dsm_undistorter *u, int n, dsm_tracker *const *trackers, const int *slots,
                                  const void *const *images_u8, const float *ab_exposures, size_t row_pitch_bytes, int form);

/* pinned host memory for images handed to dsm_tracker_upload_image (straight DMA instead of a staged copy); no reference
 * counterpart -- the reference keeps its images in ordinary host memory */
int dsm_host_alloc(size_t bytes, void **out);
int dsm_host_free(void *p);
/* read back one pyramid level as the reference's AoS (I,dx,dy) texels (gradients as makeImages forms them, zero in the
 * first and last row) */
int dsm_tracker_get_frame(dsm_tracker *t, int slot, int lvl, float *dIp_out);

/* replaces calcResPose + calcGSSSEPose as ONE fused evaluation (TrackerAndScaler.cpp:699-852, 640-697).
 * rs[6] as the reference's Vec6; H row-major 8x8 and b[8] in double, already SCALE_*-scaled.
 * n_warped = pose_buf_warped_n_ (padded to a multiple of 4). */
int dsm_tracker_calc_res_pose(dsm_tracker *t, int lvl, const double pose[7], const double aff[2],
                              float cutoff_th, double rs[6], double H[64], double b[8],
                              int *n_warped);
/* replaces calcResScale + calcGSSSEScale (TrackerAndScaler.cpp:1007-1172, 966-1005) */
int dsm_tracker_calc_res_scale(dsm_tracker *t, int lvl, float scale, float cutoff_th, double rs[6],
                               float *H, float *b, int *n_warped);
/* test aid (no reference counterpart): ONE evaluation as dsm_tracker_calc_res_pose (mode 0) / _scale (mode 1) runs it -- the same
 * preparation, the same reduction of the chunk partials, outputs of the same meaning (H, b: mode 0; Hs, bs: mode 1; pose, aff: mode 0;
 * scale: mode 1) -- with the evaluation itself launched in a chosen form of the evaluation loop:
 *   0  the evaluation kernel of the direct calls (with residual_only = 0: bit for bit what dsm_tracker_calc_res_* return);
 *   1  the split pair of the batched schedules: the kernel of the full evaluations, then the kernel of the residual-only ones;
 *   2  the tick engine's kernel (dsm_stream_*) over an item list of this evaluation's chunks;
 *   3  the one-chunk form of the chains (dsm_params.persistent_coarse < 0, the tick engine's chains): the partial formed in LDS.  Only for a
 *      level of at most one chunk under the tracker's chunk table (dsm_reduction_geometry); DSM_ERR_INVALID otherwise.
 * residual_only != 0: the evaluation that ends an LM loop -- energy, counts and flow indicators; the normal equations are not formed
 * (H, b, Hs, bs come back as zeros).  A bad mode, form or level is DSM_ERR_INVALID with nothing written.  No production path calls this. */
int dsm_diag_single_eval(dsm_tracker *t, int mode, int lvl, const double pose[7], const double aff[2], float scale, float cutoff_th,
                         int form, int residual_only, double rs[6], double H[64], double b[8], float *Hs, float *bs, int *n_warped);
/* test aid (no reference counterpart): the facts that decide which instantiation of the per-point stages a pose evaluation (mode 0)
 * of level lvl at pose {qx,qy,qz,qw,tx,ty,tz} runs, derived on the device by the code the production path runs (one thread):
 *   out[0]  the template fact of the level's list: every entry has 2^-64 <= idepth and finite u, v;
 *   out[1]  the image fact of the new left frame's plane of that level: every pixel has |I| <= 2^100;
 *   out[2]  the pose fact: 2^-21 <= pt2 < 2^31 for every point inside the list's bounds (meaningful while out[0] is 1);
 *   out[3]  1 if the evaluation takes the instantiation without the settled checks where its kernel has one (all three facts, the
 *           tracker not forced general; the tick engine's kernel and the chains have one on every level, the launch form's kernel on
 *           level 0, the work-queue kernel none), else 0.
 * bounds (may be NULL): the list's {umin, umax, vmin, vmax, idepth max} as the evaluation's inputs carry them (meaningful while out[0]
 * is 1; an empty list's are {+inf, -inf, +inf, -inf, -inf}).
 * DSM_ERR_INVALID with nothing written for a NULL t, pose or out or a bad level.  No production path calls this. */
int dsm_diag_eval_facts(dsm_tracker *t, int lvl, const double pose[7], int out[4], float bounds[5]);
/* host forms of the rules behind those facts, compiled from the inline functions the kernels run (no device needed):
 * dsm_pose_fact_host: the pose fact of n rows {M6, M7, M8, t2, xmin, xmax, ymin, ymax, idmax} into out[n] (0 / 1);
 * dsm_fact_rules_host: per value v[i], out[4 i ..] = {the order-preserving integer key the bounds are kept as, the bits of the value that
 * key turns back into, bit 0: v passes as a template entry's inverse depth, bit 1: as its coordinate, whether v passes as a pixel}.
 * DSM_ERR_INVALID for a negative n or a NULL array with n > 0. */
int dsm_pose_fact_host(int n, const float *rows9, int *out);
int dsm_fact_rules_host(int n, const float *v, int *out);
/* test aid: on != 0 makes every evaluation of this tracker whose level begins from here on take the general instantiation whatever the
 * facts say (the facts themselves are left alone); on = 0 ends that.  Waits for the context's stream.  No production path calls this. */
int dsm_diag_tracker_force_general(dsm_tracker *t, int on);
/* test aid (no reference counterpart): ONE evaluation of the loop-closure alignment (mode 2: PoseEstimator::calcRes + calcGSSSE,
 * PoseEstimator.cpp:84-296) at level lvl, pose {qx,qy,qz,qw,tx,ty,tz} and affine pair aff.  The inputs are those of
 * dsm_pose_estimator_estimate and are loaded by the same function (makeK(new_cam), the points narrowed to float, the reference with
 * affine (0, 0), the new frame's pyramid); the evaluation then runs as dsm_diag_single_eval runs one -- the direct calls' preparation
 * and reduction, outputs of dsm_tracker_calc_res_pose's meaning -- launched in form
 *   0  the evaluation kernel the estimator's LM run launches per step (eval_kernel<2, LVL0, false, 0>);
 *   1  the split pair: the kernel of the full evaluations, then the kernel of the residual-only ones;
 *   3  the chains' one-chunk form (chain_kernel<2>'s two instantiations of the loop under its register budget), for a level of at
 *      most one chunk under the estimator's chunk table; DSM_ERR_INVALID otherwise.
 * Form 2 (the tick engine) has no loop-closure instantiation and no caller: DSM_ERR_INVALID.  residual_only != 0: energy, counts and
 * flow indicators; H and b come back as zeros.  DSM_ERR_INVALID with nothing written for a NULL pe, xyz, ref_colors, new_dIp,
 * new_cam, pose or aff, n_pts < 1 or > w*h, a bad level or form.  rs, H, b, n_warped may be NULL.  No production path calls this. */
int dsm_diag_pose_estimator_eval(dsm_pose_estimator *pe, int n_pts, const double *xyz, const float *const *ref_colors,
                                 float ref_ab_exposure, const float *const *new_dIp, float new_ab_exposure, const float new_cam[4],
                                 int lvl, const double pose[7], const double aff[2], float cutoff_th, int form, int residual_only,
                                 double rs[6], double H[64], double b[8], int *n_warped);

/* test aid (no reference counterpart): the second half of a Levenberg-Marquardt round -- the step that turns H, b and lambda into the
 * next candidate (TrackerAndScaler.cpp:505-554 pose, :897-913 scale) -- run by the production device code on caller-supplied
 * systems, n problems in one launch (one workgroup each).  The tracker supplies what the step reads of it: the parameters, K^-1 of
 * level lvl (dsm_tracker_make_k must have been called), the reference affine and the exposures; no template or frame is needed.
 * mode: 0 pose, 2 loop-closure pose (M = R instead of R K^-1, reference affine (0, 0)), 1 stereo scale.
 * spec != 0: the proposal is staged as the speculative candidate (consumed one iteration later: the iteration bound is tested at
 * iteration + 2).  helper != 0 (modes 0, 2): a second wave forms the affine part and the cut-off of the candidate's evaluation, as in
 * the production step.  DSM_ERR_INVALID with nothing written for a NULL pointer, n < 1 or n > 65536, a bad mode or level, or a tracker
 * without makeK; DSM_ERR_STATE (outputs not written) when a bounded wait of the wave hand-shake expired during the call.
 * No production path calls this. */
typedef struct dsm_lm_propose_in {
  double H[64], b[8];       /* modes 0, 2: the normal equations, row-major; only the lower triangle of H is read */
  double cur[7], aff_cur[2]; /* modes 0, 2: the current pose {qx,qy,qz,qw,tx,ty,tz} and affine pair */
  float lambda;
  float level_cutoff_repeat; /* cut-off of the candidate's evaluation = coarse_cutoff_th * level_cutoff_repeat */
  int iteration;             /* iterations of the level already consumed */
  float Hs, bs, scale_cur;   /* mode 1 */
} dsm_lm_propose_in;
typedef struct dsm_lm_propose_out {
  double inc[8];   /* modes 0, 2: the solve's raw increment (before extrapolation and SCALE_*) */
  double inc_norm; /* |inc| after extrapolation (:588) */
  double cand[7], aff_cand[2];
  /* the candidate's part of the inputs of its evaluation */
  float M[9], t[3], aff0, aff1, cutoff, max_energy;
  int residual_only;
  float Ki[9];     /* K^-1 of the level, as the evaluation reads it */
  float inc_f, scale_cand; /* mode 1 */
  int pad[2];
} dsm_lm_propose_out;
int dsm_diag_lm_propose(dsm_tracker *t, int mode, int lvl, int n, const dsm_lm_propose_in *in, int spec, int helper,
                        dsm_lm_propose_out *out);

/* test aid (no reference counterpart): the FIRST half of a Levenberg-Marquardt round -- the fixed-order reduction of an evaluation's
 * chunk partials, their conversion into rs, H and b, and the state machine that consumes them (the cut-off repeat, accept / reject,
 * the lambda update, the iteration bound, the "small step" test, the consumption of a speculative candidate, the end of a level, the
 * level repeat, the hand-down and the verdicts: TrackerAndScaler.cpp:475-489, :556-638 pose, :873-885, :913-964 scale) -- run by the
 * production device code (one unchanged LM step per problem, one workgroup each, n problems per call) on caller-supplied states and
 * partials.  A step that goes on also stages the next proposal, as dsm_diag_lm_propose runs it alone.  The tracker supplies the
 * parameters, K^-1 of the levels (dsm_tracker_make_k must have been called), the reference affine and the exposures; no template or
 * frame is needed.  mode: 0 pose, 1 stereo scale, 2 loop-closure pose; every problem of a call stands on level lvl.
 * The state goes in and comes out in the same structure, so that a result can be handed to the next call as it is:
 *   in:  every field but status and lvl (the problem is running, at lvl) and, of ev and spec_ev, what the level alone determines:
 *        Ki and n, in mode 1 also M, t, aff0, aff1, in modes 0 and 2 scale (1).  nch = chunks of the evaluation the step consumes.
 *   out: every field after the step; status (DSM_LM_RUNNING ...), lvl (the level the problem now stands on), ev / spec_ev = the main
 *        and the speculative evaluation as staged (what the step did not write is as handed in); nch as handed in.
 * partials: problem p's chunk partials at partials + p * partial_stride, chunk-major, 64 floats per chunk, slots 49-51 integer bit
 * patterns; spec != 0: the step is given a speculative block (it consumes the speculative evaluation where spec_valid is set and may
 * stage a new one) and the speculative evaluation's partials sit spec_off floats behind the main ones.  helper != 0 (modes 0, 2):
 * helper waves form the affine part of the staged evaluations, as in production.  coherent != 0: the instantiation that reads and
 * writes the state with device-coherent accesses (the work-queue form's).
 * DSM_ERR_INVALID with nothing written for a NULL pointer (partials included), n < 1 or n > 65536, a bad mode or level, a tracker
 * without makeK, a phase other than 0 / 1, nch < 0 or > 4096, a partial_stride that is not a multiple of 4 in 4 .. 2^24, with spec a
 * spec_off that is negative or not a multiple of 4, or partials that would not fit: 64 nch > (spec ? spec_off : partial_stride),
 * spec_off + 64 nch > partial_stride.  DSM_ERR_STATE (outputs not written) when a bounded wait of the wave hand-shake expired during
 * the call.  No production path calls this. */
enum { DSM_LM_IDLE = 0, DSM_LM_RUNNING = 1, DSM_LM_GOOD = 2, DSM_LM_ABORTED = 3, DSM_LM_BAD_AFFINE = 4 };
typedef struct dsm_lm_step_eval { /* the candidate's part of the inputs of an evaluation */
  float M[9], t[3], aff0, aff1, cutoff, max_energy;
  int residual_only;
  float scale; /* mode 1 */
  float Ki[9]; /* out: K^-1 of the level the evaluation is staged for */
  int n;       /* out: template points of that level */
} dsm_lm_step_eval;
typedef struct dsm_lm_step_state {
  double H[64], b[8]; /* modes 0, 2 */
  double cur[7], aff_cur[2], cand[7], aff_cand[2];
  double spec_cand[7], spec_aff_cand[2];
  double inc_norm, spec_inc_norm;
  double res_old[6];
  double min_res[DSM_MAX_LEVELS], last_residuals[DSM_MAX_LEVELS], last_inners[DSM_MAX_LEVELS], flow[3];
  long long evals[DSM_MAX_LEVELS], evals_ro[DSM_MAX_LEVELS], rounds[DSM_MAX_LEVELS];
  int status, lvl; /* out */
  int phase;       /* 0: the level's first evaluation is pending, 1: a proposal's */
  int iteration, have_repeated, coarsest, spec_valid, ticks;
  float lambda, level_cutoff_repeat;
  float inc_f, spec_inc_f, scale_cur, scale_cand, spec_scale_cand, Hs, bs; /* mode 1 */
  int nch;
  dsm_lm_step_eval ev, spec_ev;
} dsm_lm_step_state;
int dsm_diag_lm_step(dsm_tracker *t, int mode, int lvl, int n, const dsm_lm_step_state *in, const float *partials,
                     long long partial_stride, int spec, int spec_off, int helper, int coherent, dsm_lm_step_state *out);

/* test aids (no reference counterpart): the tick engine's reservation, admission and item lists (csrc/form_tick.hpp) alone.  Each call
 * builds its inputs in device memory, runs the production device code unchanged and copies back everything that code may have written.
 * The words behind an item list are cap + chain_cap + G, G = every word every slot of the call could write (its reservation, both
 * candidates' positions, the first items of a problem admitted into it), all prefilled with DSM_TICK_SENTINEL -- neither a no-op nor
 * an item of a call's slots (n <= 65536): a write the list's bounds should have stopped shows as a changed word behind `cap`, never
 * as a fault.  No call waits on another workgroup.  No production path calls these.
 *
 * dsm_diag_tick_reserve: tick_reserve_kernel on nseg segment descriptors over nslots slots (running[s] != 0: slot s holds a running
 *   problem) and the waiting rings' head / count of both kinds.  admit_idx[s]: the ring index slot s takes, -1 for none, -2 where no
 *   segment covers the slot; head_out: both heads afterwards; *ctl_intact: no other word of the two control blocks changed.
 *   DSM_ERR_INVALID (nothing written): a NULL argument, nseg < 0 or > DSM_TICK_MAX_SEGS, nslots < 1 or > 65536, a segment with a mode
 *   other than 0 / 1, a negative i0 or ns, or slots beyond nslots.
 * dsm_diag_tick_stage: n crafted post-step slot states, one wave per slot and all in one launch; each wave makes the slot's
 *   reservation (reserve 0: none; 1 / 2: TickReserve::operator() with want_spec 0 / 1; 3: res_base, res_total as given) and calls
 *   tick_after_step as tick_lm_kernel does, with `stepped`.  The waiting ring holds n_pending entries from ctl->pending_head on (every
 *   one this tracker, its own start and ticket); ctl->pending_count may not exceed head + n_pending.
 *   Outputs: items[0 .. *items_len) -- with items NULL the call only writes the length it needs to *items_len --, the segment's and
 *   the kind's control blocks, the result ring (ctl->ring entries, prefilled with bytes 0xA5), per slot a dsm_tick_slot_out and the
 *   state as a dsm_lm_step_state (nch: the chunks of the evaluation now pending) and as raw bytes (state_bytes each, n of them), and
 *   per pending entry what launch_lm(LM_OP_START) leaves in a zeroed state, raw (start_raw).
 * dsm_diag_tick_step: the production tick_admit_kernel (admit_idx != NULL: per slot the ring index to take or -1) and then the
 *   production tick_lm_kernel with `speculate` and `opts` on n slots built as dsm_diag_lm_step builds its problems (all at level lvl,
 *   partials as there, the speculative ones partial_stride / 2 behind); slot[s].status DSM_LM_IDLE: a free slot (the state as built,
 *   but idle); slot[s].stepped: the state's flag.  opts: bits 0 and 1 are tick_lm_kernel's (helper waves, the early reservation),
 *   bit 2: the admission alone, no LM launch.  admit_idx names entries of [pending_head, pending_head + n_pending) only.  The list
 *   written is buffer list->buf; buffer buf ^ 1 starts with count and chain 7 (tick_lm_kernel's slot 0 clears them).  The trackers[]
 *   of the slots start as a copy of the descriptor, so tracker_set tells an admission's pointer.  Outputs as dsm_diag_tick_stage's.
 * DSM_ERR_INVALID (nothing written) for both: a NULL argument, n < 1 or n > 65536, a point count whose positions do not fit the item
 *   encoding, a ring that is not a power of two in 1 .. 2^20, negative cap, counts, offsets or heads, count > cap, chain > chain_cap,
 *   buf other than 0 / 1, an explicit reservation outside [0, cap + chain_cap + G), pending_count > pending_head + n_pending,
 *   n_pending > ring, *items_len smaller than needed; and what dsm_diag_lm_step refuses. */
#define DSM_TICK_SENTINEL 0x3FFFF5A5u
#define DSM_TICK_NOOP 0x80000000u
#define DSM_TICK_CAND 0x40000000u
#define DSM_TICK_CHUNK_BITS 12
#define DSM_TICK_MAX_SEGS 20
typedef struct dsm_tick_seg {
  int mode, i0, ns;
} dsm_tick_seg;
typedef struct dsm_tick_list_cfg {
  int cap, chain_cap, chain_max_n0, buf;
  int count, chain; /* of buffer buf, at the start */
} dsm_tick_list_cfg;
typedef struct dsm_tick_seg_ctl { /* TickSegCtl */
  int count[2], overflow, chain[2], pad[27];
} dsm_tick_seg_ctl;
typedef struct dsm_tick_mode_ctl { /* TickModeCtl */
  long long pending_head, pending_count, retired;
  int ring, pad;
  long long sched_evals[DSM_MAX_LEVELS], sched_ro[DSM_MAX_LEVELS], sched_items[DSM_MAX_LEVELS];
} dsm_tick_mode_ctl;
typedef struct dsm_tick_pending { /* a waiting problem: what dsm_stream_submit_* hands over */
  double pose[7], aff[2], min_res[DSM_MAX_LEVELS];
  float scale;
  int coarsest;
  unsigned long long ticket;
} dsm_tick_pending;
typedef struct dsm_tick_result { /* TickResult */
  unsigned long long ticket;
  int status, ticks;
  double cur[7], aff_cur[2], last_residuals[DSM_MAX_LEVELS], flow[3];
  float scale_cur, pad1;
  long long evals[DSM_MAX_LEVELS], evals_ro[DSM_MAX_LEVELS], rounds[DSM_MAX_LEVELS];
} dsm_tick_result;
typedef struct dsm_tick_slot { /* dsm_diag_tick_stage: a slot after its step; dsm_diag_tick_step: status, stepped and ticket alone */
  int status, lvl, n, ppt, spec_valid, n0, residual_only, ticks; /* n, ppt: EvalIn::n / ppt of the pending evaluation */
  int stepped, reserve, res_base, res_total;
  unsigned long long ticket;
  double cur[7], aff_cur[2], last_residuals[DSM_MAX_LEVELS], flow[3]; /* what a terminated slot's result carries */
  float scale_cur, pad1;
  long long evals[DSM_MAX_LEVELS], evals_ro[DSM_MAX_LEVELS], rounds[DSM_MAX_LEVELS];
} dsm_tick_slot;
typedef struct dsm_tick_slot_out {
  int status, lvl, stepped, n, ppt, spec_valid, n0, residual_only;
  int tracker_set, pad; /* trackers[slot] is the tracker's descriptor (an admission wrote it) */
  unsigned long long ticket; /* slot_ticket[slot] */
} dsm_tick_slot_out;
int dsm_diag_tick_reserve(dsm_context *ctx, int nseg, const dsm_tick_seg *segs, int nslots, const unsigned char *running,
                          const long long head[2], const long long count[2], long long *admit_idx, long long head_out[2], int *ctl_intact);
int dsm_diag_tick_stage(dsm_tracker *t, int mode, int n, const dsm_tick_slot *slots, const dsm_tick_list_cfg *list,
                        const dsm_tick_mode_ctl *ctl, int n_pending, const dsm_tick_pending *pending, int stepped, unsigned *items,
                        int *items_len, dsm_tick_seg_ctl *seg_out, dsm_tick_mode_ctl *ctl_out, dsm_tick_result *results,
                        dsm_tick_slot_out *slot_out, dsm_lm_step_state *state_out, unsigned char *state_raw, int *state_bytes,
                        unsigned char *start_raw);
int dsm_diag_tick_step(dsm_tracker *t, int mode, int lvl, int n, const dsm_lm_step_state *in, const dsm_tick_slot *slots,
                       const float *partials, long long partial_stride, int speculate, int opts, const dsm_tick_list_cfg *list,
                       const dsm_tick_mode_ctl *ctl, int n_pending, const dsm_tick_pending *pending, const long long *admit_idx,
                       unsigned *items, int *items_len, dsm_tick_seg_ctl *seg_out, dsm_tick_mode_ctl *ctl_out, dsm_tick_result *results,
                       dsm_tick_slot_out *slot_out, dsm_lm_step_state *state_out, unsigned char *state_raw, int *state_bytes,
                       unsigned char *start_raw);

/* replaces TrackerAndScaler::trackNewestCoarse (TrackerAndScaler.cpp:451-638).
 * min_res_for_abort / last_residuals: DSM_MAX_LEVELS doubles (reference: Vec5; NaN = no limit).
 * flow_out = lastFlowIndicators.  *good = the reference's bool return value. */
int dsm_tracker_track(dsm_tracker *t, double pose_io[7], double aff_io[2], int coarsest_lvl,
                      const double *min_res_for_abort, double *last_residuals, double flow_out[3],
                      int *good);
/* replaces TrackerAndScaler::optimizeScale (TrackerAndScaler.cpp:854-964); err_out = return value */
int dsm_tracker_optimize_scale(dsm_tracker *t, float *scale_io, int coarsest_lvl, float *err_out);
/* replaces the untrapped branch of FrontEnd::optimizeScale (FrontEnd.cpp:995-1003): optimizeScale from each of n_guesses
 * initial scales (the reference's list: 0.1, 1, 5, 10, 15, 25, 30, 50) as ONE batched call on the tracker's template and right
 * frame; *scale_out / *err_out = the result with the smallest positive error (the first one on ties; 1.0 / -1 when none is
 * positive), scales_all / errs_all (may be NULL) = every guess's result in order. */
int dsm_tracker_optimize_scale_guesses(dsm_tracker *t, int n_guesses, const float *scale_guesses, int coarsest_lvl,
                                       float *scale_out, float *err_out, float *scales_all, float *errs_all);
/* One step of many sequences in ONE call: trackNewestCoarse for the n trackers of `trackers` (arguments as dsm_track_batch) and
 * optimizeScale for the n_scale trackers of `scale_trackers` (arguments as dsm_optimize_scale_batch; a tracker may appear in
 * both lists -- a keyframe's tracker is tracked against AND scale-optimised, FrontEnd.cpp:204-206,992-998).  The two sets are
 * independent problems; the scale problems' launches run on a stream of their own under the tracking kernels.  Results are
 * bit-identical to the two separate calls.  Statistics: dsm_context_get_stats (tracking) / dsm_context_get_stats2 (scale). */
int dsm_track_and_scale_batch(dsm_context *ctx, int n, dsm_tracker *const *trackers, double *pose_io, double *aff_io, int coarsest_lvl,
                              const double *min_res_for_abort, double *last_residuals, double *flow_out, int *good, int n_scale,
                              dsm_tracker *const *scale_trackers, float *scale_io, float *err_out);
int dsm_context_get_stats2(dsm_context *ctx, dsm_stats *out);

/* ---- streaming form of the batched calls: continuous admission ------------------------------
 * dsm_track_and_scale_batch takes every problem of a batch from its first evaluation to its last before it returns, so
 * its lock-step launches run as many rounds per level as the SLOWEST problem needs.  The per-frame chain
 * (TrackerAndScaler.cpp:505-593) is sequential, frames of different sequences are independent (FrontEnd.cpp:585-686):
 * nothing requires them to start and end together.  A dsm_stream is a pool of resident problems (slots) advanced in
 * PASSES: one pass sweeps the pyramid once, coarsest level first, with the rounds per level that MOST problems need (a
 * quantile of what recently retired problems took); a problem that needs more rounds at a level simply stays there
 * (its state is device-resident and resumable) and rides with the next pass's launches at that level; problems retire
 * individually and their slots are refilled from the waiting queue.  One state read-back per pass, none inside it.
 * Results are bit-identical to the batch calls (same evaluations, steps and summation order per problem).
 *   submit_* queue problems (host copies are taken; the trackers' templates and frames must stay untouched until the
 *   problem's result has been returned; the same tracker may be resident several times -- it is only read);
 *   advance  admits waiting problems into free slots, runs one pass, retires what finished (synchronous);
 *   results  hands back retired problems in retirement order;  drain = advance until nothing is resident or waiting. */
typedef struct dsm_stream dsm_stream;
typedef struct dsm_stream_result {
  uint64_t ticket;   /* from dsm_stream_submit_* */
  int kind;          /* 0 trackNewestCoarse, 1 optimizeScale */
  int good;          /* track: the reference's bool return value; scale: 1 */
  int status;        /* raw end state: 2 good, 3 aborted (:598), 4 implausible affine parameters (:615-626) */
  int passes;        /* passes the problem was resident for */
  double pose[7];    /* track: lastToNew_out as dsm_track_batch leaves pose_io (the initial guess after an abort) */
  double aff[2];     /* track: aff_g2l_out, likewise */
  double last_residuals[DSM_MAX_LEVELS];
  double flow[3];    /* track: lastFlowIndicators */
  float scale, err;  /* scale: optimizeScale's scale (:954) and return value (:963) */
  int64_t evals[DSM_MAX_LEVELS]; /* evaluations executed per level (equal to the batch form's) */
} dsm_stream_result;
int dsm_stream_create(dsm_context *ctx, int track_slots, int scale_slots, dsm_stream **out);
int dsm_stream_destroy(dsm_stream *s);
/* arguments as dsm_track_batch / dsm_optimize_scale_batch; tickets_out (may be NULL): n tickets */
int dsm_stream_submit_track(dsm_stream *s, int n, dsm_tracker *const *trackers, const double *pose0, const double *aff0,
                            int coarsest_lvl, const double *min_res_for_abort, uint64_t *tickets_out);
int dsm_stream_submit_scale(dsm_stream *s, int n, dsm_tracker *const *trackers, const float *scale0, int coarsest_lvl,
                            uint64_t *tickets_out);
/* One advance.  Tick engine: PIPELINED by default -- the call returns once the advance is enqueued and reads back the PREVIOUS one
 * (whose kernels ran while the host prepared this one), so results surface one advance late and the device never waits for the
 * host; dsm_stream_sync waits for everything in flight and reads it back (dsm_stream_drain does so itself);
 * dsm_stream_set_pipelined(s, 0) makes every advance synchronous.  Pass engine: synchronous. */
int dsm_stream_advance(dsm_stream *s);
int dsm_stream_sync(dsm_stream *s);
int dsm_stream_set_pipelined(dsm_stream *s, int on);
int dsm_stream_drain(dsm_stream *s);
int dsm_stream_results(dsm_stream *s, int max_results, dsm_stream_result *out, int *n_out);
/* as of the last read-back: problems in a slot / waiting (on the host or in the device's waiting ring) / results ready */
int dsm_stream_counts(dsm_stream *s, int *resident_out, int *waiting_out, int *results_out);
/* The engine behind advance (set before the first advance / while nothing is resident):
 *   0  PASSES: one sweep down the pyramid per advance with a bounded number of lock-step rounds per level (below); problems
 *      that need more are carried over to the next pass;
 *   1  TICKS: every resident problem advances ONE LM round per tick whatever level it stands on -- one evaluation launch over
 *      a device-built list of (problem, chunk) items of all levels mixed, one LM launch that steps the problems, stages the
 *      next tick's items, retires finished problems and refills their slots from the waiting list ON THE DEVICE; an advance
 *      runs ticks_per_advance ticks with one host read-back at its end (0: keep what is in force; -1: back to the stream's own
 *      choice).  Until a number is named the stream sizes every advance itself: the ticks that retire 7/8 of what the advance hands over, from the mean life (in
 *      ticks) of the problems retired so far -- the rest stays in the device's waiting ring as the buffer a freed slot is
 *      refilled from (32 until the first problems have retired; with dsm_params.fixed_schedule: one cohort's whole life).
 *      The default.
 * Both are scheduling only: results are bit-identical to the batch calls. */
int dsm_stream_set_engine(dsm_stream *s, int engine, int ticks_per_advance);
/* Tick engine, CHAINS (round 6): a problem whose pending evaluation is ONE chunk (a pyramid level of at most 4096 template points under
 * the default chunk table: every level of a semi-dense template but the finest one or two; the two coarsest levels of the metric's
 * dense pyramid) needs no other workgroup for its LM round, so the workgroup that evaluates the chunk also steps the problem -- state
 * and descriptor in LDS, the partial never leaves it -- and runs the NEXT round too, up to max_rounds rounds inside one tick, for as long
 * as the staged evaluation stays one chunk.  That is the reference's LM loop (TrackerAndScaler.cpp:505-593) running in place on the
 * levels where it is a chain of tiny steps: such a frame lives a third of the ticks.
 *   max_rounds > 0  every problem with a one-chunk evaluation chains, up to that many rounds per tick;
 *   max_rounds 0    off: every round costs a tick;
 *   max_rounds -1   the default: DSM_STREAM_CHAIN_DEFAULT rounds, for problems whose level-0 template has at most
 *                   DSM_STREAM_CHAIN_DEFAULT_MAX_N0 points.  Measured: semi-dense templates (10 k points) + 31-33 %
 *                   frames/s; dense templates gain nothing (their ticks wait for level 0's items, and a chain that runs longer than
 *                   those makes every other resident problem wait), hence the rule.
 * Scheduling only: same chunk, same partial, same reduction order -- results are bit-identical (tests/test_stream.py).  May be changed
 * between advances. */
#define DSM_STREAM_CHAIN_DEFAULT 8
#define DSM_STREAM_CHAIN_DEFAULT_MAX_N0 65536 /* the default applies to problems whose level-0 template has at most this many points */
int dsm_stream_set_chain(dsm_stream *s, int max_rounds);
/* rounds per level of a pass = this quantile (default 0.75) of the rounds recently retired problems needed there;
 * lvl < 0: every level */
int dsm_stream_set_quantile(dsm_stream *s, int lvl, double q);
/* ... or fixed: rounds_per_level[DSM_MAX_LEVELS] for problems of `mode` (0 track, 1 scale); entries <= 0 / NULL = learnt */
int dsm_stream_set_rounds(dsm_stream *s, int mode, const int *rounds_per_level);
/* CUMULATIVE statistics of the stream as of the last read-back (evaluations staged, algorithmic bytes of the problems retired,
 * launches = rounds / ticks per level, device time of the advances, per-dispatch timing as dsm_context_set_timing): callers difference them */
int dsm_stream_get_stats(dsm_stream *s, dsm_stats *track_out, dsm_stats *scale_out);
/* the schedule in force and the stream's counters: passes run, problems retired (of `mode`), slot-passes spent carrying */
int dsm_stream_get_schedule(dsm_stream *s, int mode, int *rounds_out, long long *passes_out, long long *retired_out, long long *carried_out);

/* ---- hypothesis groups: the loop of FrontEnd::trackNewCoarse (FrontEnd.cpp:194-256) as ONE stream submission ----------------
 * The reference tracks a new frame from a list of pose guesses (constant motion first, then 82-108 others, FrontEnd.cpp:132-192): try i
 * runs trackNewestCoarse with minResForAbort = the best residuals of tries 0..i-1 (aborting at :598 when a level is 1.5x worse), a good
 * try with a lower level-0 residual takes over (:225-243), and the loop stops at the first take-over below last_coarse_rmse0 *
 * retrack_threshold (:245-247).  A level's LM result does not depend on minResForAbort, so the loop is reproduced exactly from tries
 * run WITHOUT abort: dsm_hypotheses_resolve replays the aborts and the take-over / stop rules from their outputs, in try order.
 * A group is scheduling only -- its result equals dsm_host::trackHypotheses (try 0 alone, then the rest as one dsm_track_batch):
 *   try 0 enters the stream as an ordinary track problem without abort thresholds (its ticket is internal: it never appears in
 *   dsm_stream_results); when it is read back and does not settle the frame, tries 1.. are queued in try order, at most `window` of them
 *   waiting or resident at once (dsm_stream_set_hypothesis_window); every retirement feeds the resolver as far as the tries retired IN
 *   ORDER reach, and refills the window.  Once the loop is decided, tries still waiting on the host are dropped, tries already on the
 *   device run to their end and are discarded, and the group's result is handed back when none of its tries is on the device any more.
 * The frame must be resident in the tracker's DSM_SLOT_NEW_LEFT slot (as for dsm_stream_submit_track) and stay untouched, like the
 * tracker's template, until the group's result is back.  Group tries count as track problems in dsm_stream_counts; dsm_stream_drain
 * returns when every group is resolved.  Both engines.  The group is expanded when try 0 is read back on the host: with pipelined
 * advances a frame that needs retries costs one or two advances more than one that does not. */
typedef struct dsm_stream_hyp_result {
  uint64_t ticket;                    /* from dsm_stream_submit_hypotheses */
  int have_one_good;                  /* haveOneGood (FrontEnd.cpp:227-233) */
  int tries_used;                     /* tries the reference's sequential loop runs (tryIterations, :208) */
  int tries_run;                      /* tries the stream ran (>= tries_used; = tries_used with window 1) */
  int advances;                       /* advances issued while the group was pending */
  double pose[7];                     /* lastF_2_fh (tries[0] when no try was good, :249-256) */
  double aff[2];                      /* aff_g2l (aff_last when no try was good) */
  double flow[3];                     /* flowVecs (0 when no try was good) */
  double achieved_res[DSM_MAX_LEVELS];/* achievedRes -- what the caller keeps as last_coarse_rmse_ (:258); [5] stays NaN (a Vec5) */
  int64_t evals[DSM_MAX_LEVELS];      /* evaluations per level, summed over the tries run */
} dsm_stream_hyp_result;
/* tries: n_tries x 7 (pose layout of dsm_stream_submit_track), aff_last[2]: the affine guess of every try; coarsest_lvl as there;
 * last_coarse_rmse0 = last_coarse_rmse_[0], retrack_threshold = setting_reTrackThreshold (1.5).  DSM_ERR_INVALID for n_tries < 1,
 * a NULL pointer or a stream without track slots. */
int dsm_stream_submit_hypotheses(dsm_stream *s, dsm_tracker *tracker, int n_tries, const double *tries, const double aff_last[2],
                                 int coarsest_lvl, double last_coarse_rmse0, double retrack_threshold, uint64_t *ticket_out);
/* resolved groups in resolution order (at most max_results) */
int dsm_stream_hypotheses_results(dsm_stream *s, int max_results, dsm_stream_hyp_result *out, int *n_out);
/* groups not resolved yet / resolved and not yet returned (either pointer may be NULL) */
int dsm_stream_hypotheses_counts(dsm_stream *s, int *pending_out, int *ready_out);
/* the most tries of one group waiting or resident at once after try 0: 0 (default) = all of them (the work of dsm_host::trackHypotheses'
 * batch), 1 = one by one as the reference runs them.  Scheduling only: a group's result does not depend on it.  Applies from the next refill. */
int dsm_stream_set_hypothesis_window(dsm_stream *s, int window);
/* HOST function (no device call): the loop of FrontEnd.cpp:194-256 replayed from the outputs of tries 0 .. k-1 run WITHOUT abort, in try
 * order -- good[k], pose[k x 7], aff[k x 2] (as dsm_track_batch leaves pose_io / aff_io), last_residuals[k x DSM_MAX_LEVELS], flow[k x 3].
 * Try i's abort (TrackerAndScaler.cpp:598) is replayed from its residuals against the achievedRes of tries 0 .. i-1.  *decided_out = 1
 * when the loop ends within these k tries; out then holds its result (ticket, tries_run = k, advances and evals zero).  Otherwise out
 * holds the loop's state after k tries, tries_used = k. */
int dsm_hypotheses_resolve(int n_tries, const double *tries, const double aff_last[2], int coarsest_lvl, double last_coarse_rmse0,
                           double retrack_threshold, int k, const int *good, const double *pose, const double *aff,
                           const double *last_residuals, const double *flow, dsm_stream_hyp_result *out, int *decided_out);

/* Batched forms: n independent trackers of one context advance in lock-step launches
 * (SURVEY.md section 7 "throughput mode").  Arrays are n x 7 / n x 2 / n x DSM_MAX_LEVELS / n x 3. */
int dsm_track_batch(dsm_context *ctx, int n, dsm_tracker *const *ts, double *pose_io, double *aff_io,
                    int coarsest_lvl, const double *min_res_for_abort, double *last_residuals,
                    double *flow_out, int *good);
int dsm_optimize_scale_batch(dsm_context *ctx, int n, dsm_tracker *const *ts, float *scale_io,
                             int coarsest_lvl, float *err_out);

/* outputs the reference exposes as public members (TrackerAndScaler.h:59-64) */
int dsm_tracker_ref_frame_id(dsm_tracker *t);

/* Geometry of the device reduction for level lvl with n template points (tests / DESIGN.md):
 * threads per workgroup, points per thread, number of chunks. */
int dsm_reduction_geometry(dsm_tracker *t, int lvl, int n, int *threads, int *pts_per_thread,
                           int *chunks);

/* ---- loop-closure pose estimation ("next" row N2) ------------------------------------- */
/* replaces PoseEstimator::PoseEstimator(w,h) / ~PoseEstimator (PoseEstimator.cpp:41-60) */
int dsm_pose_estimator_create(dsm_context *ctx, int w, int h, int nlevels, const dsm_params *params,
                              dsm_pose_estimator **out);
int dsm_pose_estimator_destroy(dsm_pose_estimator *pe);
/* replaces PoseEstimator::estimate (PoseEstimator.h:42, PoseEstimator.cpp:298-506): direct alignment of a
 * matched keyframe's 3-D points (xyz: n x 3 doubles in the matched frame, ref_colors[lvl][i] = the
 * per-level reference intensities of LoopFrame::pts_dso, LoopHandler.cpp:172-180) into the current
 * keyframe's pyramid new_dIp with intrinsics new_cam = {fx,fy,cx,cy}.  ref_to_new_io: row-major 4x4,
 * initial guess in, result out (always written, as at :466).  *ok = aff_good && pose_error < RES_THRES(10)
 * && inlier_percent > INNER_PERCENT(90)  (:469-505). */
int dsm_pose_estimator_estimate(dsm_pose_estimator *pe, int n_pts, const double *xyz,
                                const float *const *ref_colors, float ref_ab_exposure,
                                const float *const *new_dIp, float new_ab_exposure, const float new_cam[4],
                                int coarsest_lvl, double ref_to_new_io[16], float *pose_error, int *ok);

/* PoseEstimator::estimate of MANY matches in one call (the call site LoopHandler.cpp:274-279 of every sequence a node serves, between
 * dsm_loop_detect_batch_many and dsm_icp_batch).  A dsm_pose_batch serves one geometry (w, h, nlevels) and one dsm_params; intrinsics,
 * exposures, point counts and guesses differ per job.  Per job the result -- matrix, pose_error, ok -- equals
 * dsm_pose_estimator_estimate of that job on a handle of the same w, h, nlevels and params bit for bit, whatever the batch size and the
 * job's place in it.
 *   - Footprint: the templates live in an arena of 16 bytes x (n_pts + slack) x nlevels per job (NOT w*h per level), the targets in one
 *     intensity plane per level and distinct target pyramid (jobs that pass the same level pointers share the planes).  The arenas grow
 *     on demand and are kept: a repeated call of the same shape allocates nothing.
 *   - Submission: one page-locked staging buffer with every job's points, colours, pack table and device descriptor goes to the device in
 *     one copy (xyz / ref_colors arrays that lie in page-locked memory -- dsm_host_alloc -- are read in place instead); one pack launch
 *     builds every template of every level; new_dIp pyramids are imported in waves of 8 jobs through a bounded staging buffer, one launch
 *     per wave; new_I planes are copied straight to their place; then ONE mode-2 LM run over all jobs (every scheduling form of
 *     dsm_params applies) and one read-back.  Host synchronisations: those of the LM run (one per pass), independent of n_jobs.
 *   - Validation is all or nothing, before any output is written or anything is enqueued: DSM_ERR_INVALID for a NULL pointer,
 *     n_jobs < 1, n_pts < 1 or > w*h, both or neither of new_dIp / new_I, a NULL level pointer, a non-finite guess or coarsest_lvl out
 *     of range.  With dsm_params.frame_check a new_dIp whose gradient channels are not makeImages' fails the call with DSM_ERR_INVALID
 *     naming the job, the level and the texel (as dsm_tracker_upload_frame), and no job's outputs are written. */
typedef struct dsm_pose_batch dsm_pose_batch;
typedef struct dsm_pose_job {
  int n_pts;
  const double *xyz;              /* n_pts x 3, the matched keyframe's points (LoopFrame::pts_dso) */
  const float *const *ref_colors; /* [lvl][n_pts] */
  float ref_ab_exposure;
  const float *const *new_dIp;    /* the current keyframe's AoS (I,dx,dy) pyramid, as dsm_pose_estimator_estimate, or NULL */
  const float *const *new_I;      /* ... or its intensity planes per level, as dsm_tracker_upload_intensity; exactly one of the two */
  float new_ab_exposure;
  float new_cam[4];               /* per job: makeK(new_cam), PoseEstimator.cpp:306 */
  double *ref_to_new_io;          /* row-major 4x4: guess in, result out (always written, :466) */
  float *pose_error;              /* out, may be NULL */
  int *inlier_percent;            /* out, may be NULL (:486) */
  int *ok;                        /* out: aff_good && pose_error < RES_THRES && inlier_percent > INNER_PERCENT (:469-505) */
} dsm_pose_job;
int dsm_pose_batch_create(dsm_context *ctx, int w, int h, int nlevels, const dsm_params *params, dsm_pose_batch **out);
int dsm_pose_batch_destroy(dsm_pose_batch *pb);
int dsm_pose_estimate_batch(dsm_pose_batch *pb, int n_jobs, const dsm_pose_job *jobs, int coarsest_lvl);

/* ---- ring-key database (ScanContext place recognition) ------------------------------- */
/* replaces the flann::Index built at LoopHandler.cpp:35-39 plus the function-static delay
 * queue of search_ringkey (search_place.h:43-45).  dim=20, margin=LOOP_MARGIN=100,
 * k=FLANN_NN=3, thres=RINGKEY_THRES=0.1 in the reference.  dummy_key (dim floats, may be
 * NULL = zeros) is the content of the reference's uninitialised index slot 0 (quirk Q8).
 * capacity = number of keys the device shard can hold (grows by doubling when exceeded).
 * shard_rank / shard_count: this handle stores only ordinals with ordinal % count == rank. */
int dsm_ringdb_create(dsm_context *ctx, int dim, int margin, int k, float thres,
                      const float *dummy_key, int64_t capacity, int shard_rank, int shard_count,
                      dsm_ringdb **out);
int dsm_ringdb_destroy(dsm_ringdb *db);
/* number of entries in the (global) index, dummy included (flann Index::size()) */
int64_t dsm_ringdb_size(dsm_ringdb *db);
/* replaces search_ringkey (search_place.h:25-57): query, threshold, then delay-queue insert.
 * cand_out[k] receives 0..k candidate ordinals (index-1) in ascending-distance order.
 * On a sharded handle this is a COLLECTIVE call (the call site LoopHandler.cpp:247 runs once per rank with the same
 * key): needs dsm_ringdb_attach_comm; every rank scans its shard, the candidates are merged by RCCL all-reduce(min)
 * and every rank returns the same list.  Without a communicator a sharded handle fails with DSM_ERR_STATE. */
int dsm_ringdb_query_then_enqueue(dsm_ringdb *db, const float *key, int *cand_out, int *ncand_out);
/* search_ringkey (search_place.h:25-57) of n sequences in ONE call, each against its own index: equal, bit for bit, to
 * dsm_ringdb_query_then_enqueue(dbs[j], keys + j*dim, cand_out + j*k, ncand_out + j) for j = 0 .. n-1 in that order -- candidates,
 * counts, and every index's entries, size and delay queue afterwards.  An index may appear several times (two keyframes of one
 * sequence in the same advance), at most `margin` times per call; query j of an index sees the keys that earlier jobs of the call
 * moved out of that index's delay queue.  All indexes: one context, unsharded, the same dim and k (thres and margin may differ).
 * All or nothing: a NULL argument, n < 1, a mixed context, a sharded index, a dim / k mismatch or too many jobs on one index fail
 * with DSM_ERR_INVALID before any output is written, any key is enqueued or any index changes.  One host synchronisation. */
int dsm_ringdb_query_then_enqueue_many(int n, dsm_ringdb *const *dbs, const float *keys, int *cand_out, int *ncand_out);
/* bulk insert (bench / sharded DB): n_keys keys appended directly to the index */
int dsm_ringdb_add_points(dsm_ringdb *db, const float *keys, int64_t n_keys);
/* the delay-queue half of search_ringkey alone (search_place.h:41-56): used by sharded callers
 * that merge candidates across GPUs between the query and the insert */
int dsm_ringdb_enqueue(dsm_ringdb *db, const float *key);
/* batched exact k-NN over this shard: for each of nq queries (host pointer, nq x dim) writes k packed
 * candidates  (int64 = float_bits(dist2) << 32 | global index), ascending, into the DEVICE buffer
 * d_packed_out (nq*k int64).  Only entries with dist2 < thres are candidates; empty slots hold
 * DSM_RINGDB_NO_CANDIDATE.  The cross-shard merge is dsm_ringdb_merge_topk below. */
#define DSM_RINGDB_NO_CANDIDATE 0x7FFFFFFFFFFFFFFFll
int dsm_ringdb_knn_packed(dsm_ringdb *db, const float *queries, int nq, void *d_packed_out);
/* same, queries already on the device (nq x dim float32) */
int dsm_ringdb_knn_packed_dev(dsm_ringdb *db, const void *d_queries, int nq, void *d_packed_out);
/* same, result copied to host memory (nq*k int64) */
int dsm_ringdb_knn_packed_host(dsm_ringdb *db, const float *queries, int nq, int64_t *packed_out);
/* Which scan would run?  Host only, launches nothing: the form that a scan of nq queries over the index as it stands takes
 * (many = 0: dsm_ringdb_knn_packed* / dsm_ringdb_query_then_enqueue; many != 0: this index as one of
 * dsm_ringdb_query_then_enqueue_many's, where nq is not used), the number of slices its local entries are cut into and the keys of
 * one slice (the last may hold fewer).  The launches switch on the same rule, so the answer cannot drift from what runs; tests
 * use it to prove that they reach every form, a second key tile (more than 128 keys per slice of a DSM_RINGKEY_FORM_TILE_* scan)
 * and a thread's second iteration (more than 1024 keys per slice of the FEWQ4 / MANY4 forms).  Every form returns the same bits. */
enum {
  DSM_RINGKEY_FORM_FEWQ4_1 = 0,     /* dim 20, 1 query: a thread per four keys */
  DSM_RINGKEY_FORM_FEWQ4_2 = 1,     /* dim 20, 2 queries: a thread per four keys */
  DSM_RINGKEY_FORM_FEWQ_4 = 2,      /* dim 20, 3-4 queries: a thread per key, one query group of four */
  DSM_RINGKEY_FORM_FEWQ_8 = 3,      /* dim 20, 5-32 queries: a thread per key, query groups of eight */
  DSM_RINGKEY_FORM_TILE_1 = 4,      /* dim 20, 33-511 queries: a thread per query, key tiles of 128 through LDS */
  DSM_RINGKEY_FORM_TILE_2 = 5,      /* dim 20, from 512 queries: two queries per thread */
  DSM_RINGKEY_FORM_TILE_ANYDIM = 6, /* any other dimension: a thread per query, flann::L2's tail loop */
  DSM_RINGKEY_FORM_MANY4 = 7,       /* many indexes, dim 20: a thread per four keys */
  DSM_RINGKEY_FORM_MANY_ANYDIM = 8, /* many indexes, any other dimension: a thread per key */
  DSM_RINGKEY_FORM_COUNT = 9
};
int dsm_ringdb_scan_plan(dsm_ringdb *db, int nq, int many, int *form_out, int *n_slices_out, long long *keys_per_slice_out);

/* ---- sharded ring-key database across the GPUs of a node -------- */
/* The index of LoopHandler.cpp:35-39 split `ordinal mod G` over G processes (one per GPU); search_ringkey's k-NN
 * (search_place.h:29-33) becomes a local scan per shard + a cross-shard merge of the packed candidates over xGMI.
 * The communicator wraps an RCCL communicator (librccl.so.1 is loaded at run time, on first use):
 *   rank 0: dsm_comm_unique_id(id) -> the host distributes the 128 bytes to all ranks (its launcher's business: MPI,
 *   a file, a socket; bench.py uses torch.distributed) -> every rank: dsm_comm_create(ctx, id, rank, nranks, &comm). */
#define DSM_COMM_ID_BYTES 128
int dsm_comm_unique_id(unsigned char id_out[DSM_COMM_ID_BYTES]);
int dsm_comm_create(dsm_context *ctx, const unsigned char id[DSM_COMM_ID_BYTES], int rank, int nranks, dsm_comm **out);
int dsm_comm_destroy(dsm_comm *comm);
int dsm_comm_rank(dsm_comm *comm);
int dsm_comm_size(dsm_comm *comm);
/* Cross-shard merge, collective over the communicator: d_packed (DEVICE, nq*k int64) holds this rank's sorted local
 * candidates (dsm_ringdb_knn_packed*) on entry and the global top-k (identical on every rank, ascending) on return.
 * Enqueued on the context's stream; synchronise the context before reading the buffer from the host.
 * algo: DSM_MERGE_ALLREDUCE_MIN = k rounds of ncclAllReduce(ncclMin, ncclUint64) with winner pop (8*nq bytes per round);
 *       DSM_MERGE_ALLGATHER     = one ncclAllGather of every rank's nq*k candidates + local k-way merge.  Same result. */
enum { DSM_MERGE_ALLREDUCE_MIN = 0, DSM_MERGE_ALLGATHER = 1 };
int dsm_ringdb_merge_topk(dsm_ringdb *db, dsm_comm *comm, void *d_packed, int nq, int algo);
/* the same merge over a caller-supplied transport (hosts that do not use RCCL; tests that run the ranks as threads or
 * gloo processes): the callbacks run the collective on DEVICE buffers, in order, on `hip_stream`, and return 0 on success.
 * allreduce_min: element-wise unsigned 64-bit min over the ranks, in place.  allgather: recv[r*count .. ] = rank r's send. */
typedef int (*dsm_allreduce_min_u64_fn)(void *user, void *d_buf, size_t count, void *hip_stream);
typedef int (*dsm_allgather_u64_fn)(void *user, const void *d_send, void *d_recv, size_t count, void *hip_stream);
int dsm_ringdb_merge_topk_with(dsm_ringdb *db, void *d_packed, int nq, int algo, int nranks,
                               dsm_allreduce_min_u64_fn allreduce_min, dsm_allgather_u64_fn allgather, void *user);
/* attach (or, with NULL, detach) the communicator dsm_ringdb_query_then_enqueue uses on a sharded handle.  Borrowed:
 * dsm_comm_destroy detaches it from every database it is attached to (a later collective query on such a database fails
 * with DSM_ERR_STATE); destroy communicators before their context.  A collective query starts with an agreement round
 * (one all-reduce word per rank): if any rank cannot take part -- allocation failure, a different number of entries --
 * EVERY rank returns an error and none enters the merge rounds. */
int dsm_ringdb_attach_comm(dsm_ringdb *db, dsm_comm *comm);
/* the same with a caller-supplied transport instead of an RCCL communicator (allreduce_min NULL detaches) */
int dsm_ringdb_attach_transport(dsm_ringdb *db, int nranks, dsm_allreduce_min_u64_fn allreduce_min, dsm_allgather_u64_fn allgather,
                                void *user);

/* replaces ScanContext::generate (src/loop_closure/loop_detection/ScanContext.cpp:78-141, with
 * align_points_PCA :19-66).  Host side by design: a few 10^3 points per
 * keyframe.  pts: n x 3 doubles.  ringkey_out: num_r floats.  sig_idx_out / sig_val_out: capacity
 * num_s*num_r, *n_sig_out entries written (sparse signature, ascending bin index).  tfm_pca_rig_out:
 * row-major 4x4.  Eigenvector signs are not defined by the reference (Eigen's solver); here every
 * eigenvector is oriented so that its largest-magnitude component is positive. */
int dsm_scancontext_generate(const double *pts, int n, double lidar_range, int num_s, int num_r,
                             float *ringkey_out, int *sig_idx_out, double *sig_val_out, int *n_sig_out,
                             double *tfm_pca_rig_out);

/* replaces generate_spherical_points (loop_detection/generate_spherical_points.h:27-85; call site LoopHandler.cpp:186-187) in
 * flat-array form.  kf_pose_wc: n_kf x 6 Sophus tangents (translation, rotation) as in id_pose_wc; cur_cw: row-major 3x4
 * matrix of the current keyframe's camera<-world pose; pt_kf_id / pt_xyz: the nearby points with the keyframe that owns each.
 * Outputs: kf_keep[n_kf] (0: the reference erases that keyframe, :33-41), *n_out selected points, sel_idx (their indices in the
 * input list: the reference's updated pts_nearby) and pts_spherical (n_out x 3, current camera frame).  Per 1 x 0.5 x 1 m voxel the
 * highest point (smallest y) is kept (:64-76).  A point whose norm in the current camera frame is not < lidar_range is dropped: the
 * reference's `>=` test for every finite point, and a non-finite point as well (it never reaches the voxel index).  Order of the output: ascending voxel index -- the reference emits its
 * unordered_map in implementation-defined order.  Host side (tens of thousands of points per keyframe). */
int dsm_generate_spherical_points(int n_kf, const int *kf_ids, const double *kf_pose_wc, const double *cur_cw,
                                  double lidar_range, int n_pts, const int *pt_kf_id, const double *pt_xyz, int *kf_keep,
                                  int *n_out, int *sel_idx, double *pts_spherical);

/* DEVICE form of the pair generate_spherical_points + ScanContext::generate (the two calls a marginalised keyframe makes on its
 * way to the ring-key search: LoopHandler.cpp:186-187 and ScanContext.cpp:78-141 via LoopHandler.cpp:240-245), batched over
 * n_jobs keyframes -- of one sequence or of several concurrent sequences sharing the GPU (BASELINE configs[4]); the jobs are
 * independent.  Per job the inputs are those of
 * dsm_generate_spherical_points; outputs: kf_keep, *n_out, sel_idx, pts_spherical as there, and -- when ringkey is not NULL --
 * ringkey[num_r], the sparse signature (sig_idx / sig_val, capacity num_s*num_r, *n_sig entries) and tfm_pca_rig[16] as
 * dsm_scancontext_generate returns them for pts_spherical.  The voxel "highest point" filter runs as two atomic-min passes
 * over a dense voxel grid plus an ordered compaction, the polar binning as atomic max per bin (csrc/loopdet_kernels.hip); the
 * keyframe trim (a handful of keyframes) and the 3x3 eigen-decomposition stay on the host.  Same results as the two host
 * entry points (bit for bit wherever device and host libm agree on atan2).  lidar_range up to 100 m (dense grid). */
typedef struct dsm_loop_job {
  int n_kf;
  const int *kf_ids;
  const double *kf_pose_wc;   /* n_kf x 6 */
  const double *cur_cw;       /* row-major 3x4 */
  int n_pts;
  const int *pt_kf_id;
  const double *pt_xyz;       /* n_pts x 3.  If pt_kf_id AND pt_xyz of a job lie in page-locked memory (dsm_host_alloc, hipHostMalloc,
                                 hipHostRegister) the device reads them in place -- no host copy of the cloud; pageable clouds are staged
                                 (28 bytes per point copied on the host).  Same results either way. */
  int *kf_keep;               /* out: n_kf */
  int *n_out;                 /* out */
  int *sel_idx;               /* out: capacity n_pts; NULL (together with pts_spherical): the selected points stay on the device */
  double *pts_spherical;      /* out: capacity n_pts x 3 */
  float *ringkey;             /* out: num_r floats, or NULL to stop after the point filter (job by job: one batch may hold both kinds;
                                 a job without is skipped by the ScanContext kernels and none of its five descriptor outputs is written) */
  int *sig_idx;               /* out: capacity num_s*num_r */
  double *sig_val;            /* out: capacity num_s*num_r */
  int *n_sig;                 /* out */
  double *tfm_pca_rig;        /* out: row-major 4x4 */
} dsm_loop_job;
int dsm_loop_descriptors_batch(dsm_context *ctx, int n_jobs, const dsm_loop_job *jobs, double lidar_range, int num_s, int num_r);
/* The per-keyframe loop chain -- generate_spherical_points (LoopHandler.cpp:186), ScanContext::generate (:236), search_ringkey (:247,
 * search_place.h:25-57) -- as ONE enqueue and ONE read-back for keyframes of ONE index (n_jobs <= its margin): the ring keys go from
 * the descriptor kernels to the index's k-NN on the device.  One index is one sequence's search (LoopHandler.cpp:35-39): every job
 * searches, and is enqueued into, the same index and delay queue.  Keyframes of several concurrent sequences, each with its own index,
 * go through dsm_loop_detect_batch_many below.  Every job
 * needs its descriptor outputs (ringkey ... tfm_pca_rig); sel_idx / pts_spherical may both be NULL (the selected points -- 0.45 MB per
 * keyframe -- then stay on the device).  Results equal the jobs' dsm_loop_descriptors_batch + dsm_ringdb_query_then_enqueue calls one
 * after the other, bit for bit: cand_out[j * k ...] / ncand_out[j] = search_ringkey's candidate list of job j, and every key is enqueued.
 * Unsharded index; num_r = its key dimension.
 * Errors are all-or-nothing: a job whose filtered cloud is empty while a descriptor is asked for fails the call with DSM_ERR_INVALID
 * BEFORE any output array of any job is written and before any key is enqueued (dsm_loop_descriptors_batch likewise writes nothing). */
int dsm_loop_detect_batch(dsm_context *ctx, dsm_ringdb *db, int n_jobs, const dsm_loop_job *jobs, double lidar_range, int num_s, int num_r,
                          int *cand_out, int *ncand_out);
/* dsm_loop_detect_batch with one index PER JOB (dbs[j]: the index of job j's sequence): equal to, per job in order,
 * dsm_loop_descriptors_batch of that job followed by dsm_ringdb_query_then_enqueue(dbs[j], its ring key, ...).  The indexes follow the
 * rules of dsm_ringdb_query_then_enqueue_many (the call's context, unsharded, dim = num_r, one k, at most `margin` jobs per index);
 * every job needs its descriptor outputs.  All or nothing as both calls: on any invalid argument or a job whose filtered cloud is empty,
 * DSM_ERR_INVALID before any output is written, any key is enqueued or any index changes.  One read-back, one synchronisation. */
int dsm_loop_detect_batch_many(dsm_context *ctx, int n_jobs, const dsm_loop_job *jobs, dsm_ringdb *const *dbs, double lidar_range, int num_s,
                               int num_r, int *cand_out, int *ncand_out);

/* The ICP fallback of loop closure: replaces icp() (src/loop_closure/pose_estimation/icp.h:44-71), which LoopHandler::run calls when direct
 * alignment rejects a ScanContext match (LoopHandler.cpp:284-288) -- PCL's IterativeClosestPoint<PointXYZ, PointXYZ> with the settings of
 * icp.h:58-61 -- batched over independent matches (of one sequence or of several).  Semantics: DESIGN.md section 10, quirks P1-P9 and
 * deviations D1-D5; in short, per job:
 *   - the source (matched keyframe's pts_spherical) is moved by the guess tfm_target_source in double and rounded to float, the target
 *     (current keyframe's pts_spherical) rounded to float;
 *   - up to max_iterations rounds of: exact nearest target of every source point, pairs kept within max_corr_dist, Umeyama (no scale)
 *     increment, the convergence tests of PCL's DefaultConvergenceCriteria; fewer than 3 pairs end the loop (NO_CORRESPONDENCES);
 *   - tfm_target_source = double(final) * tfm_target_source; score = getFitnessScore() (the guess-moved source moved by the final
 *     transformation, mean squared nearest-neighbour distance, no limit); ok = score < score_thres;
 *   - an empty source or target (D3) leaves tfm_target_source unchanged: score = +inf, ok = 0, iterations = 0, state = EMPTY.
 * The RANSAC threshold of icp.h:61 has no effect in PCL (no rejector is installed): it is not a parameter (P7).
 * One launch sequence and one read-back for the whole batch; a job's results do not depend on the other jobs of the call.  Points are
 * expected finite; they are not validated, and D5 says what a non-finite coordinate does.  Validation is all or nothing, before any
 * output is written: DSM_ERR_INVALID for NULL pointers, negative sizes or more than DSM_ICP_MAX_POINTS points, max_iterations outside
 * [1, DSM_ICP_ITERATIONS_LIMIT], a non-finite or negative max_corr_dist, a non-finite transformation_epsilon, a NaN score_thres or a
 * non-finite guess.  The steady state allocates nothing (the loop chain's device arena and page-locked mirror of the context). */
#define DSM_ICP_MAX_ITERATIONS 5                /* icp.h:58 setMaximumIterations */
#define DSM_ICP_TRANSFORMATION_EPSILON 0.01     /* icp.h:59 setTransformationEpsilon */
#define DSM_ICP_MAX_CORRESPONDENCE_DISTANCE 2.0 /* icp.h:60 setMaxCorrespondenceDistance */
#define DSM_ICP_RANSAC_THRESHOLD 0.5            /* icp.h:61 setRANSACOutlierRejectionThreshold: no effect (P7), not used */
#define DSM_ICP_THRES 1.5                       /* icp.h:20 ICP_THRES: a match is accepted iff score < it */
#define DSM_ICP_ITERATIONS_LIMIT 64             /* largest max_iterations accepted */
#define DSM_ICP_MAX_POINTS (1 << 24)            /* largest cloud accepted */
/* end states (dsm_icp_job.state): PCL's ConvergenceState values; 4 (relative MSE) is never reached (P6), 6 is D3 */
#define DSM_ICP_STATE_NOT_CONVERGED 0
#define DSM_ICP_STATE_ITERATIONS 1
#define DSM_ICP_STATE_TRANSFORM 2
#define DSM_ICP_STATE_ABS_MSE 3
#define DSM_ICP_STATE_NO_CORRESPONDENCES 5
#define DSM_ICP_STATE_EMPTY 6
typedef struct dsm_icp_job {
  int n_src;                 /* pts_source: the matched keyframe's pts_spherical */
  const double *src_xyz;     /* n_src x 3 */
  int n_tgt;                 /* pts_target: the current keyframe's pts_spherical */
  const double *tgt_xyz;     /* n_tgt x 3 */
  double *tfm_target_source; /* in: the guess (LoopHandler.cpp:266-268), out: the ICP result; row-major 4x4 */
  float *score;              /* out: icp_score */
  int *ok;                   /* out: icp()'s return value */
  int *iterations;           /* out: iterations run (increments applied) */
  int *state;                /* out: DSM_ICP_STATE_* */
  int *corr_counts;          /* out, optional (NULL): capacity max_iterations; the pairs kept by each correspondence search in order,
                                -1 past the last search (the last one is the failing search of a NO_CORRESPONDENCES end) */
} dsm_icp_job;
int dsm_icp_batch(dsm_context *ctx, int n_jobs, dsm_icp_job *jobs, int max_iterations, double transformation_epsilon, double max_corr_dist,
                  double score_thres);

/* test aid (no reference counterpart): dsm_icp_batch's own launch sequence -- the same block table, arena layout, staging and kernels,
 * one function serves both -- stopped after a stage, with what the device holds there copied out.  Stages in launch order:
 * prep (P1); search and step (P2; P3-P6) of iteration stop_iteration (0-based, < max_iterations); fitness prep, fitness search and
 * fitness (P9); DSM_ICP_STAGE_FITNESS is the whole sequence.  A batch none of whose jobs has points runs the prep alone.
 * want_slices: the number of target slices a job's search is cut into (at least one 256-point tile each, so at most that many
 * tiles); 0 = the production rule (about 2048 workgroups per call), under which the states after DSM_ICP_STAGE_FITNESS are bit for bit
 * what dsm_icp_batch unpacks.  Of a job only the inputs are read (n_src, src_xyz, n_tgt, tgt_xyz, tfm_target_source); nothing of it is
 * written.  Outputs, each optional (NULL), the jobs back to back in call order: orig / work (the guess-moved source and the working
 * cloud) and target as float x, y, z, 0 per point; keys, one per source point: (float bits of dist2 << 32) | target index,
 * DSM_ICP_NO_KEY where the point has no neighbour (yet); states, one per job.  DSM_ERR_INVALID with nothing written for what
 * dsm_icp_batch refuses of these arguments, want_slices < 0, an unknown stage or an iteration outside [0, max_iterations).
 * No production path calls this. */
#define DSM_ICP_STAGE_PREP 0
#define DSM_ICP_STAGE_SEARCH 1
#define DSM_ICP_STAGE_STEP 2
#define DSM_ICP_STAGE_FITNESS_PREP 3
#define DSM_ICP_STAGE_FITNESS_SEARCH 4
#define DSM_ICP_STAGE_FITNESS 5
#define DSM_ICP_NO_KEY 0xFFFFFFFFFFFFFFFFull
typedef struct dsm_icp_state {  /* what the device keeps per job between the launches of a call */
  float final_tf[16];           /* PCL's final_transformation_, row-major */
  double prev_mse;              /* mean dist2 of the last iteration that went on (DBL_MAX before the first) */
  double fitness;               /* getFitnessScore() before its cast to float (+inf until the fitness stage) */
  int state;                    /* DSM_ICP_STATE_*, 0 while iterating */
  int iterations;               /* increments applied */
  int searches;                 /* correspondence searches evaluated: iterations, plus the one that found fewer than 3 pairs */
  int pad;
  int corr[DSM_ICP_ITERATIONS_LIMIT]; /* pairs kept by each search, -1 past the last */
} dsm_icp_state;
int dsm_diag_icp_stages(dsm_context *ctx, int n_jobs, const dsm_icp_job *jobs, int max_iterations, double transformation_epsilon,
                        double max_corr_dist, int want_slices, int stop_stage, int stop_iteration, float *orig_xyzw, float *work_xyzw,
                        float *target_xyzw, unsigned long long *keys, dsm_icp_state *states);

/* ---- CoarseDistanceMap and the activation walk -------------------------------------------------------------
 * replaces dso::CoarseDistanceMap (TrackerAndScaler.h:139-170, TrackerAndScaler.cpp:1174-1362) and the distance-map part of
 * FrontEnd::activatePointsMT (FrontEnd.cpp:371-451), for the windows of many sequences in one call.  The map has
 * w1 x h1 = (w >> 1) x (h >> 1) cells (makeK, :1349-1350) holding 0 .. 39 or 1000.  Everything is integer-exact; the float32
 * projection is evaluated as ((m0 u + m1 v) + m2) + kt idepth per component, without contraction. */

/* replaces CoarseDistanceMap(ww, hh) (:1174-1187) and its destructor (:1189-1195); a fresh map holds 1000 everywhere */
int dsm_distmap_create(dsm_context *ctx, int w, int h, dsm_distmap **map_out);
int dsm_distmap_destroy(dsm_distmap *map);
/* reads fwdWarpedIDDistFinal (FrontEnd.cpp:439): w1 * h1 floats, row-major */
int dsm_distmap_get(dsm_distmap *map, float *out);
/* replaces CoarseDistanceMap::addIntoDistFinal (:1326-1332): the cell becomes 0 unconditionally, then growDistBFS(1) (:1235-1324) runs
 * from it on the map as it stands.  DSM_ERR_INVALID outside [0, w1) x [0, h1) (the reference would write out of bounds). */
int dsm_distmap_add(dsm_distmap *map, int u, int v);

/* One window.  hosts: the frames of the window other than the newest, each with KRKi = K[1] R Ki[0] (row-major 3x3) and Kt = K[1] t
 * of host-to-newest (:1212-1214, FrontEnd.cpp:387-392).  seeds: the active points of those frames (ph->u, ph->v, ph->idepth_scaled,
 * :1216-1226).  candidates: the immature points that passed the canActivate filter (FrontEnd.cpp:400-429), in the reference's order,
 * with idepth = 0.5f * (idepth_max + idepth_min) formed by the caller (:433) and type = my_type (:442). */
typedef struct dsm_activation_job {
  dsm_distmap *map;
  int n_hosts;
  const float *krki; /* n_hosts * 9, row-major */
  const float *kt;   /* n_hosts * 3 */
  int n_seeds;
  const int *seed_host;
  const float *seed_u, *seed_v, *seed_idepth;
  int n_cand;
  const int *cand_host;
  const float *cand_u, *cand_v, *cand_idepth, *cand_type;
  float min_act_dist;           /* current_min_act_dist_ (FrontEnd.cpp:442) */
  unsigned char *decision_out;  /* n_cand: 0 keep, 1 activate, 2 out of bounds (the reference deletes the point, :446-449) */
  int *n_activated_out;         /* may be NULL */
} dsm_activation_job;

/* replaces CoarseDistanceMap::makeDistanceMap (:1197-1230) for every job: the map is reset to 1000, every seed whose projection
 * (qu, qv) = (ptp0 / ptp2 + 0.5f, ptp1 / ptp2 + 0.5f) satisfies qu >= 1 && qv >= 1 && qu < w1 && qv < h1 (NaN and +-inf fail) sets
 * cell ((int)qu, (int)qv) to 0, then growDistBFS: level k = 1 .. 39 writes k into the neighbours (8 for odd k, 4 for even k) that
 * hold more than k, and a cell on the map's border is never expanded.  The cand_* fields are ignored. */
int dsm_distmaps_make(dsm_context *ctx, int n_jobs, const dsm_activation_job *jobs);
/* dsm_distmaps_make, then the walk of FrontEnd.cpp:431-449 per job: a candidate outside the bounds above gets decision 2; otherwise
 * dist = map[cell] + (ptp0 - floorf(ptp0)), it is activated (1) iff dist >= min_act_dist * type and then added to the map
 * (dsm_distmap_add) before the next candidate is looked at; otherwise 0.  One launch sequence and one host wait for all jobs; a
 * job's map and decisions do not depend on the other jobs of the call.  One geometry per call (as dsm_set_refs_from_points), a
 * map in one job only, n_seeds == 0 and n_cand == 0 are valid.  Validation is all or nothing, before anything is enqueued:
 * DSM_ERR_INVALID for NULL arrays, negative counts, mixed geometries, a map twice, or a host index outside [0, n_hosts). */
int dsm_activate_points_batch(dsm_context *ctx, int n_jobs, const dsm_activation_job *jobs);
/* The same as one plain sequential loop on the host (the reference's list BFS, :1235-1324): job->map is ignored, (w, h) is the
 * level-0 size, map_out (w1 * h1 floats, may be NULL) receives the final map.  The CPU baseline of tools/activation_timing.py and
 * a checker that needs no device, like dsm_make_coarse_depth_l0 beside the device template builder. */
int dsm_activate_points_host(int w, int h, const dsm_activation_job *job, float *map_out);

/* ---- Optimisation of the selected immature points --------------------------------------------------------------
 * replaces the second half of FrontEnd::activatePointsMT (FrontEnd.cpp:458-468): FrontEnd::optimizeImmaturePoint
 * (dso_helpers/FrontEndOptPoint.cpp:35-138) for every selected point of the windows of many sequences in one call.  Everything is
 * float32 without contraction except the LM step and the convergence test, which are double as in the reference (M3, M5). */
#define DSM_IMMATURE_HUBER_TH 9.0f            /* setting_huberTH */
#define DSM_IMMATURE_MIN_IDEPTH_H_ACT 100.0f  /* setting_minIdepthH_act */
#define DSM_IMMATURE_GN_ITERATIONS 3          /* setting_GNItsOnPointActivation */
#define DSM_IMMATURE_GN_ITERATIONS_LIMIT 16   /* largest gn_iterations accepted */
#define DSM_WINDOW_MAX_FRAMES 16              /* largest capacity of a dsm_window */
#define DSM_IMMATURE_MAX_FRAMES 9             /* largest n_frames of a job: at most 8 residuals per point */
/* residual states (dsm_immature_job.res_state): ResState IN / OOB / OUTLIER, and the mark of the host's own column */
#define DSM_RES_IN 0
#define DSM_RES_OOB 1
#define DSM_RES_OUTLIER 2
#define DSM_RES_HOST 255

/* The keyframe images of one window on the device: level-0 intensity planes only (gradients are formed where they are
 * interpolated), w * h floats per frame, all memory allocated at creation.  capacity in [1, DSM_WINDOW_MAX_FRAMES]. */
int dsm_window_create(dsm_context *ctx, int w, int h, int capacity, dsm_window **win_out);
int dsm_window_destroy(dsm_window *win);
/* a new frame from w * h host intensities (pageable or from dsm_host_alloc, as dsm_tracker_upload_intensity); returns when the
 * caller's buffer is free.  DSM_ERR_INVALID for a frame id already in the store or a full store. */
int dsm_window_put_host(dsm_window *win, int frame_id, const float *I);
/* a new frame as a device-side copy of level 0 of the frame resident in `slot` (DSM_SLOT_NEW_LEFT / _RIGHT) of `owner`: the frame
 * that has just become a keyframe.  DSM_ERR_INVALID as above, for a tracker of another context or geometry, or an empty slot. */
int dsm_window_put_from_tracker(dsm_window *win, int frame_id, dsm_tracker *owner, int slot);
/* marginalisation: the frame's place is free again.  DSM_ERR_INVALID for an id not in the store. */
int dsm_window_drop(dsm_window *win, int frame_id);
/* reads a frame back (w * h floats); for tests */
int dsm_window_get(dsm_window *win, int frame_id, float *out);

/* One window.  frame_ids: frame_hessians_ in order; pre_*: FrameFramePrecalc::PRE_RTll / PRE_tTll / PRE_aff_mode of every
 * [host][target] pair in float32, formed by the caller (the exp of the affine model stays on the host); the diagonal is not read.
 * A point is an ImmaturePoint that dsm_activate_points_batch selected: host (an index into frame_ids), u, v, idepth_min, idepth_max,
 * energyTH, color[8], weights[8]. */
typedef struct dsm_immature_job {
  dsm_window *window;       /* ignored by dsm_optimize_immature_points_host */
  float cam[4];             /* fxl, fyl, cxl, cyl */
  float cam_inv[2];         /* fxli, fyli */
  int n_frames;             /* 1 .. DSM_IMMATURE_MAX_FRAMES */
  const int *frame_ids;     /* n_frames */
  const float *pre_R;       /* n_frames * n_frames * 9, [host][target], row-major 3x3 */
  const float *pre_t;       /* n_frames * n_frames * 3 */
  const float *pre_aff;     /* n_frames * n_frames * 2 */
  int n_pts;
  const int *host;          /* n_pts */
  const float *u, *v, *idepth_min, *idepth_max, *energy_th; /* n_pts each */
  const float *color;       /* n_pts * 8 */
  const float *weights;     /* n_pts * 8 */
  int min_obs;              /* the reference passes 1 (FrontEnd.cpp:336) */
  unsigned char *status;    /* n_pts: 0 = `return 0` (the point stays immature), 1 = activated, 2 = (PointHessian*)-1 (delete the point) */
  float *idepth_out;        /* n_pts: currentIdepth at the exit taken */
  unsigned char *res_state; /* n_pts * n_frames: DSM_RES_* of the residual against each frame at the exit taken, DSM_RES_HOST in the
                               host's own column; the caller builds the PointFrameResiduals and lastResiduals from it (:154-173) */
  float *hdd_out, *bd_out, *energy_out; /* optional (NULL): lastHdd, lastbd, lastEnergy at the exit taken */
  int *iterations_out;      /* optional (NULL): trial evaluations run (0 .. gn_iterations) */
} dsm_immature_job;

/* FrontEndOptPoint.cpp:37-138 for every point of every job, as written down in DESIGN.md section 13 (M1-M8, U1-U9): one staged copy,
 * one launch, one host wait for the whole batch; nothing is allocated once the context's arena has grown to the batch size; a job's
 * results do not depend on the other jobs of the call.  A window may serve several jobs; one geometry per call; n_pts == 0 is valid;
 * a point whose window holds its host frame only has no residuals, Hdd = 0, and gets status 0.  PointHessian's own energyTH
 * finiteness test (:141) reads caller data only and stays with the caller.  Validation is all or nothing, before anything is
 * enqueued: DSM_ERR_INVALID for NULL arrays or negative counts, n_frames outside [1, 9], a host index outside [0, n_frames), a frame
 * id that is not in the window, mixed geometries, gn_iterations outside [0, 16], non-finite huber_th or min_idepth_h_act. */
int dsm_optimize_immature_points_batch(dsm_context *ctx, int n_jobs, const dsm_immature_job *jobs, float huber_th, float min_idepth_h_act,
                                       int gn_iterations);
/* The same for one job as one plain sequential loop on the host: job->window is ignored, frame_I[i] is the w * h level-0 intensity
 * plane of frame_ids[i].  The CPU baseline of tools/point_optimisation_timing.py and a checker that needs no device. */
int dsm_optimize_immature_points_host(int w, int h, const dsm_immature_job *job, const float *const *frame_I, float huber_th,
                                      float min_idepth_h_act, int gn_iterations);

/* ---- Tracing the immature points against the new frame -------------------------------------------------------
 * replaces the loop of FrontEnd::traceNewCoarse (FrontEnd.cpp:276-327), which runs on every frame (:717, :730) over every immature
 * point of every frame of the window: ImmaturePoint::traceOn (UPSTREAM-DSO, parity unpinned) as the rules T1-T16 of DESIGN.md section
 * 14 state it, for the points of many sequences in one call.  Everything is float32 without contraction. */
/* ImmaturePointStatus, in the upstream enum's order (lastTraceStatus) */
#define DSM_IPS_GOOD 0
#define DSM_IPS_OOB 1
#define DSM_IPS_OUTLIER 2
#define DSM_IPS_SKIPPED 3
#define DSM_IPS_BADCONDITION 4
#define DSM_IPS_UNINITIALIZED 5
#define DSM_TRACE_MAX_HOSTS 16 /* largest n_hosts of a job */
#define DSM_TRACE_MAX_STEPS 99 /* the cap of the line search (T7) */

/* the settings traceOn reads; dsm_trace_params_default fills the upstream defaults */
typedef struct dsm_trace_params {
  float max_pix_search;    /* 0.027f  setting_maxPixSearch (times w + h) */
  float slack_interval;    /* 1.5f    setting_trace_slackInterval */
  float stepsize;          /* 1.0f    setting_trace_stepsize */
  float min_improvement;   /* 2.0f    setting_trace_minImprovementFactor */
  int min_test_radius;     /* 2       setting_minTraceTestRadius */
  int gn_iterations;       /* 3       setting_trace_GNIterations, 0 .. 16 */
  float gn_threshold;      /* 0.1f    setting_trace_GNThreshold */
  float extra_slack_on_th; /* 1.2f    setting_trace_extraSlackOnTH */
  float huber_th;          /* 9.0f    setting_huberTH */
} dsm_trace_params;

/* The immature points of one sequence against its new frame.  The new frame is level 0 of `target_slot` of `target_tracker` if
 * that is non-NULL (FrontEnd.cpp:717, :730: the frame just tracked), else frame `target_frame_id` of `target_window`; exactly one
 * of the two is given.  hosts: frame_hessians_ in order, with K R K^-1 and K t of host-to-new (:292-293) and
 * fromToVecExposure(host, new) cast to float (:295-297; the exp stays on the host).  The last seven arrays are the fields traceOn
 * reads and writes, updated in place. */
typedef struct dsm_trace_job {
  dsm_tracker *target_tracker;
  int target_slot;
  dsm_window *target_window;
  int target_frame_id;
  int n_hosts;       /* 0 .. DSM_TRACE_MAX_HOSTS */
  const float *krki; /* n_hosts * 9, row-major */
  const float *kt;   /* n_hosts * 3 */
  const float *aff;  /* n_hosts * 2 */
  int n_pts;
  const int *host;                  /* n_pts: index into the hosts */
  const float *u, *v, *energy_th;   /* n_pts each */
  const float *grad_h;              /* n_pts * 4: gradH, row-major */
  const float *color, *weights;     /* n_pts * 8 each */
  unsigned char *status;            /* n_pts, in/out: lastTraceStatus (DSM_IPS_*) */
  float *idepth_min, *idepth_max, *quality; /* n_pts each, in/out */
  float *trace_uv;                  /* n_pts * 2, in/out: lastTraceUV */
  float *trace_interval;            /* n_pts, in/out: lastTracePixelInterval */
  int *steps_out;                   /* optional (NULL), n_pts: numSteps searched, 0 if the search was not reached */
  int *counts_out;                  /* optional (NULL), 6: points per status after the call (:302-313) */
} dsm_trace_job;

/* the upstream defaults listed above */
int dsm_trace_params_default(dsm_trace_params *p);
/* FrontEnd.cpp:276-327 for every job: one staged copy through the context's page-locked arena, one launch, one host wait for the whole
 * batch; nothing is allocated once the arena has grown to the batch size; a job's results do not depend on the other jobs of the
 * call; one geometry per call; n_pts == 0 and n_hosts == 0 (then n_pts == 0) are valid.  Validation is all or nothing, before
 * anything is enqueued: DSM_ERR_INVALID for NULL arrays or negative counts, n_hosts above DSM_TRACE_MAX_HOSTS, a host index outside
 * [0, n_hosts), a status byte above 5, an empty or unknown target (an empty slot, an id not in the window, both or neither of
 * tracker and window), a tracker or window of another context, mixed geometries, gn_iterations outside [0, 16], a non-finite or
 * non-positive stepsize, any other non-finite parameter, a negative min_test_radius. */
int dsm_trace_points_batch(dsm_context *ctx, int n_jobs, const dsm_trace_job *jobs, const dsm_trace_params *params);
/* The same for one job as one plain sequential loop on the host plane target_I (w * h floats); the target fields of the job are
 * ignored.  The CPU baseline of tools/trace_timing.py and a checker that needs no device. */
int dsm_trace_points_host(int w, int h, const float *target_I, const dsm_trace_job *job, const dsm_trace_params *params);

/* ---- Selecting candidate pixels and creating the immature points ----------------------------------------------
 * replaces FrontEnd::makeNewTraces (FrontEnd.cpp:936-962, called at :824): PixelSelector::makeMaps and the ImmaturePoint constructor
 * (both UPSTREAM-DSO, parity unpinned) as the rules P1-P14 of DESIGN.md section 15 state them, for the new keyframes of many sequences
 * in one call.  Everything is float32 without contraction, or integer. */
#define DSM_SELECT_MAX_POTENTIAL 4096 /* largest potential a job may enter with or adapt to (P10) */

/* the settings makeMaps and the ImmaturePoint constructor read; dsm_select_params_default fills the upstream defaults */
typedef struct dsm_select_params {
  float min_grad_hist_cut;           /* 0.5f   setting_minGradHistCut */
  float min_grad_hist_add;           /* 7      setting_minGradHistAdd */
  float grad_downweight_per_level;   /* 0.75f  setting_gradDownweightPerLevel */
  int select_direction_distribution; /* 1      setting_selectDirectionDistribution */
  float th_factor;                   /* 1      thFactor of makeMaps */
  int recursions;                    /* 1      recursionsLeft of makeMaps, 0 .. 4 */
  int pattern_padding;               /* 2      patternPadding, 2 .. 8 */
  float outlier_th;                  /* 144    setting_outlierTH (12 * 12) */
  float outlier_th_sum_component;    /* 2500   setting_outlierTHSumComponent (50 * 50) */
  float overall_energy_th_weight;    /* 1      setting_overallEnergyTHWeight */
} dsm_select_params;

/* The new keyframe of one sequence: levels 0-2 of frame slot `slot` of `tracker`.  The point arrays have the layout dsm_trace_job
 * consumes, so they go straight into the next dsm_trace_points_batch; only the first max_pts points are written. */
typedef struct dsm_select_job {
  dsm_tracker *tracker; /* >= 3 levels, a frame in `slot` (0 or 1) */
  int slot;
  const float *b_inv;   /* optional (NULL), 256: the inverse response; weights the squared gradients (P1) */
  float density;        /* setting_desiredImmatureDensity (1500 in the reference's presets) */
  int *potential_io;    /* in/out: currentPotential of the sequence's PixelSelector, 3 at first use */
  int max_pts;          /* capacity of the point arrays */
  float *u, *v, *energy_th; /* max_pts each */
  float *grad_h;            /* max_pts * 4: gradH, row-major */
  float *color, *weights;   /* max_pts * 8 each */
  unsigned char *status;    /* max_pts: DSM_IPS_UNINITIALIZED */
  float *idepth_min, *idepth_max, *quality; /* max_pts each: 0, NaN, 10000 */
  float *type;              /* max_pts: the map value 1, 2 or 4 (my_type; dsm_activation_job.cand_type) */
  int *n_pts_out;           /* the points found (P13), which may exceed max_pts */
  int *num_total_out;       /* makeMaps' return value: the map entries left after the thinning (P11) */
  int *counts_out;          /* optional (NULL), 3: n2, n3, n4 of the last pass */
  int *passes_out;          /* optional (NULL): select passes run, 1 .. recursions + 1 */
  unsigned char *map_out;   /* optional (NULL), w * h: the selection map after the thinning */
} dsm_select_job;

/* the upstream defaults listed above */
int dsm_select_params_default(dsm_select_params *p);
/* The device copy of the random pattern (w * h bytes; upstream: srand(3141592), rand() & 0xFF, which depends on the libc) and all
 * scratch for max_jobs jobs of geometry w x h, allocated here and never afterwards.  w, h >= 32, max_jobs in [1, 4096]. */
int dsm_pixel_selector_create(dsm_context *ctx, int w, int h, int max_jobs, const unsigned char *random_pattern, dsm_pixel_selector **sel_out);
int dsm_pixel_selector_destroy(dsm_pixel_selector *sel);
/* FrontEnd.cpp:936-962 for every job: one staged copy through the context's page-locked arena, a fixed launch sequence (the
 * adaptation of the potential, P10, is decided on the device: every pass is enqueued and jobs that do not recurse leave it at
 * once), one host wait for the whole batch; nothing is allocated once the arena has grown to the batch size; a job's results do not
 * depend on the other jobs of the call.  Validation is all or nothing, before anything is enqueued: DSM_ERR_INVALID for NULL
 * arrays, n_jobs outside [1, max_jobs], a potential outside [1, DSM_SELECT_MAX_POTENTIAL], a density that is not finite or not
 * positive, a negative max_pts, recursions outside [0, 4], pattern_padding outside [2, 8], any non-finite setting, a tracker of
 * another context or with an empty slot, a geometry other than the selector's, fewer than 3 levels. */
int dsm_select_pixels_batch(dsm_pixel_selector *sel, int n_jobs, const dsm_select_job *jobs, const dsm_select_params *params);
/* The same for one job as one plain sequential loop on the host (upstream's loop with its running counter): I0, I1, I2 are the
 * intensity planes of levels 0-2 ((w >> l) * (h >> l) floats), random_pattern w * h bytes; job->tracker and job->slot are ignored;
 * w < 32 or h < 32 is refused.  The CPU baseline of tools/select_timing.py and a checker that needs no device. */
int dsm_select_pixels_host(int w, int h, const float *I0, const float *I1, const float *I2, const unsigned char *random_pattern,
                           const dsm_select_job *job, const dsm_select_params *params);

/* ---- Linearising the active residuals of the window optimisation ------------------------------------------------
 * replaces FrontEnd::linearizeAll (dso_helpers/FrontEndOptimize.cpp:121-179), which FrontEnd::optimize runs 8 to 14 times per keyframe:
 * PointFrameResidual::linearize (UPSTREAM-DSO, parity unpinned) for every active residual of the windows of many sequences in one call,
 * as the rules L1-L8 of DESIGN.md section 16 state it, with the per-window work around it (B1-B4): the energy sum, setNewFrameEnergyTH
 * and, in the fixLinearization pass, the keep / remove verdict and the relative baseline.  The call is stateless: the caller holds
 * state_state / state_energy, applies applyRes and decides whether the step is accepted.  Everything is float32 without contraction
 * except the energy sum (double) and the 0.01 factor of the relative baseline (double). */
#define DSM_LINEARIZE_HUBER_TH 9.0f                      /* setting_huberTH */
#define DSM_LINEARIZE_OUTLIER_TH_SUM_COMPONENT 2500.0f   /* setting_outlierTHSumComponent (50 * 50) */
#define DSM_LINEARIZE_SCALE_IDEPTH 1.0f                  /* SCALE_IDEPTH */
#define DSM_LINEARIZE_SCALE_F 50.0f                      /* SCALE_F */
#define DSM_LINEARIZE_SCALE_C 50.0f                      /* SCALE_C */
#define DSM_LINEARIZE_FRAME_ENERGY_TH_N 0.7f             /* setting_frameEnergyTHN */
#define DSM_LINEARIZE_FRAME_ENERGY_TH_FAC_MEDIAN 1.5f    /* setting_frameEnergyTHFacMedian */
#define DSM_LINEARIZE_FRAME_ENERGY_TH_CONST_WEIGHT 0.5f  /* setting_frameEnergyTHConstWeight */
#define DSM_LINEARIZE_OVERALL_ENERGY_TH_WEIGHT 1.0f      /* setting_overallEnergyTHWeight */
#define DSM_LINEARIZE_EMPTY_FRAME_ENERGY_TH 1152.0f      /* 12 * 12 * patternNum: no residual against the newest frame (B2) */
#define DSM_LINEARIZE_J_FLOATS 74                        /* one RawResidualJacobian row (L8) */

/* the settings linearize and setNewFrameEnergyTH read; dsm_linearize_params_default fills the upstream defaults */
typedef struct dsm_linearize_params {
  float huber_th;                 /* 9     */
  float outlier_th_sum_component; /* 2500  */
  float scale_idepth;             /* 1     */
  float scale_f;                  /* 50    */
  float scale_c;                  /* 50    */
  float thn;                      /* 0.7   in [0, 1) */
  float fac_median;               /* 1.5   */
  float cw;                       /* 0.5   */
  float ow;                       /* 1     */
  int zero_jab_a;                 /* 0     setting_affineOptModeA < 0: JabF[0] is stored as 0 (L6) */
  int zero_jab_b;                 /* 0     setting_affineOptModeB < 0: JabF[1] is stored as 0 */
} dsm_linearize_params;

/* One window.  frame_ids: frame_hessians_ in order; pre_*: the FrameFramePrecalc fields of every [host][target] pair in float32
 * (row-major 3 x 3), the diagonal is not read; frame_energy_th: frameEnergyTH of every frame, which this pass compares against.
 * A point is a PointHessian (host: an index into frame_ids), a residual a PointFrameResidual of it (point: an index into the points,
 * target: an index into frame_ids, never the point's host) with its committed state_state / state_energy. */
typedef struct dsm_linearize_job {
  dsm_window *window;         /* ignored by dsm_linearize_residuals_host */
  float cam[4];               /* fxl, fyl, cxl, cyl */
  float cam_inv[2];           /* fxli, fyli */
  int n_frames;               /* 1 .. DSM_WINDOW_MAX_FRAMES */
  const int *frame_ids;       /* n_frames */
  const float *pre_RTll_0;    /* n_frames * n_frames * 9, [host][target] */
  const float *pre_tTll_0;    /* n_frames * n_frames * 3 */
  const float *pre_KRKiTll;   /* n_frames * n_frames * 9 */
  const float *pre_KtTll;     /* n_frames * n_frames * 3 */
  const float *pre_aff_mode;  /* n_frames * n_frames * 2 */
  const float *pre_b0_mode;   /* n_frames * n_frames */
  const float *frame_energy_th; /* n_frames */
  int n_pts;
  const int *host;            /* n_pts */
  const float *u, *v, *idepth_scaled, *idepth_zero_scaled; /* n_pts each */
  const float *color;         /* n_pts * 8 */
  const float *weights;       /* n_pts * 8 */
  int n_res;
  const int *point;           /* n_res */
  const int *target;          /* n_res */
  const unsigned char *state_in; /* n_res: DSM_RES_IN / _OOB / _OUTLIER */
  const float *energy_in;     /* n_res: state_energy */
  const unsigned char *is_new;   /* n_res: isNew; read only with fix_linearization */
  int fix_linearization;
  unsigned char *new_state;   /* n_res: state_NewState */
  float *new_energy;          /* n_res: the value linearize returns (state_NewEnergy; energy_in for a residual that ends OOB) */
  float *new_energy_with_outlier; /* n_res: state_NewEnergyWithOutlier, -1 for a residual that ends OOB */
  float *J_out;               /* optional (NULL), n_res * 74: resF[8], Jpdxi[2][6], Jpdc[2][4], Jpdd[2], JIdx[2][8], JabF[2][8], JIdx2[4],
                                 JabJIdx[4], Jab2[4]; like the next two, the row of a residual that ends OOB is not written */
  float *center_projected_to; /* optional (NULL), n_res * 3 */
  float *projected_to;        /* optional (NULL), n_res * 16: (Ku, Kv) of every pattern pixel */
  unsigned char *keep;        /* optional (NULL), n_res; written with fix_linearization only: 1 = the residual stays active */
  float *rel_bs;              /* optional (NULL), n_res; written with fix_linearization only: the relative baseline of a kept new
                                 residual, 0 for every other */
  double *energy_out;         /* the sum of new_energy in residual order, in double (B1) */
  float *new_frame_energy_th_out; /* setNewFrameEnergyTH: the next frameEnergyTH of the newest frame, frame_ids[n_frames - 1] (B2) */
} dsm_linearize_job;

/* the upstream defaults listed above */
int dsm_linearize_params_default(dsm_linearize_params *p);
/* FrontEndOptimize.cpp:121-179 for every job: one staged copy through the context's page-locked arena, one launch, one host wait for
 * the whole batch; the energy sum and the order statistic of B2 are formed on the host from the read-back; nothing is allocated once
 * the arena has grown to the batch size; a job's results do not depend on the other jobs of the call.  A window may serve several
 * jobs; one geometry per call; n_res == 0, n_pts == 0 and a job of one frame are valid (energy 0, threshold 1152).  Validation is
 * all or nothing, before anything is enqueued: DSM_ERR_INVALID for NULL required arrays or negative counts, n_frames outside
 * [1, DSM_WINDOW_MAX_FRAMES], a host, point or target index out of range, a target equal to the host of the residual's point, a
 * state_in other than DSM_RES_IN / _OOB / _OUTLIER, a frame id that is not in the window, mixed geometries, non-finite parameters,
 * thn outside [0, 1). */
int dsm_linearize_residuals_batch(dsm_context *ctx, int n_jobs, const dsm_linearize_job *jobs, const dsm_linearize_params *params);
/* The same for one job as one plain sequential loop on the host: job->window is ignored, frame_I[i] is the w * h level-0 intensity
 * plane of frame_ids[i].  The CPU baseline of tools/linearize_timing.py and a checker that needs no device. */
int dsm_linearize_residuals_host(int w, int h, const dsm_linearize_job *job, const float *const *frame_I, const dsm_linearize_params *params);

/* ---- Hessian and Schur accumulation of the window optimisation ---------------------------------------------------
 * replaces, for the active residuals, what FrontEnd::optimize (dso_helpers/FrontEndOptimize.cpp:332-486) does between linearizeAll
 * and the solve of solveSystem: accumulateAF_MT / accumulateSCF_MT, that is AccumulatedTopHessianSSE::addPoint and
 * AccumulatedSCHessianSSE::addPoint per point and their stitchDouble (UPSTREAM-DSO, parity unpinned), as the rules A0-A3, P1, S1-S3
 * and T1 of DESIGN.md section 17 state them.  One call linearises (lin, section 16, every output with the same meaning) and
 * accumulates; the Jacobian rows stay on the device unless lin.J_out asks for them.  The call is stateless: a rejected trial step
 * discards its accumulators.  Products are float32 without contraction, the accumulators and the stitch are double. */
#define DSM_HESSIAN_TOP 13 /* one pair's accumulator: C (4), xi (6), a, b, r */

/* One window: lin and what the accumulation reads and returns on top of it; n = lin.n_frames, N = 4 + 8 n. */
typedef struct dsm_hessian_job {
  dsm_linearize_job lin;      /* J_out is normally NULL */
  const double *ad_host;      /* n * n * 8 * 8, [host][target], row-major: EF->adHost */
  const double *ad_target;    /* n * n * 8 * 8: EF->adTarget */
  const float *prior;         /* the next seven: optional (NULL: zeros).  n_pts: priorF */
  const float *delta;         /* n_pts: deltaF */
  const float *hdd_lin;       /* n_pts: Hdd_accLF */
  const float *bd_lin;        /* n_pts: bd_accLF */
  const float *hcd_lin;       /* n_pts * 4: Hcd_accLF */
  int shift_prior_to_zero;    /* solveSystemF passes 1: bd_sum takes prior * delta */
  double *H_A, *b_A;          /* N * N (full, symmetric) and N: accumulateAF after stitchDouble */
  double *H_sc, *b_sc;        /* N * N and N: accumulateSCF after stitchDouble */
  double *acc_top;            /* the rest: optional (NULL).  n * n * 13 * 13, full: acc[tid][h + n t] of AccumulatedTopHessianSSE */
  double *acc_D;              /* n * n * n * 8 * 8 as [host][t1][t2] */
  double *acc_E;              /* n * n * 8 * 4 */
  double *acc_EB;             /* n * n * 8 */
  double *acc_Hcc;            /* 16 */
  double *acc_bc;             /* 4 */
  unsigned char *active;      /* n_res: 1 = the residual contributes (A0) */
  float *JpJdF;               /* n_res * 8, written for active residuals only: what resubstituteFPt reads */
  float *hdd_acc, *bd_acc;    /* n_pts each: Hdd_accAF, bd_accAF */
  float *hcd_acc;             /* n_pts * 4: Hcd_accAF */
  float *hdi, *bd_sum, *idepth_hessian; /* n_pts each: HdiF, bdSumF, idepth_hessian (all 0 for a point without an active residual) */
} dsm_hessian_job;

/* accumulateAF_MT + accumulateSCF_MT after linearizeAll for every job: one staged copy through the context's arena, the launch of
 * dsm_linearize_residuals_batch and four more, one read-back of the heads, the accumulators and the optional arrays; the stitch (T1)
 * and B1 / B2 run on the host.  A job's results do not depend on the other jobs of the call or on the launch geometry.  Validation is
 * all or nothing, before anything is enqueued: DSM_ERR_INVALID for everything dsm_linearize_residuals_batch refuses, a NULL ad_host,
 * ad_target, H_A, b_A, H_sc or b_sc, a non-finite ad_*, prior, delta or *_lin, and a point with two residuals against one target.
 * n_res == 0, n_pts == 0 and a job of one frame are valid and give zero matrices. */
int dsm_window_hessian_batch(dsm_context *ctx, int n_jobs, const dsm_hessian_job *jobs, const dsm_linearize_params *params);
/* The same for one job as plain sequential loops on the host planes frame_I (as dsm_linearize_residuals_host; job->lin.window is
 * ignored).  The CPU baseline of tools/hessian_timing.py and a checker that needs no device. */
int dsm_window_hessian_host(int w, int h, const dsm_hessian_job *job, const float *const *frame_I, const dsm_linearize_params *params);

/* ---- Stitch, damping, solve and back-substitution of the window optimisation -------------------------------------
 * replaces, together with the section above, everything FrontEnd::optimize (dso_helpers/FrontEndOptimize.cpp:332-486) does between
 * backupState and doStepFromBackup for one trial step: linearizeAll, accumulateAF_MT / accumulateSCF_MT, the non-SVD,
 * non-ORTHOGONALIZE_SYSTEM branch of EnergyFunctional::solveSystemF with the orthogonalize projection on a caller-supplied basis, and
 * resubstituteF_MT / resubstituteFPt (UPSTREAM-DSO, parity unpinned), as the rules T1d, F1-F8, R1-R3 and V of DESIGN.md section 18
 * state them.  All arithmetic is IEEE, left to right as written, without contraction. */
#define DSM_SOLVE_MAX_NULL 8
#define DSM_SOLVE_X_NOT_FINITE 1    /* flags bit 0: some x[i] is not finite */
#define DSM_SOLVE_STEP_NOT_FINITE 2 /* flags bit 1: some point's step is not finite */

/* One window: hes and what the solve reads and returns on top of it; n = hes.lin.n_frames, N = 4 + 8 n. */
typedef struct dsm_solve_job {
  dsm_hessian_job hes;        /* H_A, b_A, H_sc, b_sc are optional (NULL) here; every other field with the same meaning */
  const double *H_L, *b_L;    /* N * N (row-major) and N: accumulateLF_MT's stitched result */
  const double *H_M, *b_M;    /* the next three: optional (NULL: zeros).  N * N and N: HM, bM */
  const double *delta_x;      /* N: getStitchedDeltaF */
  double lambda;              /* finite, > -1; the caller applies SOLVER_FIX_LAMBDA / SOLVER_USE_GN itself */
  int n_null;                 /* 0 .. DSM_SOLVE_MAX_NULL; 0: no projection (F7) */
  const double *null_basis;   /* N * n_null, row-major: the nullspaces to project out; read with n_null > 0 only */
  const double *null_pinv;    /* n_null * N: their pseudo-inverse */
  double *x;                  /* N: lastX; the steps are -x */
  float *step;                /* n_pts: the inverse-depth step of every point (0 for a point without an active residual) */
  int *flags;                 /* one word: DSM_SOLVE_X_NOT_FINITE | DSM_SOLVE_STEP_NOT_FINITE; nothing is clamped or replaced */
  double *last_HS, *last_bS;  /* optional (NULL).  N * N and N: HFinal - H_sc and bFinal before damping */
} dsm_solve_job;

/* One trial step for every job: the staged copy and the five launches of dsm_window_hessian_batch, then three more (stitch, solve,
 * back-substitution) on the same arena, one read-back of the heads, x, the steps, the flags and what the job asks for on top: the
 * stitched matrices, the raw accumulators and the per-point results cost their read-back only when a job asks for them.  A job's
 * results do not depend on the other jobs of the call or on the launch geometry.  Validation is all or nothing, before anything is
 * enqueued: DSM_ERR_INVALID for everything dsm_window_hessian_batch refuses except a NULL H_A, b_A, H_sc or b_sc, and for a NULL H_L,
 * b_L, x, step or flags, a non-finite lambda or lambda <= -1, a non-finite H_L, b_L, H_M, b_M, delta_x, null_basis or null_pinv,
 * n_null outside [0, DSM_SOLVE_MAX_NULL], n_null > 0 with a NULL basis or pseudo-inverse.  n_res == 0, n_pts == 0 and a job of one
 * frame are valid: the system is then H_L + H_M alone. */
int dsm_window_solve_batch(dsm_context *ctx, int n_jobs, const dsm_solve_job *jobs, const dsm_linearize_params *params);
/* The same for one job on the host: dsm_window_hessian_host, then plain loops over F1-R3.  The CPU baseline of tools/solve_timing.py
 * and a checker that needs no device. */
int dsm_window_solve_host(int w, int h, const dsm_solve_job *job, const float *const *frame_I, const dsm_linearize_params *params);

/* ---- Applying a step and re-linearising: one iteration of the window optimisation in one call -------------------
 * replaces, together with the three sections above, one iteration of the loop of FrontEnd::optimize (dso_helpers/FrontEndOptimize.cpp:
 * 332-486): doStepFromBackup (:182-262, the non-SOLVER_MOMENTUM branch) with what it calls -- FrameHessian::setState,
 * CalibHessian::setValue, PointHessian::setIdepth / setIdepthZero, setPrecalcValues (:300-323, FrameFramePrecalc::set and
 * EnergyFunctional::setDeltaF), calcMEnergyF and the prior lines of the stitch (UPSTREAM-DSO, parity unpinned; the priors are
 * FrontEnd.cpp:964-972's) -- as the rules D1-D4, Q1-Q4, E1-E3 and V of DESIGN.md section 19 state them, and then everything
 * dsm_window_solve_batch does, at the trial state.  The call takes the backed-up state and a step, forms the trial state and what
 * derives from it on the device, and returns the trial state, its energies, can_break and the next step, computed as if the trial
 * were accepted.  Accept: commit the returned state and pass the returned x (as frame_step = -x, calib_step = -x[0..3], idepth_step =
 * step) to the next call.  Reject: call again with all five factors 0 and lambda * 100.
 * NOT here: SOLVER_MOMENTUM; the step-size heuristic (:390-405; the caller passes the factors); calcLEnergy and accumulateLF_MT (zero
 * while no residual is linearised, which is all of optimize); setAdjointsF (ad_host / ad_target stay the caller's: the evaluation point
 * does not move inside optimize); the nullspaces; setEvalPT after the loop (:455-464); applyRes; the accept decision.  (Marginalisation, which produces H_M / b_M, is
 * dsm_window_marginalize_batch below; setAdjointsF and setEvalPT after the loop are dsm_window_finish_batch)
 * All arithmetic is IEEE, left to right as written, without contraction. */
typedef struct dsm_step_params {
  double scale_xi_trans;     /* 0.5   SCALE_XI_TRANS */
  double scale_xi_rot;       /* 1     SCALE_XI_ROT */
  double scale_a;            /* 10    SCALE_A */
  double scale_b;            /* 1000  SCALE_B */
  double th_opt_iterations;  /* 1.2   setting_thOptIterations */
} dsm_step_params;

/* One window; n = sol.hes.lin.n_frames, N = 4 + 8 n, n_pts = sol.hes.lin.n_pts; poses are {qx,qy,qz,qw,tx,ty,tz}.  In sol, every field
 * the device does not form keeps its meaning.  What the device forms MUST be NULL: sol.hes.lin.pre_RTll_0, pre_tTll_0, pre_KRKiTll,
 * pre_KtTll, pre_aff_mode, pre_b0_mode, idepth_scaled, idepth_zero_scaled, sol.hes.delta and sol.delta_x.  sol.hes.lin.cam and cam_inv
 * are not read. */
typedef struct dsm_step_job {
  dsm_solve_job sol;
  const double *world_to_cam_eval; /* n * 7: worldToCam_evalPT, unit quaternions */
  const double *state_zero;        /* n * 8, unscaled: state_zero */
  const double *state_backup;      /* n * 8: state_backup */
  const double *frame_step;        /* n * 8: fh->step, which is -x of F8 */
  const double *calib_zero;        /* 4: value_zero */
  const double *calib_backup;      /* 4: value_backup */
  const double *calib_step;        /* 4: h_calib_.step */
  const float *idepth_backup;      /* n_pts */
  const float *idepth_step;        /* n_pts: ph->step */
  const float *exposure;           /* n: ab_exposure */
  float stepfac[5];                /* C, T, R, A, D */
  const double *prior;             /* the next two: optional (NULL: no prior).  N: cPrior, then every frame's prior */
  const double *prior_zero;        /* N: the calibration's value_zero, then every frame's getPriorZero */
  double *state_out;               /* n * 8: the trial state */
  double *calib_out;               /* 4 */
  float *idepth_out;               /* n_pts */
  double *world_to_cam_out;        /* n * 7: PRE_worldToCam */
  double *cam_to_world_out;        /* optional (NULL), n * 7: PRE_camToWorld */
  int *can_break;                  /* one word: what doStepFromBackup returns */
  float *step_sums;                /* 6: sumA, sumB, sumR, sumT, sumID, sumNID after their divisions */
  double *energy_m;                /* calcMEnergyF */
  float *cam_out;                  /* the rest: optional (NULL), what the device formed in the shapes dsm_solve_job takes it, so that a
                                      returned set is a valid input of dsm_window_solve_batch.  6: cam, cam_inv */
  float *pre_RTll_0_out, *pre_tTll_0_out, *pre_KRKiTll_out, *pre_KtTll_out, *pre_aff_mode_out, *pre_b0_mode_out; /* n * n * (9, 3, 9, 3, 2, 1) */
  double *delta_x_out;             /* N */
  double *H_L_out, *b_L_out;       /* N * N and N: H_L, b_L with the priors added (E3) */
} dsm_step_job;

/* the upstream defaults listed above */
int dsm_step_params_default(dsm_step_params *p);
/* One iteration for every job: the staged copy of dsm_window_solve_batch with the step's inputs on top, two launches (stp_frame_kernel,
 * stp_point_kernel) that write the trial state's tables where the eight launches of dsm_window_solve_batch read them, those eight
 * launches unchanged, one read-back.  A job's results do not depend on the other jobs of the call or on the launch geometry.
 * Validation is all or nothing, before anything is enqueued: DSM_ERR_INVALID for everything dsm_window_solve_batch refuses (except
 * the NULLs this call requires), one of the must-be-NULL fields given, a NULL required array, a non-finite input or step factor, a
 * world_to_cam_eval quaternion whose squared norm is further than 1e-9 from 1, prior without prior_zero or the reverse, non-finite or
 * non-positive step parameters.  n_res == 0, n_pts == 0 and a job of one frame are valid. */
int dsm_window_step_batch(dsm_context *ctx, int n_jobs, const dsm_step_job *jobs, const dsm_linearize_params *lp, const dsm_step_params *sp);
/* The same for one job on the host: D1-E3 as plain loops, then dsm_window_solve_host.  A checker that needs no device. */
int dsm_window_step_host(int w, int h, const dsm_step_job *job, const float *const *frame_I, const dsm_linearize_params *lp,
                         const dsm_step_params *sp);

/* ---- The accept / reject loop of the window optimisation in one call -------------------------------------------
 * replaces, together with the four sections above, the loop of FrontEnd::optimize (dso_helpers/FrontEndOptimize.cpp:332-486): the
 * linearizeAll and applyRes before it (:362-371), and per iteration (:382-453) backupState, the step-size heuristic (:390-405),
 * doStepFromBackup, linearizeAll, the accept test (:427-429), applyRes or loadSateBackup with its linearizeAll (:444-448), the lambda
 * schedule and the break (:451).  A PASS is what one dsm_window_step_batch call does.  Every job carries its own lambda, factors,
 * iteration count and break:
 *   pass 0:      zero factors, lambda = lambda_init                      -> always committed; last = E + E_M
 *   iteration i: trial pass, factors = stepsize, lambda_trial = lambda * lambda_accept_fac
 *                accept (force_accept, or E + E_M < last, in double): commit; lambda = lambda_trial
 *                reject: lambda = lambda * lambda_reject_fac; re-pass with zero factors at the backed-up state with that lambda; commit it
 *                break after the iteration if the TRIAL's can_break && i >= min_iterations
 * Commit: the returned state, calibration and depths become the backup, new_state / new_energy become state_in / energy_in (applyRes),
 * frame_step = -x[4..], calib_step = -x[0..3], idepth_step = step.  frame_energy_th[n - 1] takes new_frame_energy_th after EVERY pass.
 * The rules are the project's statement; parity with the parts of DSO that are not under the reference tree is
 * unpinned.  NOT here: accumulateLF_MT, the nullspaces, setEvalPT after the loop, SOLVER_MOMENTUM.  (Marginalisation, which
 * produces the H_M / b_M this loop reads, is dsm_window_marginalize_batch below; setEvalPT after the loop with what follows it is
 * dsm_window_finish_batch, which runs this loop first: DESIGN.md section 22.)
 * The struct defaults reproduce the loop of host/step_demo.cpp (lambda 0.1, x 0.25, x 100, setting_minOptIterations = 1, the energy
 * test, step size 1).  The recalled upstream defaults are setting_forceAceptStep = true and SOLVER_FIX_LAMBDA set (the solve then
 * always gets 1e-5): force_accept = 1, fixed_lambda = 1e-5; they are not citable under the reference tree. */
#define DSM_OPTIMIZE_MAX_ITERATIONS 20

typedef struct dsm_optimize_params {
  double lambda_init;        /* 0.1   :382 */
  double lambda_accept_fac;  /* 0.25  :442 */
  double lambda_reject_fac;  /* 100   :448 */
  double fixed_lambda;       /* -1    >= 0: every solve gets this value; the schedule still runs and is logged */
  int min_iterations;        /* 1     setting_minOptIterations */
  int force_accept;          /* 0     setting_forceAceptStep */
  int step_momentum;         /* 0     SOLVER_STEPMOMENTUM: the step-size heuristic of :390-405; otherwise the step size is 1 */
} dsm_optimize_params;

/* One window.  step describes the window at its current state: state_backup, calib_backup and idepth_backup are the current values,
 * sol.hes.lin.state_in / energy_in the committed residual states.  step.frame_step, step.calib_step and step.idepth_step MUST be NULL
 * (the loop forms them); step.stepfac and step.sol.lambda are not read.  Every output of step receives the values of THE JOB'S LAST
 * PASS: in both branches they describe the committed state, with the solve (x, step, flags) computed as for a next iteration.
 * P = 1 + 2 * max_iterations bounds the passes. */
typedef struct dsm_optimize_job {
  dsm_step_job step;
  int max_iterations;            /* 0 .. DSM_OPTIMIZE_MAX_ITERATIONS; 0: pass 0 only */
  int *n_iterations;             /* iterations run */
  int *n_passes;                 /* passes run: 1 + iterations + rejected iterations */
  unsigned char *pattern;        /* max_iterations: 'A' or 'R' per iteration run, 0 behind them */
  double *pass_energy;           /* P * 2: E and E_M of every pass, 0 behind them */
  double *pass_lambda;           /* P: the schedule's lambda of every pass (what the solve gets unless fixed_lambda >= 0), 0 behind them */
  float *iter_stepsize;          /* max_iterations: the factor of every trial, 0 behind them */
  unsigned char *iter_can_break; /* max_iterations: the trial's can_break, 0 behind them */
  double *last_energy;           /* 2: E and E_M of the last committed pass */
  double *lambda_out;            /* the schedule's lambda after the last iteration */
  float *frame_energy_th_out;    /* frame_energy_th[n - 1] after the last pass */
} dsm_optimize_job;

/* the defaults listed above */
int dsm_optimize_params_default(dsm_optimize_params *p);
/* The loop for every job: ONE staged copy (that of dsm_window_step_batch with the loop's state on top), then the passes back to back on
 * the context's stream with no host wait between them: the ten launches of dsm_window_step_batch and two more (opt_decide_kernel: the
 * ordered energy sum and the order statistic of new_frame_energy_th, the decision, the lambda schedule, the heuristic and the frames'
 * part of the commit; opt_commit_kernel: the points' and residuals' part) that write the next pass's inputs where the ten read them.
 * 1 + max over the jobs of max_iterations passes are enqueued and read back; only if a job is then unfinished (it rejected a step), the
 * remaining passes follow: at most two host waits per call.  A finished job is frozen: its later passes recompute the same bytes.  A
 * job's results do not depend on the other jobs of the call or on the launch geometry.  Validation is all or nothing, before anything
 * is enqueued: DSM_ERR_INVALID for everything dsm_window_step_batch refuses (except the NULLs this call requires), frame_step,
 * calib_step or idepth_step given, a NULL output of this struct, parameters that are not finite, lambda_init <= -1, a factor <= 0,
 * min_iterations < 0, max_iterations outside [0, DSM_OPTIMIZE_MAX_ITERATIONS]. */
int dsm_window_optimize_batch(dsm_context *ctx, int n_jobs, const dsm_optimize_job *jobs, const dsm_linearize_params *lp,
                              const dsm_step_params *sp, const dsm_optimize_params *op);
/* The same for one job on the host: the loop over dsm_window_step_host.  A checker that needs no device.  (A state that stops being
 * finite in the middle of the loop is refused by the pass that would read it: DSM_ERR_INVALID, the outputs of step then hold the last
 * completed pass and the outputs of this struct are not written; the device form carries the NaNs through.) */
int dsm_window_optimize_host(int w, int h, const dsm_optimize_job *job, const float *const *frame_I, const dsm_linearize_params *lp,
                             const dsm_step_params *sp, const dsm_optimize_params *op);

/* ---- Marginalising points and frames of the window ---------------------------------------------------------------
 * replaces what FrontEnd::makeKeyFrame does right after optimize (FrontEnd.cpp:816-839): flagPointsForRemoval (FrontEnd.cpp:504-583),
 * EnergyFunctional::marginalizePointsF and, per frame that leaves, EnergyFunctional::marginalizeFrame (FrontEndMarginalize.cpp:148-153
 * calls it).  isOOB, isInlierNew, fixLinearizationF, addPoint<2>, marginalizePointsF and marginalizeFrame are UPSTREAM-DSO and not under
 * the reference tree: parity is unpinned, and the rules C, M1, X1, A1', M2, G1-G7, Z and V of DESIGN.md section 21 are the project's
 * statement.  The call produces the H_M / b_M that the next keyframe's dsm_window_solve_batch / _step_batch / _optimize_batch reads.
 * NOT here: the SOLVER_ORTHOGONALIZE_* projections, connectivityMap, the bookkeeping that erases points, residuals and frames (the
 * verdicts and marg_frames tell the caller what to erase), flagFramesForMarginalization, the nullspaces, setEvalPT (which, with the
 * final linearizeAll(true) whose results this call reads, is dsm_window_finish_batch: DESIGN.md section 22).
 * All arithmetic is IEEE, left to right as written, without contraction. */
typedef struct dsm_marginalize_params {
  int min_good_active_res_for_marg; /* 3       setting_minGoodActiveResForMarg */
  int min_good_res_for_marg;        /* 4       setting_minGoodResForMarg */
  float min_idepth_h_marg;          /* 50      setting_minIdepthH_marg */
  float marg_weight_fac;            /* 0.25    setting_margWeightFac */
  float idepth_fix_prior_marg_fac;  /* 360000  setting_idepthFixPriorMargFac (600 * 600) */
} dsm_marginalize_params;           /* the defaults are the recalled upstream settings; they are not citable under the reference tree */

/* One window as optimize left it; n = hes.lin.n_frames, N = 4 + 8 n, n_pts = hes.lin.n_pts, n_res = hes.lin.n_res.
 * hes describes the WHOLE window: lin.state_in the committed state of every residual, the precalc tables at the committed state,
 * frame_energy_th, ad_host, ad_target, per point prior and delta.  Not read: lin.energy_in's values, lin.is_new, hes.hdd_lin,
 * hes.bd_lin, hes.hcd_lin, hes.shift_prior_to_zero (M1 and A1' fix them).  MUST be NULL / 0: lin.J_out, lin.keep, lin.rel_bs,
 * lin.fix_linearization.  H_A, b_A, H_sc, b_sc are optional here.  Every per-residual and per-point output of hes (lin.new_state,
 * new_energy, new_energy_with_outlier, center_projected_to, projected_to, active, JpJdF, hdd_acc ... idepth_hessian) is indexed as
 * the window's residuals and points are and is written for the residuals and points of the sub-window (M1) only; the rest keeps the
 * caller's bytes.  lin.energy_out and lin.new_frame_energy_th_out take the sub-window's values (B1, B2 over its residuals); H_A, b_A,
 * H_sc, b_sc and the raw accumulators are those of the sub-window. */
typedef struct dsm_marginalize_job {
  dsm_hessian_job hes;
  const unsigned char *flagged;    /* n: flaggedForMarginalization */
  const int *n_good_residuals;     /* n_pts: numGoodResiduals */
  const unsigned char *last_state; /* n_pts * 2: lastResiduals[0].second, [1].second as DSM_RES_* */
  const float *idepth_hessian;     /* n_pts: idepth_hessian as the last accumulation of optimize left it */
  const float *ad_ht_delta;        /* n * n * 8, [host][target]: EF->adHTdeltaF */
  const float *c_delta;            /* 4: cDeltaF */
  const double *H_M, *b_M;         /* optional (NULL: zeros).  N * N (row-major) and N */
  int n_marg_frames;               /* 0 .. n */
  const int *marg_frames;          /* n_marg_frames: strictly ascending indices into frame_ids, each with flagged set */
  const double *frame_prior;       /* n_marg_frames * 8: EFFrame::prior of each */
  const double *frame_delta_prior; /* n_marg_frames * 8: EFFrame::delta_prior of each */
  unsigned char *verdict;          /* n_pts: 0 keep, 1 marginalise, 2 drop (as dsm_activate_points_batch) */
  double *H_M_out, *b_M_out;       /* N' * N' and N', N' = N - 8 n_marg_frames: the frames that stay, in order */
  int *n_res_marg;                 /* one word: the increment of resInM */
  double *H_M_points, *b_M_points; /* the rest: optional (NULL).  N * N and N: the prior after the points, before a frame leaves */
  float *res_to_zero;              /* n_res * 8, written for the active residuals of the sub-window only (X1) */
} dsm_marginalize_job;

/* the defaults listed above */
int dsm_marginalize_params_default(dsm_marginalize_params *p);
/* flagPointsForRemoval's verdicts, marginalizePointsF and marginalizeFrame for every job: the verdicts (C) during staging on the host,
 * ONE staged copy of the sub-window (the points of verdict 1 with all their residuals), the five launches of dsm_window_hessian_batch
 * with mrg_fix_kernel (X1) between the linearisation and the accumulation, the stitch of dsm_window_solve_batch, mrg_fold_kernel (M2)
 * and mrg_frame_kernel (G1-G7 for the job's frames, one workgroup per job), one read-back.  A job's results do not depend on the other
 * jobs of the call or on the launch geometry.  Validation is all or nothing, before anything is enqueued and with no output touched:
 * DSM_ERR_INVALID for everything dsm_window_hessian_batch refuses (except a NULL H_A, b_A, H_sc or b_sc), one of the must-be-NULL
 * fields given, a NULL flagged, n_good_residuals, last_state, idepth_hessian, ad_ht_delta, c_delta, verdict, H_M_out, b_M_out or
 * n_res_marg, a last_state other than DSM_RES_IN / _OOB / _OUTLIER, a non-finite idepth_hessian, ad_ht_delta, c_delta, H_M, b_M,
 * frame_prior or frame_delta_prior, n_marg_frames outside [0, n] or, when it is not 0, a NULL marg_frames, frame_prior or
 * frame_delta_prior, marg_frames that are not strictly ascending, out of range or not flagged, a marginalised frame that still hosts
 * a point of verdict 0, parameters that are not finite, or a negative count among them.  n_res == 0, n_pts == 0, a job of one frame
 * and a job whose every frame leaves (N' = 4) are valid. */
int dsm_window_marginalize_batch(dsm_context *ctx, int n_jobs, const dsm_marginalize_job *jobs, const dsm_linearize_params *lin_params,
                                 const dsm_marginalize_params *marg_params);
/* The same for one job on the host planes frame_I (as dsm_window_hessian_host; job->hes.lin.window is ignored): plain loops over the
 * same marginalize_math.hpp.  A checker that needs no device. */
int dsm_window_marginalize_host(int w, int h, const dsm_marginalize_job *job, const float *const *frame_I,
                                const dsm_linearize_params *lin_params, const dsm_marginalize_params *marg_params);

/* ---- The end of optimize in the same call as its loop ----------------------------------------------------------
 * replaces, behind the loop of the section above, what FrontEnd::optimize does after it (dso_helpers/FrontEndOptimize.cpp:455-486):
 * setEvalPT of the newest frame (:455-460), EnergyFunctional::setAdjointsF and setDeltaF, setPrecalcValues at the new evaluation point,
 * linearizeAll(true) with its bookkeeping (:466, :39-72, :145-176: numGoodResiduals, maxRelBaseline, lastResiduals, the residuals that
 * do not survive) and removeOutliers (:504-523), as the rules Z1-Z8 and V of DESIGN.md section 22 state them.  setEvalPT, setAdjointsF
 * and setDeltaF are UPSTREAM-DSO and not under the reference tree: parity is unpinned.  What the call returns is what
 * dsm_window_marginalize_batch reads.  NOT here: the nullspaces, flagFramesForMarginalization, erasing the residuals and points (the
 * index maps tell the caller what to erase and how to renumber).
 * All arithmetic is IEEE, left to right as written, without contraction. */

/* One window; n, N, n_pts, n_res as in opt.  opt runs exactly as dsm_window_optimize_batch runs it and every output of opt keeps its
 * meaning (the job's last pass).  opt.step.sol.hes.lin.is_new is read here (and only here).  A residual is REMOVED when keep is 0. */
typedef struct dsm_finish_job {
  dsm_optimize_job opt;
  const int *n_good_residuals_in;      /* n_pts: numGoodResiduals */
  const float *max_rel_baseline_in;    /* n_pts: maxRelBaseline */
  const int *last_res;                 /* n_pts * 2: the residual index of lastResiduals[0].first, [1].first; -1: none */
  const unsigned char *last_state_in;  /* n_pts * 2: lastResiduals[0].second, [1].second as DSM_RES_* */
  double *world_to_cam_eval_out;       /* n * 7: worldToCam_evalPT after setEvalPT (Z1) */
  double *state_zero_out;              /* n * 8 */
  double *state_out;                   /* n * 8 */
  double *ad_host_out, *ad_target_out; /* n * n * 8 * 8 each, as dsm_hessian_job reads them (Z2) */
  float *ad_ht_delta_out;              /* n * n * 8, as dsm_marginalize_job reads it (Z3) */
  float *c_delta_out;                  /* 4 */
  double *delta_x_out;                 /* N */
  float *pre_RTll_0_out, *pre_tTll_0_out, *pre_KRKiTll_out, *pre_KtTll_out, *pre_aff_mode_out, *pre_b0_mode_out; /* n * n * (9, 3, 9, 3, 2, 1) */
  float *cam_out;                      /* 6: cam, cam_inv */
  unsigned char *new_state;            /* the next five: n_res each, the final linearisation (Z4); a residual's state from here on */
  float *new_energy;
  float *new_energy_with_outlier;
  unsigned char *keep;
  float *rel_bs;
  double *energy;                      /* B1 of the final linearisation */
  float *frame_energy_th_out;          /* B2 of the final linearisation */
  int *n_good_residuals_out;           /* n_pts (Z5) */
  float *max_rel_baseline_out;         /* n_pts */
  int *last_res_out;                   /* n_pts * 2, in the old numbering; -1 where the residual was removed */
  unsigned char *last_state_out;       /* n_pts * 2 */
  int *n_res_kept;                     /* n_pts */
  unsigned char *point_dropped;        /* n_pts: 1 = the point lost all its residuals (Z6) */
  int *res_index_out;                  /* n_res: the residual's index among the kept ones, -1 if removed (Z7) */
  int *point_index_out;                /* n_pts: the point's index among those not dropped, -1 if dropped */
  int *n_res_out, *n_pts_out;          /* one word each */
  float *rmse;                         /* one word (Z8) */
  int *lost;                           /* one word */
  double *cam_to_world_out;            /* optional (NULL), n * 7: PRE_camToWorld at the new evaluation point */
  float *J_out;                        /* optional (NULL), n_res * 74: the rows of the final linearisation (not written for a residual that ends OOB) */
} dsm_finish_job;

/* The loop of dsm_window_optimize_batch and, behind the call's last pass, four more launches on the same arena (fin_frame_kernel:
 * Z1-Z3; linearize_kernel with the fix flag: Z4; fin_point_kernel: Z5, Z6; fin_prefix_kernel: B1, Z7, Z8), which write only a region
 * of their own.  They run once: with force_accept every job's pass count is known in advance and the call has ONE host wait; otherwise
 * they follow the read-back that tells whether a job needs the remaining passes, and the call has two.  B2 of the final linearisation is formed on the host from the
 * read-back, as dsm_linearize_residuals_batch forms it.  A job's results do not depend on the other jobs of the call or on the launch
 * geometry.  Validation is all or nothing, before anything is enqueued and with no output touched: DSM_ERR_INVALID for everything
 * dsm_window_optimize_batch refuses, a NULL required array, a last_res outside [-1, n_res) or naming a residual of another point, a
 * last_state_in other than DSM_RES_IN / _OOB / _OUTLIER, a negative n_good_residuals_in, a non-finite max_rel_baseline_in.  n_res == 0,
 * n_pts == 0, a job of one frame and a newest frame that hosts nothing are valid. */
int dsm_window_finish_batch(dsm_context *ctx, int n_jobs, const dsm_finish_job *jobs, const dsm_linearize_params *lp,
                            const dsm_step_params *sp, const dsm_optimize_params *op);
/* The same for one job on the host: dsm_window_optimize_host, plain loops over Z1-Z3, dsm_linearize_residuals_host, plain loops over
 * Z5-Z8.  A checker that needs no device. */
int dsm_window_finish_host(int w, int h, const dsm_finish_job *job, const float *const *frame_I, const dsm_linearize_params *lp,
                           const dsm_step_params *sp, const dsm_optimize_params *op);

/* DIAGNOSTIC, not a maintained interface (tools/finish_timing.py's route before): the host form's two halves on their own, for a
 * run of the loop and of the final linearisation as separate calls: after
 * dsm_window_optimize_batch (or _host) has filled job->opt's outputs, _prepare_host forms Z1-Z3 into the job's outputs and fills *lin
 * with the final linearisation's job (fix_linearization = 1; its tables are the job's pre_*_out arrays, its outputs the job's;
 * frame_energy_th and the scaled depths go to scratch, n + n_pts floats, which must outlive the use of *lin); the caller runs
 * dsm_linearize_residuals_batch (or _host) on *lin; _book_host then forms Z5-Z8 from the job's filled new_state, keep, rel_bs and
 * energy.  Plain loops on one core; DSM_ERR_INVALID for what V refuses. */
int dsm_diag_finish_prepare_host(const dsm_finish_job *job, const dsm_linearize_params *lp, const dsm_step_params *sp, float *scratch,
                                   dsm_linearize_job *lin);
int dsm_diag_finish_book_host(const dsm_finish_job *job);

/* ---- The window's nullspaces and their pseudo-inverse ------------------------------------------------------------
 * replaces what FrontEnd::solveSystem does before every solve (dso_helpers/FrontEndOptimize.cpp:488-494): getNullspaces (:525-574) with
 * what feeds it and what reads it -- the frames' numeric nullspaces that FrameHessian::setStateZero recomputes whenever a state_zero
 * moves (setEvalPT of the newest frame, section 22 Z1), and the basis N with its pseudo-inverse that EnergyFunctional::orthogonalize
 * forms from the pose and scale vectors (SOLVER_ORTHOGONALIZE_X_LATER, rule F7 of section 18).  getNullspaces is under the reference
 * tree and followed line for line; setStateZero, orthogonalize, Sophus and Eigen are not: parity is unpinned, and the rules G1-G7 and V
 * of DESIGN.md section 23 are the project's statement.  From the evaluation poses that dsm_window_finish_batch returns, the call
 * produces the null_basis / null_pinv (n_null = 7) that the next keyframe's dsm_solve_job reads.
 * NOT here: the H projections of SOLVER_ORTHOGONALIZE_SYSTEM / _POINTMARG / _FULL, upstream's symmetrised projector, a call from
 * inside dsm_window_finish_batch, flagFramesForMarginalization.
 * All arithmetic is IEEE double, left to right as written, without contraction. */
typedef struct dsm_nullspace_params {
  int struct_size;          /* sizeof(dsm_nullspace_params) */
  double scale_xi_trans;    /* 0.5   SCALE_XI_TRANS */
  double scale_xi_rot;      /* 1     SCALE_XI_ROT */
  double scale_a;           /* 10    SCALE_A */
  double scale_b;           /* 1000  SCALE_B */
  double solver_mode_delta; /* 1e-5  setting_solverModeDelta */
} dsm_nullspace_params;

#define DSM_NULLSPACE_NONFINITE 1    /* flags: an entry of null_basis, null_pinv or sing is not finite */
#define DSM_NULLSPACE_SWEEP_CAP 2    /* the Jacobi iteration still rotated in its last allowed sweep */
#define DSM_NULLSPACE_UNNORMALISED 4 /* a column whose sum of squares is not > 0 was left as it is (G5) */

/* One window; n = n_frames, N = 4 + 8 n; poses are {qx,qy,qz,qw,tx,ty,tz}. */
typedef struct dsm_nullspace_job {
  int n_frames;                    /* 1 .. DSM_WINDOW_MAX_FRAMES */
  const double *world_to_cam_eval; /* n * 7: worldToCam_evalPT, unit quaternions (as dsm_step_job) */
  const double *state_zero;        /* n * 8, unscaled; only entry 6 of a frame is read */
  const float *exposure;           /* n: ab_exposure, positive */
  const double *frame_null_in;     /* optional (NULL), n * 42: per frame a 6 x 7 block, row-major; columns 0-5 nullspaces_pose,
                                      column 6 nullspaces_scale.  Given: G1 and G2 are skipped and the block is used as it is */
  double *null_basis;              /* N * 7, row-major: what F7 reads */
  double *null_pinv;               /* 7 * N */
  double *sing;                    /* 7: the singular values, in column order after G6 */
  int *rank;                       /* one word: the singular values kept */
  int *flags;                      /* one word: DSM_NULLSPACE_* */
  double *frame_null_out;          /* optional (NULL), n * 42: the blocks used */
  double *null_x0_pre;             /* optional (NULL), N * 9: getNullspaces' return value in its own order (pose 0-5, affA, affB,
                                      scale), not normalised */
} dsm_nullspace_job;

/* the defaults listed above, struct_size set */
int dsm_nullspace_params_default(dsm_nullspace_params *p);
/* G1-G7 for every job: one staged copy, ONE launch (nsp_kernel, one 256-lane workgroup per job), one read-back.  params NULL: the
 * defaults.  A job's results do not depend on the other jobs of the call or on the launch geometry.  Validation is all or nothing,
 * before anything is enqueued and with no output touched: DSM_ERR_INVALID for a NULL required array, n_frames outside
 * [1, DSM_WINDOW_MAX_FRAMES], a world_to_cam_eval quaternion whose squared norm is further than 1e-9 from 1, a non-finite input or
 * parameter, a non-positive exposure, a non-positive scale or delta, a struct_size that is not this struct's. */
int dsm_window_nullspace_batch(dsm_context *ctx, int n_jobs, const dsm_nullspace_job *jobs, const dsm_nullspace_params *params);
/* The same on the host, job after job: plain loops over the same nullspace_math.hpp.  The CPU baseline of tools/nullspace_timing.py
 * and a checker that needs no device. */
int dsm_window_nullspace_host(int n_jobs, const dsm_nullspace_job *jobs, const dsm_nullspace_params *params);

/* ---- Adopting the stereo scale into the window ---------------------------------------------------------------------
 * replaces what FrontEnd::makeKeyFrame does between removeOutliers and flagPointsForRemoval (FrontEnd.cpp:806): FrontEnd::optimizeScale
 * behind its scale search (FrontEnd.cpp:1010-1061) -- the accept / reject decision with its trapped and fail-count state (function
 * statics there, per job here), the division of every active point's inverse depth by the accepted scale, the newest keyframe's
 * translation to its tracking reference scaled and its pose and evaluation point rebuilt from the reference's pose, and
 * setPrecalcValues -- as the rules S0-S6 and V of DESIGN.md section 25 state them.  The cited lines are followed literally; setIdepth,
 * setIdepthZero, setEvalPT_scaled and setStateScaled are UPSTREAM-DSO and not under the reference tree: parity is unpinned.  The
 * call sits between dsm_window_finish_batch and dsm_window_marginalize_batch / dsm_window_nullspace_batch and returns every array it
 * changes in the shape those calls and the next keyframe's dsm_step_job take it.
 * NOT here: the scale search (dsm_optimize_scale_batch, dsm_tracker_optimize_scale_guesses), scaleCoarseDepthL0 (:1032, the tracker's),
 * setAdjointsF at the rescaled pose, rescaling immature points, H_M / b_M or the other frames (the reference does none of these),
 * flagFramesForMarginalization.
 * All arithmetic is IEEE, left to right as written, without contraction. */
#define DSM_RESCALE_DISABLED 0
#define DSM_RESCALE_REJECTED 1
#define DSM_RESCALE_ACCEPTED 2

/* One window as dsm_window_finish_batch left it (after the caller erased what the finish removed); n = n_frames, N = 4 + 8 n; poses are
 * {qx,qy,qz,qw,tx,ty,tz}; the newest frame is n - 1.  Every array is required unless it says optional. */
typedef struct dsm_rescale_job {
  int n_frames;                     /* 1 .. DSM_WINDOW_MAX_FRAMES */
  int n_pts;                        /* >= 0: the active points of the whole window */
  int enabled;                      /* 0: scale_opt_thres_ <= 0 or fewer than five keyframes (FrontEnd.cpp:806) */
  float scale_error;                /* what the scale call returned; -1 when no guess gave a positive error.  NaN is valid and rejects */
  float new_scale;                  /* finite, not 0 */
  float thres;                      /* scale_opt_thres_ */
  int trapped, fails;               /* scale_trapped, scale_opt_fails before the call */
  const float *idepth;              /* the next four: n_pts each.  ph->idepth */
  const float *idepth_scaled;
  const float *idepth_zero_scaled;
  const float *delta;               /* EFPoint::deltaF */
  const double *world_to_cam_eval;  /* n * 7: worldToCam_evalPT, unit quaternions */
  const double *state;              /* n * 8, unscaled */
  const double *state_zero;         /* n * 8, unscaled */
  const float *exposure;            /* n: ab_exposure */
  const double *cam_to_tracking_ref; /* 7: the newest frame's shell->camToTrackingRef, as tracked */
  const double *ref_cam_to_world;   /* 7: shell->trackingRef->camToWorld */
  const double *cam_to_world;       /* 7: the newest frame's shell->camToWorld (copied through when not accepted) */
  double aff_g2l[2];                /* shell->aff_g2l: (state[n-1][6] * scale_a, state[n-1][7] * scale_b) of the finished window */
  const double *calib_value;        /* 4: h_calib_.value, unscaled */
  const double *calib_zero;         /* 4: value_zero */
  const double *ad_host, *ad_target; /* n * n * 8 * 8 each, as dsm_hessian_job reads them: NOT recomputed (S4) */
  const float *pre_RTll_0, *pre_tTll_0, *pre_KRKiTll, *pre_KtTll, *pre_aff_mode, *pre_b0_mode; /* n * n * (9, 3, 9, 3, 2, 1): the tables given */
  const float *cam;                 /* 6: cam, cam_inv */
  const float *c_delta;             /* 4 */
  const double *delta_x;            /* N */
  const float *ad_ht_delta;         /* n * n * 8 */
  const double *world_to_cam;       /* n * 7: PRE_worldToCam */
  const double *cam_to_world_all;   /* optional (NULL) unless cam_to_world_out_all is given, n * 7: PRE_camToWorld */
  float *idepth_out, *idepth_scaled_out, *idepth_zero_scaled_out, *delta_out; /* n_pts each (S2) */
  double *world_to_cam_eval_out;    /* n * 7 (S3) */
  double *state_out;                /* n * 8 */
  double *state_zero_out;           /* n * 8 */
  double *cam_to_tracking_ref_out;  /* 7 */
  double *cam_to_world_out;         /* 7 */
  float *pre_RTll_0_out, *pre_tTll_0_out, *pre_KRKiTll_out, *pre_KtTll_out, *pre_aff_mode_out, *pre_b0_mode_out; /* (S4) */
  float *cam_out;                   /* 6 */
  float *c_delta_out;               /* 4 */
  double *delta_x_out;              /* N */
  float *ad_ht_delta_out;           /* n * n * 8 */
  double *world_to_cam_out;         /* n * 7 */
  double *cam_to_world_out_all;     /* optional (NULL), n * 7 */
  int *decision;                    /* one word each: DSM_RESCALE_* (S1) */
  float *scale_error_out;           /* what optimizeScale returns: -1 when disabled or after the sixth failure in a row */
  int *trapped_out, *fails_out;
  float *applied_scale;             /* new_scale when accepted, otherwise 1 */
} dsm_rescale_job;

/* S0-S6 for every job: the decisions during staging on the host, ONE staged copy of the accepted jobs, ONE launch (rsc_kernel: per
 * accepted job one workgroup with a lane per frame and per pair, and up to eight workgroups that stride over the points), one
 * read-back; a job that is not accepted gets its byte copies on the host and is not staged.  lp and sp NULL: the defaults.  A job's
 * results do not depend on the other jobs of the call or on the launch geometry.  Validation is all or nothing, before anything is
 * enqueued and with no output touched: DSM_ERR_INVALID for a NULL required array, n_frames outside [1, DSM_WINDOW_MAX_FRAMES], a
 * negative n_pts, a non-finite input (scale_error apart), a world_to_cam_eval, cam_to_tracking_ref, ref_cam_to_world or cam_to_world
 * quaternion whose squared norm is further than 1e-9 from 1, a new_scale that is not finite or 0, a negative fails, cam_to_world_out_all
 * without cam_to_world_all, parameters that are not finite and positive.  n_pts == 0 and a job of one frame are valid. */
int dsm_window_rescale_batch(dsm_context *ctx, int n_jobs, const dsm_rescale_job *jobs, const dsm_linearize_params *lp, const dsm_step_params *sp);
/* The same on the host, job after job: plain loops over the same rescale_math.hpp.  The CPU baseline of tools/rescale_timing.py and a
 * checker that needs no device. */
int dsm_window_rescale_host(int n_jobs, const dsm_rescale_job *jobs, const dsm_linearize_params *lp, const dsm_step_params *sp);
/* The launch geometry of rsc_kernel, for tests that choose point counts at its edges: the workgroup size and the points' grid stride */
int dsm_rescale_geometry(int *block, int *grid_stride);

/* ---- Admitting the new keyframe into the window -------------------------------------------------------------------
 * replaces the head of FrontEnd::makeKeyFrame (FrontEnd.cpp:722-762): the new frame's pose and evaluation point (:725-727),
 * flagFramesForMarginalization (dso_helpers/FrontEndMarginalize.cpp:62-146, called at :735 BEFORE the insertion), ef_->insertFrame
 * (:742: H_M, b_M grown by eight zero rows and columns, the frame's prior taken, setAdjointsF over all pairs), setPrecalcValues on
 * n + 1 frames (:744) and one forward residual of every active point against the new frame (:746-762) -- as the rules A1-A6 and V
 * of DESIGN.md section 26 state them.  The cited lines are followed literally; insertFrame, EFFrame::takeData, getPrior,
 * FrameFramePrecalc::set's distanceLL, setAdjointsF and setEvalPT_scaled are UPSTREAM-DSO and not under the reference tree: parity
 * is unpinned.  The call needs no adjoint input: it forms the adjoints of every pair.
 * NOT here: the first keyframes (initializeFromInitializer), erasing and renumbering after a marginalisation, connectivityMap,
 * merging the points dsm_activate_points_batch activates into the lists, dso_error, clearing is_new of old residuals.
 * All arithmetic is IEEE, left to right as written, without contraction. */
typedef struct dsm_admit_params {
  int min_frames;                  /* setting_minFrames, 5; >= 0 */
  int max_frames;                  /* setting_maxFrames, 7; >= 0 */
  int min_frame_age;               /* setting_minFrameAge, 1 */
  float min_points_remaining;      /* setting_minPointsRemaining, 0.05f */
  float max_log_aff_fac_in_window; /* setting_maxLogAffFacInWindow, 0.7f */
} dsm_admit_params;
void dsm_admit_params_default(dsm_admit_params *p);

/* One window BEFORE the admission; n = n_frames, N = 4 + 8 n; the new frame becomes frame n of n + 1, and the lists hold
 * n_res + n_pts residuals afterwards.  Poses are {qx,qy,qz,qw,tx,ty,tz}.  Every array is required unless it says optional; an array of
 * n_pts or n_res entries may be NULL when that count is 0. */
typedef struct dsm_admit_job {
  int n_frames;                     /* 1 .. DSM_WINDOW_MAX_FRAMES - 1 */
  int n_pts;                        /* >= 0: the active points of the whole window */
  int n_res;                        /* >= 0: their residuals, grouped by point in ascending point order (makeIDX's order) */
  int new_keyframe_id;              /* the new frame's frameID (:740) */
  float new_exposure;               /* its ab_exposure */
  float new_frame_energy_th;        /* its frameEnergyTH: the constructor's 8*8*8 (:770 assigns the value to itself) */
  double aff_g2l[2];                /* its shell->aff_g2l, as tracked */
  const double *world_to_cam_eval;  /* n * 7: worldToCam_evalPT, unit quaternions */
  const double *state;              /* n * 8, unscaled */
  const double *state_zero;         /* n * 8, unscaled */
  const float *exposure;            /* n: ab_exposure */
  const float *frame_energy_th;     /* n */
  const int *keyframe_id;           /* n: frameID */
  const int *n_points_in;           /* n: pointHessians.size() + immaturePoints.size() */
  const int *n_points_out;          /* n: pointHessiansMarginalized.size() + pointHessiansOut.size() */
  const double *ref_cam_to_world;   /* 7: shell->trackingRef->camToWorld */
  const double *cam_to_tracking_ref; /* 7: shell->camToTrackingRef */
  const double *new_frame_prior;    /* 8: getPrior of the new frame */
  const double *new_frame_prior_zero; /* 8 */
  const double *calib_value;        /* 4: h_calib_.value, unscaled */
  const double *calib_zero;         /* 4: value_zero */
  const double *H_M, *b_M;          /* optional (NULL: absent), N * N (row-major) and N */
  const double *H_L, *b_L;          /* optional, N * N and N */
  const double *prior, *prior_zero; /* optional, both or neither, N each: what dsm_step_job takes as state_prior, state_prior_zero */
  const int *host;                  /* n_pts */
  const int *last_res;              /* n_pts * 2: the residual index of lastResiduals[0].first, [1].first; -1: none */
  const unsigned char *last_state;  /* n_pts * 2: DSM_RES_* */
  const int *point;                 /* n_res, non-decreasing */
  const int *target;                /* n_res */
  const unsigned char *state_in;    /* n_res: DSM_RES_IN / _OOB / _OUTLIER */
  const float *energy_in;           /* n_res */
  const unsigned char *is_new;      /* n_res */
  double *world_to_cam_eval_out;    /* (n + 1) * 7 (A1) */
  double *state_out;                /* (n + 1) * 8 */
  double *state_zero_out;           /* (n + 1) * 8 */
  float *exposure_out;              /* n + 1 */
  float *frame_energy_th_out;       /* n + 1 */
  int *keyframe_id_out;             /* n + 1 */
  double *world_to_cam_out;         /* (n + 1) * 7: PRE_worldToCam (A2) */
  unsigned char *flagged_out;       /* n + 1: flaggedForMarginalization (A4); the new frame's is 0 */
  double *cam_to_world_out;         /* 7: the new frame's shell->camToWorld */
  float *pre_RTll_0_out, *pre_tTll_0_out, *pre_KRKiTll_out, *pre_KtTll_out, *pre_aff_mode_out, *pre_b0_mode_out; /* (n+1)^2 * (9, 3, 9, 3, 2, 1) */
  float *distance_ll_out;           /* optional (NULL), (n+1)^2 */
  float *cam_out;                   /* 6 */
  float *c_delta_out;               /* 4 */
  double *delta_x_out;              /* N + 8 */
  double *ad_host_out, *ad_target_out; /* (n+1)^2 * 8 * 8 each (A3) */
  float *ad_ht_delta_out;           /* (n+1)^2 * 8 */
  double *H_M_out, *b_M_out;        /* (N+8)^2 and N + 8; required where the input is given, not read otherwise (A5) */
  double *H_L_out, *b_L_out;        /* likewise */
  double *prior_out, *prior_zero_out; /* N + 8 each, likewise */
  double *frame_prior_out;          /* 8: the new EFFrame's prior */
  double *frame_delta_prior_out;    /* 8: its delta_prior */
  int *point_out, *target_out;      /* n_res + n_pts each (A6) */
  unsigned char *res_state_out;     /* n_res + n_pts */
  float *energy_out;                /* n_res + n_pts */
  unsigned char *is_new_out;        /* n_res + n_pts */
  int *res_index_out;               /* n_res: where each old residual stands */
  int *new_res_index_out;           /* n_pts: where each point's new residual stands */
  int *last_res_out;                /* n_pts * 2, in the new numbering */
  unsigned char *last_state_out;    /* n_pts * 2 */
  int *n_res_out;                   /* one word: n_res + n_pts */
  int *n_flagged;                   /* one word: the frames flagged */
  double *dist_score_out;           /* n: F2's score of a candidate, 0 otherwise and where F2 did not run */
} dsm_admit_job;

/* A1-A6 for every job: ONE staged copy, ONE launch (adm_kernel: per job one workgroup with a lane per frame and per pair, and up to
 * eight workgroups that stride over the residuals, the points and the grown matrices), one read-back.  lp, sp, ap NULL: the defaults.
 * A job's results do not depend on the other jobs of the call or on the launch geometry.  Validation is all or nothing, before
 * anything is enqueued and with no output touched: DSM_ERR_INVALID for a NULL required array, n_frames outside
 * [1, DSM_WINDOW_MAX_FRAMES - 1], a negative n_pts or n_res, a host, point or target out of range, a target equal to its point's host,
 * residuals not grouped by ascending point, a last_res that is out of range or names another point's residual, a state byte other than
 * DSM_RES_IN / _OOB / _OUTLIER, a non-finite input, a quaternion whose squared norm is further than 1e-9 from 1, a negative
 * n_points_in or n_points_out or a sum of the two that overflows, prior without prior_zero or the reverse, parameters that are not
 * finite, a negative min_frames or max_frames.  n_pts == 0, n_res == 0 and a window of one frame are valid. */
int dsm_window_admit_batch(dsm_context *ctx, int n_jobs, const dsm_admit_job *jobs, const dsm_linearize_params *lp, const dsm_step_params *sp,
                           const dsm_admit_params *ap);
/* The same on the host, job after job: plain loops over the same admit_math.hpp.  The CPU baseline of tools/admit_timing.py and a
 * checker that needs no device. */
int dsm_window_admit_host(int n_jobs, const dsm_admit_job *jobs, const dsm_linearize_params *lp, const dsm_step_params *sp, const dsm_admit_params *ap);
/* The launch geometry of adm_kernel, for tests that choose counts at its edges: the workgroup size and the lists' grid stride */
int dsm_admit_geometry(int *block, int *grid_stride);

/* replaces TrackerAndScaler::makeCoarseDepthL0 (TrackerAndScaler.cpp:143-315) for callers that hold
 * the active points as flat arrays: (pu,pv) = centerProjectedTo[0..1], pidepth = centerProjectedTo[2],
 * pweight = sqrtf(1e-3/(HdiF+1e-12)) (:155-158).  ref_dIp[lvl]: the keyframe's (I,dx,dy) pyramid.
 * Outputs: n_out[lvl] and the four template lists (capacity w_l*h_l each) -- exactly the arguments of
 * dsm_tracker_set_ref.  Host side in this round (row A4 / N3).
 * COORDINATES: as dsm_tracker_set_ref_from_points -- a point is accepted exactly when pu + 0.5f and pv + 0.5f are finite and
 * truncate toward zero into [0, w) x [0, h); anything else returns DSM_ERR_INVALID (outputs then unspecified). */
int dsm_make_coarse_depth_l0(int w, int h, int nlevels, int npts, const float *pu, const float *pv,
                             const float *pidepth, const float *pweight, const float *const *ref_dIp,
                             int *n_out, float *const *pc_u, float *const *pc_v, float *const *pc_idepth,
                             float *const *pc_color);

/* replaces the inner loop of search_sc (search_place.h:67-79): sparse merge-join distance of
 * two ScanContext signatures.  Host side by design (<= 3 candidates per query). */
float dsm_sc_distance(const int *sigA_idx, const double *sigA_val, int nA, const int *sigB_idx,
                      const double *sigB_val, int nB, int sc_width);
/* replaces search_sc (search_place.h:59-84) over caller supplied candidate signatures */
int dsm_search_sc(const int *sig_idx, const double *sig_val, int n_sig, int n_cand,
                  const int *cand_ids, const int *const *cand_idx, const double *const *cand_val,
                  const int *cand_n, int sc_width, int *res_idx, float *res_diff);

/* replaces the file output of LoopHandler::savePose (LoopHandler.cpp:59-80): writes n lines "incoming_id x y z" with six
 * significant digits (std::setprecision(6)) -- the dslam.txt (optimised poses, tfm_w_c.translation()) and sodso.txt
 * (trans_w_c_orig) trajectory surface of the reference.  t_wc: n x 3 doubles. */
int dsm_write_trajectory(const char *path, int n, const int *incoming_ids, const double *t_wc);

#ifdef __cplusplus
}
#endif
#endif /* DSM_HOTPATH_H */
