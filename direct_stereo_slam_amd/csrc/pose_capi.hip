// pose_capi.hip -- loop-closure pose estimation (row N2): PoseEstimator::estimate, PoseEstimator.cpp:298-506, as the single handle
// dsm_pose_estimator and as dsm_pose_batch, many matches in one call.  Both run the LM state machine through batch_capi.hip's run_lm_batch.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "dsm_internal.hpp"

using namespace dsm;

// what PoseEstimator::estimate hands back from a terminated problem (:466-505); every output but M may be NULL
static void read_pose_result(const LMState &S, int n_pts, double *M, float *pose_error, int *inlier_percent_out, int *ok) {
  { // refToNew_current.matrix(), :466
    const double x = S.cur[0], y = S.cur[1], z = S.cur[2], w = S.cur[3];
    M[0] = 1 - 2 * (y * y + z * z), M[1] = 2 * (x * y - z * w), M[2] = 2 * (x * z + y * w), M[3] = S.cur[4];
    M[4] = 2 * (x * y + z * w), M[5] = 1 - 2 * (x * x + z * z), M[6] = 2 * (y * z - x * w), M[7] = S.cur[5];
    M[8] = 2 * (x * z - y * w), M[9] = 2 * (y * z + x * w), M[10] = 1 - 2 * (x * x + y * y), M[11] = S.cur[6];
    M[12] = M[13] = M[14] = 0, M[15] = 1;
  }
  const float err = (float)S.last_residuals[0]; // :467
  if (pose_error) *pose_error = err;
  const bool aff_good = S.status == ST_GOOD;                                        // :469-482
  const bool low_res = err < 10.0f;                                                 // RES_THRES, PoseEstimator.h:26
  const int inlier_percent = 100 * float((int)S.last_inners[0]) / (float)n_pts;     // :486
  const bool enough_inlier = inlier_percent > 90;                                   // INNER_PERCENT, PoseEstimator.h:27
  if (inlier_percent_out) *inlier_percent_out = inlier_percent;
  if (ok) *ok = (aff_good && low_res && enough_inlier) ? 1 : 0;                     // :505
}

extern "C" {

int dsm_pose_estimator_create(dsm_context *ctx, int w, int h, int nlevels, const dsm_params *params,
                              dsm_pose_estimator **out) {
  if (!out) return invalid("dsm_pose_estimator_create: out is NULL");
  const double I4[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  const float k1[4] = {1, 1, 0, 0};
  dsm_tracker *t = nullptr;
  int rc = dsm_tracker_create(ctx, w, h, nlevels, I4, k1, params, &t);
  if (rc) return rc;
  // the loop-closure point set is the same on every level: give every level the level-0 capacity
  for (int l = 1; l < nlevels; l++) {
    hipFree(t->d_pts[l]);
    t->d_pts[l] = nullptr;
    hipError_t e = hipMalloc(&t->d_pts[l], sizeof(float4) * ((size_t)w * h + kTemplatePad));
    if (e == hipSuccess) e = hipMemsetAsync(t->d_pts[l], 0, sizeof(float4) * ((size_t)w * h + kTemplatePad), ctx->stream);
    if (e != hipSuccess) {
      dsm_tracker_destroy(t);
      DSM_HIP(e);
    }
    t->pts_cap[l] = w * h;
    t->desc.lv[l].pts = t->d_pts[l];
  }
  t->desc_dirty = true;
  {
    const hipError_t e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
      dsm_tracker_destroy(t);
      DSM_HIP(e);
    }
  }
  dsm_pose_estimator *pe = new dsm_pose_estimator();
  pe->t = t;
  *out = pe;
  return DSM_OK;
}

int dsm_pose_estimator_destroy(dsm_pose_estimator *pe) {
  if (!pe) return DSM_OK;
  dsm_tracker_destroy(pe->t);
  delete pe;
  return DSM_OK;
}

} // extern "C"

namespace dsm {
// The loading half of PoseEstimator::estimate (:306-319), shared by dsm_pose_estimator_estimate and dsm_diag_pose_estimator_eval:
// makeK(new_cam), the points narrowed to float, the reference with affine (0, 0), the new frame's pyramid
int pose_estimator_load(dsm_pose_estimator *pe, int n_pts, const double *xyz, const float *const *ref_colors, float ref_ab_exposure,
                               const float *const *new_dIp, float new_ab_exposure, const float new_cam[4]) {
  dsm_tracker *t = pe->t;
  int rc = dsm_tracker_make_k(t, new_cam[0], new_cam[1], new_cam[2], new_cam[3]); // makeK(new_cam), :306
  if (rc) return rc;
  pe->x.resize(n_pts), pe->y.resize(n_pts), pe->z.resize(n_pts);
  for (int i = 0; i < n_pts; i++) { // `float x = pts_[i].first(0)` ..., PoseEstimator.cpp:183-185
    pe->x[i] = (float)xyz[3 * i];
    pe->y[i] = (float)xyz[3 * i + 1];
    pe->z[i] = (float)xyz[3 * i + 2];
  }
  int n[DSM_MAX_LEVELS];
  const float *px[DSM_MAX_LEVELS], *py[DSM_MAX_LEVELS], *pz[DSM_MAX_LEVELS];
  for (int l = 0; l < t->nlevels; l++) {
    n[l] = n_pts; // the same point set on every level, one reference colour per level (:238)
    px[l] = pe->x.data(), py[l] = pe->y.data(), pz[l] = pe->z.data();
  }
  // the float4 template slot holds (x, y, z, refColor[lvl]); ref_aff_g2l_ = (0,0) (:317)
  rc = dsm_tracker_set_ref(t, 0, 0.0, 0.0, ref_ab_exposure, n, px, py, pz, ref_colors);
  if (rc) return rc;
  return dsm_tracker_upload_frame(t, DSM_SLOT_NEW_LEFT, new_dIp, new_ab_exposure);
}

} // namespace dsm

extern "C" {

int dsm_pose_estimator_estimate(dsm_pose_estimator *pe, int n_pts, const double *xyz, const float *const *ref_colors,
                                float ref_ab_exposure, const float *const *new_dIp, float new_ab_exposure,
                                const float new_cam[4], int coarsest_lvl, double ref_to_new_io[16], float *pose_error,
                                int *ok) {
  if (!pe || n_pts < 1 || !xyz || !ref_colors || !new_dIp || !new_cam || !ref_to_new_io)
    return invalid("dsm_pose_estimator_estimate: bad argument");
  dsm_tracker *t = pe->t;
  if (n_pts > t->w * t->h) return invalid("dsm_pose_estimator_estimate: more points than pixels");
  int rc = pose_estimator_load(pe, n_pts, xyz, ref_colors, ref_ab_exposure, new_dIp, new_ab_exposure, new_cam);
  if (rc) return rc;
  dsm_context *ctx = t->ctx;
  dsm_tracker *ts[1] = {t};
  rc = prepare_batch(ctx, 1, ts, 2);
  if (rc) return rc;
  double pose0[7];
  const double aff0[2] = {0.0, 0.0};
  se3_from_matrix(ref_to_new_io, pose0); // SE3(R, t) constructor, :321-322
  fill_track_start(ctx->lm.h_start[0], pose0, aff0, nullptr, coarsest_lvl);
  rc = run_lm_batch(ctx, 1, ts, 2, coarsest_lvl);
  if (rc) return rc;
  read_pose_result(ctx->lm.h_states[0], n_pts, ref_to_new_io, pose_error, nullptr, ok);
  return DSM_OK;
}

// ---- the batched form: PoseEstimator::estimate of many matches in one call ----
} // extern "C"

// One geometry, many jobs.  Device memory follows the points, not the pixels: the templates of a job are nlevels lists of
// n_pts + kTemplatePad float4 in one arena, its target one intensity plane per level in another (shared by the jobs that pass the same
// pyramid).  Both arenas, the staging of the inputs and the staging of imported pyramids grow on demand and are kept.
struct dsm_pose_batch {
  dsm_context *ctx = nullptr;
  int w = 0, h = 0, nlevels = 0;
  dsm_params params{};
  size_t plane_off[DSM_MAX_LEVELS] = {}, planes_floats = 0; // an intensity pyramid: plane_bytes() per level, each level 16-byte aligned
  size_t dip_off[DSM_MAX_LEVELS] = {}, dip_floats = 0;      // a staged (I, dx, dy) pyramid, likewise
  unsigned char *d_in = nullptr, *h_in = nullptr;           // descriptors, job tables, check counters, staged points and colours (device / pinned)
  size_t in_bytes = 0;
  float4 *d_tpl = nullptr;
  size_t tpl_entries = 0;
  float *d_img = nullptr;
  size_t img_slots = 0;
  float *d_dip = nullptr; // kPoseImportWave staged pyramids
  std::vector<dsm_tracker> trackers; // what run_lm_batch reads of a problem: geometry, parameters, the host copy of the descriptor
  std::vector<dsm_tracker *> ts;
};

namespace {
constexpr int kPoseImportWave = 8; // pyramids staged at a time: 12 B x sum of pixels each, whatever the batch size
size_t align16(size_t bytes) { return (bytes + 15) & ~(size_t)15; }
struct PosePyramid { // a distinct target pyramid of a call
  bool dip;
  const float *const *lv;
};
} // namespace

extern "C" {

int dsm_pose_batch_create(dsm_context *ctx, int w, int h, int nlevels, const dsm_params *params, dsm_pose_batch **out) {
  if (!out) return invalid("dsm_pose_batch_create: out is NULL");
  *out = nullptr;
  if (!ctx) return invalid("dsm_pose_batch_create: null context");
  if (nlevels < 1 || nlevels > DSM_MAX_LEVELS) return invalid("dsm_pose_batch_create: nlevels out of range");
  if ((w >> (nlevels - 1)) < 8 || (h >> (nlevels - 1)) < 8) return invalid("dsm_pose_batch_create: image too small for nlevels");
  if ((long long)w * h * 16 >= (1ll << 32)) return invalid("dsm_pose_batch_create: image too large");
  dsm_params P;
  const int rc = take_params(params, &P);
  if (rc) return rc;
  dsm_pose_batch *pb = new dsm_pose_batch();
  pb->ctx = ctx, pb->w = w, pb->h = h, pb->nlevels = nlevels, pb->params = P;
  for (int l = 0; l < nlevels; l++) {
    const size_t npx = (size_t)(w >> l) * (h >> l);
    pb->plane_off[l] = pb->planes_floats;
    pb->planes_floats += align16(plane_bytes(w >> l, h >> l)) / sizeof(float);
    pb->dip_off[l] = pb->dip_floats;
    pb->dip_floats += align16(npx * 12) / sizeof(float);
  }
  *out = pb;
  return DSM_OK;
}

int dsm_pose_batch_destroy(dsm_pose_batch *pb) {
  if (!pb) return DSM_OK;
  hipSetDevice(pb->ctx->device);
  hipStreamSynchronize(pb->ctx->stream);
  hipFree(pb->d_in);
  if (pb->h_in) hipHostFree(pb->h_in);
  hipFree(pb->d_tpl);
  hipFree(pb->d_img);
  hipFree(pb->d_dip);
  delete pb;
  return DSM_OK;
}

int dsm_pose_estimate_batch(dsm_pose_batch *pb, int n_jobs, const dsm_pose_job *jobs, int coarsest_lvl) {
  if (!pb || !jobs || n_jobs < 1) return invalid("dsm_pose_estimate_batch: null handle, null jobs or n_jobs < 1");
  dsm_context *ctx = pb->ctx;
  const int nl = pb->nlevels, n = n_jobs;
  if (coarsest_lvl < 0 || coarsest_lvl >= nl) return invalid("dsm_pose_estimate_batch: coarsest level out of range");
  // ---- all-or-nothing validation, and the call's distinct target pyramids ----
  std::vector<PosePyramid> pyr;
  std::vector<int> pyr_of(n);
  char msg[200];
  for (int j = 0; j < n; j++) {
    const dsm_pose_job &J = jobs[j];
    const char *what = nullptr;
    if (!J.xyz || !J.ref_colors || !J.ref_to_new_io || !J.ok) what = "a NULL pointer (xyz, ref_colors, ref_to_new_io, ok)";
    else if (J.n_pts < 1) what = "n_pts < 1";
    else if ((long long)J.n_pts > (long long)pb->w * pb->h) what = "more points than pixels";
    else if ((J.new_dIp != nullptr) == (J.new_I != nullptr)) what = "exactly one of new_dIp and new_I must be given";
    if (!what) {
      const float *const *lv = J.new_dIp ? J.new_dIp : J.new_I;
      for (int l = 0; l < nl && !what; l++)
        if (!J.ref_colors[l] || !lv[l]) what = "a NULL level pointer";
      for (int k = 0; k < 16 && !what; k++)
        if (!std::isfinite(J.ref_to_new_io[k])) what = "a non-finite guess";
      if (!what) {
        int p = -1;
        for (size_t q = 0; q < pyr.size() && p < 0; q++) {
          bool same = pyr[q].dip == (J.new_dIp != nullptr);
          for (int l = 0; l < nl && same; l++) same = pyr[q].lv[l] == lv[l];
          if (same) p = (int)q;
        }
        if (p < 0) {
          p = (int)pyr.size();
          pyr.push_back(PosePyramid{J.new_dIp != nullptr, lv});
        }
        pyr_of[j] = p;
      }
    }
    if (what) {
      snprintf(msg, sizeof msg, "dsm_pose_estimate_batch: job %d: %s", j, what);
      return invalid(msg);
    }
  }
  DSM_HIP(hipSetDevice(ctx->device));
  // ---- layout ----
  const size_t npyr = pyr.size();
  size_t nimp = 0;
  std::vector<int> imp_of(npyr, -1); // imported pyramids first come, first served
  for (size_t q = 0; q < npyr; q++)
    if (pyr[q].dip) imp_of[q] = (int)nimp++;
  const size_t desc_off = 0, pack_off = align16(desc_off + sizeof(TrackerDev) * n), imp_off = align16(pack_off + sizeof(PosePackJob) * n);
  const size_t bad_off = align16(imp_off + sizeof(PoseImportJob) * nimp);
  size_t in_need = align16(bad_off + sizeof(int) * 2 * DSM_MAX_LEVELS * nimp);
  size_t tpl_need = 0;
  std::vector<size_t> xyz_off(n), col_off(n), tpl_off(n);
  std::vector<const void *> dev_xyz(n, nullptr);
  std::vector<const void *> dev_col((size_t)n * DSM_MAX_LEVELS, nullptr);
  int max_n = 0;
  for (int j = 0; j < n; j++) {
    const dsm_pose_job &J = jobs[j];
    const size_t np = (size_t)J.n_pts;
    // page-locked caller arrays are read in place by the pack kernel; anything else goes through the staging buffer
    bool in_place = (dev_xyz[j] = pinned_device_pointer(J.xyz)) != nullptr;
    for (int l = 0; l < nl && in_place; l++) in_place = (dev_col[(size_t)j * DSM_MAX_LEVELS + l] = pinned_device_pointer(J.ref_colors[l])) != nullptr;
    if (!in_place) {
      dev_xyz[j] = nullptr;
      xyz_off[j] = in_need;
      in_need += align16(np * 3 * sizeof(double));
      col_off[j] = in_need;
      in_need += align16(np * sizeof(float)) * nl;
    }
    tpl_off[j] = tpl_need;
    tpl_need += (np + kTemplatePad) * nl;
    if (J.n_pts > max_n) max_n = J.n_pts;
  }
  // ---- arenas (a call ends with the stream idle: nothing reads the old ones) ----
  if (in_need > pb->in_bytes) {
    pb->in_bytes = 0;
    int rc = realloc_dev(&pb->d_in, in_need);
    if (!rc) rc = realloc_pinned(&pb->h_in, in_need);
    if (rc) return rc;
    pb->in_bytes = in_need;
  }
  if (tpl_need > pb->tpl_entries) {
    pb->tpl_entries = 0;
    const int rc = realloc_dev(&pb->d_tpl, tpl_need);
    if (rc) return rc;
    pb->tpl_entries = tpl_need;
  }
  if (npyr > pb->img_slots) {
    pb->img_slots = 0;
    const int rc = realloc_dev(&pb->d_img, npyr * pb->planes_floats);
    if (rc) return rc;
    DSM_HIP(hipMemsetAsync(pb->d_img, 0, npyr * pb->planes_floats * sizeof(float), ctx->stream)); // (the slack behind every plane)
    pb->img_slots = npyr;
  }
  if (nimp && !pb->d_dip) {
    const int rc = realloc_dev(&pb->d_dip, (size_t)kPoseImportWave * pb->dip_floats);
    if (rc) return rc;
  }
  // ---- the problems: descriptor, pack job and staged inputs of every job ----
  if ((int)pb->trackers.size() < n) pb->trackers.resize(n);
  pb->ts.resize(n);
  TrackerDev *h_desc = (TrackerDev *)(pb->h_in + desc_off), *d_desc = (TrackerDev *)(pb->d_in + desc_off);
  PosePackJob *h_pack = (PosePackJob *)(pb->h_in + pack_off);
  const double I4[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  const float k1[4] = {1, 1, 0, 0};
  for (int j = 0; j < n; j++) {
    const dsm_pose_job &J = jobs[j];
    const size_t np = (size_t)J.n_pts;
    TrackerDev D; // as dsm_pose_estimator_create + make_k + set_ref + upload_frame leave the single handle's
    desc_init(D, nl, pb->params);
    se3_from_matrix(I4, D.T10);
    desc_cam1(D, nl, k1);
    desc_make_k(D, nl, J.new_cam[0], J.new_cam[1], J.new_cam[2], J.new_cam[3]); // makeK(new_cam), :306
    PosePackJob &K = h_pack[j];
    memset(&K, 0, sizeof K);
    K.n = J.n_pts;
    const bool in_place = dev_xyz[j] != nullptr;
    K.xyz = in_place ? (const double *)dev_xyz[j] : (const double *)(pb->d_in + xyz_off[j]);
    if (!in_place) memcpy(pb->h_in + xyz_off[j], J.xyz, np * 3 * sizeof(double));
    float *planes = pb->d_img + (size_t)pyr_of[j] * pb->planes_floats;
    for (int l = 0; l < nl; l++) {
      const size_t co = col_off[j] + (size_t)l * align16(np * sizeof(float));
      K.col[l] = in_place ? (const float *)dev_col[(size_t)j * DSM_MAX_LEVELS + l] : (const float *)(pb->d_in + co);
      if (!in_place) memcpy(pb->h_in + co, J.ref_colors[l], np * sizeof(float));
      K.pts[l] = pb->d_tpl + tpl_off[j] + (size_t)l * (np + kTemplatePad);
      D.lv[l].w = pb->w >> l;
      D.lv[l].h = pb->h >> l;
      D.lv[l].pts = K.pts[l];
      D.lv[l].n = J.n_pts; // the same point set on every level, one reference colour per level (:238)
      D.lv[l].img[0] = D.lv[l].img[1] = planes + pb->plane_off[l];
    }
    D.ref_a = 0.0, D.ref_b = 0.0; // ref_aff_g2l_ = (0,0) (:317)
    D.ref_exposure = J.ref_ab_exposure;
    D.exposure[0] = J.new_ab_exposure;
    h_desc[j] = D;
    dsm_tracker &t = pb->trackers[j];
    t.ctx = ctx, t.w = pb->w, t.h = pb->h, t.nlevels = nl, t.params = pb->params;
    t.desc = D;
    t.d_desc = d_desc + j;
    t.have_k = t.have_ref = t.have_frame[0] = true;
    t.desc_dirty = false; // (the descriptor travels with the staged inputs)
    pb->ts[j] = &t;
  }
  PoseImportJob *h_imp = (PoseImportJob *)(pb->h_in + imp_off), *d_imp = (PoseImportJob *)(pb->d_in + imp_off);
  int *h_bad = (int *)(pb->h_in + bad_off), *d_bad = (int *)(pb->d_in + bad_off);
  for (size_t q = 0; q < npyr; q++) {
    if (!pyr[q].dip) continue;
    const int k = imp_of[q];
    PoseImportJob &M = h_imp[k];
    memset(&M, 0, sizeof M);
    for (int l = 0; l < nl; l++) {
      M.in3[l] = pb->d_dip + (size_t)(k % kPoseImportWave) * pb->dip_floats + pb->dip_off[l];
      M.plane[l] = pb->d_img + q * pb->planes_floats + pb->plane_off[l];
    }
    M.bad = d_bad + 2 * DSM_MAX_LEVELS * k;
    for (int l = 0; l < DSM_MAX_LEVELS; l++) h_bad[2 * DSM_MAX_LEVELS * k + 2 * l] = 0, h_bad[2 * DSM_MAX_LEVELS * k + 2 * l + 1] = 0x7FFFFFFF;
  }
  int rc = prepare_batch(ctx, n, pb->ts.data(), 2);
  if (rc) return rc;
  const double aff0[2] = {0.0, 0.0};
  for (int j = 0; j < n; j++) {
    double pose0[7];
    se3_from_matrix(jobs[j].ref_to_new_io, pose0); // SE3(R, t) constructor, :321-322
    fill_track_start(ctx->lm.h_start[j], pose0, aff0, nullptr, coarsest_lvl);
  }
  // ---- one transfer, one pack launch, the targets, one LM run ----
  DSM_HIP(hipMemcpyAsync(pb->d_in, pb->h_in, in_need, hipMemcpyHostToDevice, ctx->stream));
  launch_pose_pack(ctx->stream, (const PosePackJob *)(pb->d_in + pack_off), n, nl, max_n);
  const bool check = pb->params.frame_check != 0;
  std::vector<int> wave; // pyramids (indices into pyr) of the wave being staged
  for (size_t q = 0; q < npyr; q++) {
    for (int l = 0; l < nl; l++) {
      const size_t npx = (size_t)(pb->w >> l) * (pb->h >> l);
      if (pyr[q].dip)
        DSM_HIP(hipMemcpyAsync(pb->d_dip + (size_t)(imp_of[q] % kPoseImportWave) * pb->dip_floats + pb->dip_off[l], pyr[q].lv[l], npx * 12,
                               hipMemcpyHostToDevice, ctx->stream));
      else
        DSM_HIP(hipMemcpyAsync(pb->d_img + q * pb->planes_floats + pb->plane_off[l], pyr[q].lv[l], npx * sizeof(float), hipMemcpyHostToDevice,
                               ctx->stream));
    }
    if (pyr[q].dip) wave.push_back((int)q);
    if (!wave.empty() && ((int)wave.size() == kPoseImportWave || q + 1 == npyr)) { // (import jobs are numbered in the order they are staged)
      launch_pose_import(ctx->stream, d_imp + imp_of[wave[0]], (int)wave.size(), pb->w, pb->h, nl, check, pb->params.frame_grad_tol);
      wave.clear();
    }
  }
  DSM_HIP(hipGetLastError());
  if (check && nimp) DSM_HIP(hipMemcpyAsync(h_bad, d_bad, sizeof(int) * 2 * DSM_MAX_LEVELS * nimp, hipMemcpyDeviceToHost, ctx->stream));
  rc = run_lm_batch(ctx, n, pb->ts.data(), 2, coarsest_lvl); // (ends with the stream idle: the check's counters are home as well)
  if (rc) return rc;
  for (int j = 0; check && j < n; j++) {
    const int k = imp_of[pyr_of[j]];
    for (int l = 0; k >= 0 && l < nl; l++) {
      const int *bad = h_bad + 2 * DSM_MAX_LEVELS * k + 2 * l;
      if (!bad[0]) continue;
      const int wl = pb->w >> l, idx = bad[1];
      char m[360];
      snprintf(m, sizeof m,
               "dsm_pose_estimate_batch: job %d: level %d: %d texel(s) whose gradient channels are not the central differences of channel 0 "
               "(makeImages), the first at index %d (x = %d, y = %d); see dsm_params.frame_check / frame_grad_tol",
               j, l, bad[0], idx, idx % wl, idx / wl);
      return invalid(m);
    }
  }
  for (int j = 0; j < n; j++)
    read_pose_result(ctx->lm.h_states[j], jobs[j].n_pts, jobs[j].ref_to_new_io, jobs[j].pose_error, jobs[j].inlier_percent, jobs[j].ok);
  return DSM_OK;
}

} // extern "C"
