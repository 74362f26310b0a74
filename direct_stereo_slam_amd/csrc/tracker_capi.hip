// tracker_capi.hip -- the tracker handle (dsm_tracker_*): its device descriptor piece by piece, the templates, the single-frame
// uploads and read-backs.  Host side only orchestrates; the kernels are template_kernels.hip's and frame_kernels.hip's.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "call_arena.hpp"
#include "dsm_internal.hpp"

namespace dsm {

// One intensity plane of a w x h level.  Lanes whose point is not usable fetch their twelve taps around texel (2, 2)
// instead (rows 1-4, columns 1-4), always inside the image (dsm_tracker_create wants a coarsest level of at least 8 x 8);
// the four rows and few texels of slack are belt and braces.
size_t plane_bytes(int w, int h) { return sizeof(float) * ((size_t)w * h + 4 * (size_t)w + 16); }

int sync_desc(dsm_tracker *t) {
  if (!t->desc_dirty) return DSM_OK;
  DSM_HIP(hipMemcpyAsync(t->d_desc, &t->desc, sizeof(TrackerDev), hipMemcpyHostToDevice, t->ctx->stream));
  // the host copy may change again before the copy engine reads it
  DSM_HIP(hipStreamSynchronize(t->ctx->stream));
  t->desc_dirty = false;
  return DSM_OK;
}

// the same for a batch: all changed descriptors through one pinned staging buffer, one copy and one scatter launch
int sync_descs(dsm_context *ctx, dsm_tracker *const *ts, int n) {
  int dirty = 0;
  for (int i = 0; i < n; i++) dirty += ts[i]->desc_dirty ? 1 : 0;
  if (dirty <= 2) {
    for (int i = 0; i < n; i++) {
      int rc = sync_desc(ts[i]);
      if (rc) return rc;
    }
    return DSM_OK;
  }
  const size_t per = sizeof(TrackerDev) + sizeof(TrackerDev *);
  if (dirty > ctx->descs.desc_stage_cap) {
    if (ctx->descs.desc_stage_busy) DSM_HIP(hipEventSynchronize(ctx->descs.desc_event));
    ctx->descs.desc_stage_busy = false;
    int rc = realloc_dev(&ctx->descs.d_desc_stage, per * dirty);
    if (rc) return rc;
    rc = realloc_pinned(&ctx->descs.h_desc_stage, per * dirty);
    if (rc) return rc;
    ctx->descs.desc_stage_cap = dirty;
  }
  if (!ctx->descs.desc_event) DSM_HIP(hipEventCreateWithFlags(&ctx->descs.desc_event, hipEventDisableTiming));
  if (ctx->descs.desc_stage_busy) DSM_HIP(hipEventSynchronize(ctx->descs.desc_event)); // the previous copy still reads the buffer
  TrackerDev *hd = (TrackerDev *)ctx->descs.h_desc_stage;
  TrackerDev **hp = (TrackerDev **)(ctx->descs.h_desc_stage + sizeof(TrackerDev) * dirty);
  int k = 0;
  for (int i = 0; i < n; i++) {
    if (!ts[i]->desc_dirty) continue;
    bool seen = false; // the same tracker twice in a batch (hypotheses)
    for (int j = 0; j < k && !seen; j++) seen = hp[j] == ts[i]->d_desc;
    if (seen) continue;
    hd[k] = ts[i]->desc;
    hp[k] = ts[i]->d_desc;
    k++;
  }
  DSM_HIP(hipMemcpyAsync(ctx->descs.d_desc_stage, ctx->descs.h_desc_stage, per * dirty, hipMemcpyHostToDevice, ctx->stream));
  launch_desc_scatter(ctx->stream, k, (const TrackerDev *)ctx->descs.d_desc_stage,
                      (TrackerDev *const *)(ctx->descs.d_desc_stage + sizeof(TrackerDev) * dirty));
  DSM_HIP(hipGetLastError());
  DSM_HIP(hipEventRecord(ctx->descs.desc_event, ctx->stream));
  ctx->descs.desc_stage_busy = true;
  for (int i = 0; i < n; i++) ts[i]->desc_dirty = false;
  return DSM_OK;
}

// ---- small host math (float, contraction off): makeK, TrackerAndScaler.cpp:117-141 ----
static float cof3(const float *m, int i, int j) {
  const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
  return m[i1 * 3 + j1] * m[i2 * 3 + j2] - m[i1 * 3 + j2] * m[i2 * 3 + j1];
}
static void mat3f_inverse(const float *m, float *r) { // Eigen Matrix3f::inverse(), cofactor form
  const float c0 = cof3(m, 0, 0), c1 = cof3(m, 1, 0), c2 = cof3(m, 2, 0);
  const float det = (c0 * m[0] + c1 * m[3]) + c2 * m[6];
  const float invdet = 1.0f / det;
  r[0] = c0 * invdet;
  r[1] = c1 * invdet;
  r[2] = c2 * invdet;
  r[3] = cof3(m, 0, 1) * invdet;
  r[4] = cof3(m, 1, 1) * invdet;
  r[5] = cof3(m, 2, 1) * invdet;
  r[6] = cof3(m, 0, 2) * invdet;
  r[7] = cof3(m, 1, 2) * invdet;
  r[8] = cof3(m, 2, 2) * invdet;
}

// SE3(Matrix4d) of Sophus/Eigen for tfm_f1_f0_ (TrackerAndScaler.cpp:82-86)
void se3_from_matrix(const double T[16], double pose[7]) {
  const double M[3][3] = {{T[0], T[1], T[2]}, {T[4], T[5], T[6]}, {T[8], T[9], T[10]}};
  double q[4];
  double t = M[0][0] + M[1][1] + M[2][2];
  if (t > 0.0) {
    t = std::sqrt(t + 1.0);
    q[3] = 0.5 * t;
    t = 0.5 / t;
    q[0] = (M[2][1] - M[1][2]) * t;
    q[1] = (M[0][2] - M[2][0]) * t;
    q[2] = (M[1][0] - M[0][1]) * t;
  } else {
    int i = 0;
    if (M[1][1] > M[0][0]) i = 1;
    if (M[2][2] > M[i][i]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    t = std::sqrt(M[i][i] - M[j][j] - M[k][k] + 1.0);
    q[i] = 0.5 * t;
    t = 0.5 / t;
    q[3] = (M[k][j] - M[j][k]) * t;
    q[j] = (M[j][i] + M[i][j]) * t;
    q[k] = (M[k][i] + M[i][k]) * t;
  }
  const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  for (int i = 0; i < 4; i++) pose[i] = q[i] / n;
  pose[4] = T[3];
  pose[5] = T[7];
  pose[6] = T[11];
}

// ---- the device descriptor of a tracker, piece by piece (dsm_tracker_*; dsm_pose_estimate_batch builds its jobs' descriptors from the same pieces) ----
void desc_init(TrackerDev &D, int nlevels, const dsm_params &P) {
  memset(&D, 0, sizeof D);
  D.nlevels = nlevels;
  D.p.huber_th = P.huber_th;
  D.p.coarse_cutoff_th = P.coarse_cutoff_th;
  D.p.scale_xi_rot = P.scale_xi_rot;
  D.p.scale_xi_trans = P.scale_xi_trans;
  D.p.scale_a = P.scale_a;
  D.p.scale_b = P.scale_b;
  D.p.affine_opt_mode_a = P.affine_opt_mode_a;
  D.p.affine_opt_mode_b = P.affine_opt_mode_b;
  D.p.lambda_extrapolation_limit = P.lambda_extrapolation_limit;
  for (int l = 0; l < DSM_MAX_LEVELS; l++) D.p.max_iterations[l] = P.max_iterations[l];
  D.p.fixed_schedule = P.fixed_schedule;
  D.p.geometry = P.chunk_geometry;
}
// camera 1 pyramid, TrackerAndScaler.cpp:89-98
void desc_cam1(TrackerDev &D, int nlevels, const float K1[4]) {
  D.lv[0].fx1 = K1[0];
  D.lv[0].fy1 = K1[1];
  D.lv[0].cx1 = K1[2];
  D.lv[0].cy1 = K1[3];
  for (int l = 1; l < nlevels; l++) {
    D.lv[l].fx1 = D.lv[l - 1].fx1 * 0.5;
    D.lv[l].fy1 = D.lv[l - 1].fy1 * 0.5;
    D.lv[l].cx1 = (D.lv[0].cx1 + 0.5) / ((int)1 << l) - 0.5;
    D.lv[l].cy1 = (D.lv[0].cy1 + 0.5) / ((int)1 << l) - 0.5;
  }
}
// makeK, TrackerAndScaler.cpp:117-141
void desc_make_k(TrackerDev &D, int nlevels, float fx, float fy, float cx, float cy) {
  D.lv[0].fx = fx;
  D.lv[0].fy = fy;
  D.lv[0].cx = cx;
  D.lv[0].cy = cy;
  for (int l = 1; l < nlevels; l++) { // :126-133
    D.lv[l].fx = D.lv[l - 1].fx * 0.5;
    D.lv[l].fy = D.lv[l - 1].fy * 0.5;
    D.lv[l].cx = (D.lv[0].cx + 0.5) / ((int)1 << l) - 0.5;
    D.lv[l].cy = (D.lv[0].cy + 0.5) / ((int)1 << l) - 0.5;
  }
  for (int l = 0; l < nlevels; l++) { // :135-140
    const float K[9] = {D.lv[l].fx, 0.0f, D.lv[l].cx, 0.0f, D.lv[l].fy, D.lv[l].cy, 0.0f, 0.0f, 1.0f};
    mat3f_inverse(K, D.lv[l].Ki);
  }
}

int check_ready(dsm_tracker *t, int mode) {
  if (!t->have_k || !t->have_ref || !t->have_frame[mode == 1 ? 1 : 0]) {
    set_error(mode ? "optimize_scale needs make_k, set_ref and the right frame (slot 1)"
                   : "track needs make_k, set_ref and the new left frame (slot 0)");
    return DSM_ERR_STATE;
  }
  return DSM_OK;
}

} // namespace dsm

// ---- the owner of the facts (dsm_internal.hpp): the only writers of the words from the host side ----
int dsm_tracker::announce_template_write(hipStream_t s, FactUse use) {
  dsm::launch_facts_set(s, facts.d, (1 << nlevels) - 1, -1, 0, use == kFactArm ? 1 : 0);
  DSM_HIP(hipGetLastError());
  return DSM_OK;
}
int dsm_tracker::announce_plane_write(int slot, hipStream_t s, FactUse use) {
  dsm::launch_facts_set(s, facts.d, 0, facts.set_of(slot), (1 << nlevels) - 1, use == kFactArm ? 1 : 0);
  DSM_HIP(hipGetLastError());
  return DSM_OK;
}

using namespace dsm;

extern "C" {

// ---- tracker ------------------------------------------------------------------------------
static int tracker_create_fill(dsm_tracker *t, dsm_context *ctx, int w, int h, int nlevels, const double T_f1_f0[16],
                               const float K1[4], const dsm_params *params);

int dsm_tracker_create(dsm_context *ctx, int w, int h, int nlevels, const double T_f1_f0[16],
                       const float K1[4], const dsm_params *params, dsm_tracker **out) {
  if (!ctx || !out || !T_f1_f0 || !K1) return invalid("dsm_tracker_create: null argument");
  if (nlevels < 1 || nlevels > DSM_MAX_LEVELS) return invalid("dsm_tracker_create: nlevels out of range");
  if ((w >> (nlevels - 1)) < 8 || (h >> (nlevels - 1)) < 8) return invalid("dsm_tracker_create: image too small for nlevels");
  // the eval kernels address texels with 32-bit byte offsets (16 bytes per texel at most)
  if ((long long)w * h * 16 >= (1ll << 32)) return invalid("dsm_tracker_create: image too large");
  DSM_HIP(hipSetDevice(ctx->device));
  dsm_tracker *t = new dsm_tracker();
  const int rc = tracker_create_fill(t, ctx, w, h, nlevels, T_f1_f0, K1, params);
  if (rc != DSM_OK) { // e.g. out of device memory half way: give back what was allocated (hipFree(nullptr) is a no-op)
    const std::string keep = dsm_last_error();
    dsm_tracker_destroy(t);
    set_error(keep);
    return rc;
  }
  *out = t;
  return DSM_OK;
}

static int tracker_create_fill(dsm_tracker *t, dsm_context *ctx, int w, int h, int nlevels, const double T_f1_f0[16],
                               const float K1[4], const dsm_params *params) {
  t->ctx = ctx;
  t->w = w;
  t->h = h;
  t->nlevels = nlevels;
  const int prc = take_params(params, &t->params);
  if (prc) return prc;
  TrackerDev &D = t->desc;
  desc_init(D, nlevels, t->params);
  se3_from_matrix(T_f1_f0, D.T10);
  for (int l = 0; l < nlevels; l++) { // TrackerAndScaler.cpp:52-64
    const int wl = w >> l, hl = h >> l;
    D.lv[l].w = wl;
    D.lv[l].h = hl;
    DSM_HIP(hipMalloc(&t->d_pts[l], sizeof(float4) * ((size_t)wl * hl + kTemplatePad)));
    DSM_HIP(hipMemsetAsync(t->d_pts[l], 0, sizeof(float4) * ((size_t)wl * hl + kTemplatePad), ctx->stream)); // (not the null stream: streams_overlap)
    t->pts_cap[l] = wl * hl;
    for (int s = 0; s < 2; s++) {
      DSM_HIP(hipMalloc(&t->d_img[s][l], plane_bytes(wl, hl)));
      DSM_HIP(hipMemsetAsync(t->d_img[s][l], 0, plane_bytes(wl, hl), ctx->stream));
      D.lv[l].img[s] = t->d_img[s][l];
    }
    D.lv[l].pts = t->d_pts[l];
    D.lv[l].n = 0;
  }
  desc_cam1(D, nlevels, K1);
  DSM_HIP(hipMalloc(&t->facts.d, sizeof(TrackerFacts)));
  DSM_HIP(hipMemsetAsync(t->facts.d, 0, sizeof(TrackerFacts), ctx->stream)); // nothing established
  D.facts = t->facts.d;
  D.img_set[0] = t->facts.set[0], D.img_set[1] = t->facts.set[1];
  DSM_HIP(hipMalloc(&t->d_desc, sizeof(TrackerDev)));
  t->desc_dirty = true;
  DSM_HIP(hipStreamSynchronize(ctx->stream)); // the zero fills are through before any other stream may write these buffers
  return DSM_OK;
}

int dsm_tracker_destroy(dsm_tracker *t) {
  if (!t) return DSM_OK;
  hipSetDevice(t->ctx->device);
  (void)t->ctx->handover.drain(t->ctx->stream); // an asynchronous hand-over may still write its buffers
  for (int l = 0; l < t->nlevels; l++) {
    hipFree(t->d_pts[l]);
    hipFree(t->d_img[0][l]);
    hipFree(t->d_img[1][l]);
  }
  hipFree(t->d_raw[0]);
  hipFree(t->d_raw[1]);
  for (int s = 0; s < 2; s++) {
    hipFree(t->d_raw_back[s]);
    for (int l = 0; l < DSM_MAX_LEVELS; l++) hipFree(t->d_img_back[s][l]);
  }
  hipFree(t->d_desc);
  hipFree(t->facts.d);
  delete t;
  return DSM_OK;
}

int dsm_tracker_make_k(dsm_tracker *t, float fx, float fy, float cx, float cy) {
  if (!t) return invalid("null tracker");
  desc_make_k(t->desc, t->nlevels, fx, fy, cx, cy);
  t->have_k = true;
  t->desc_dirty = true;
  return DSM_OK;
}

int dsm_tracker_set_ref(dsm_tracker *t, int ref_frame_id, double ref_aff_a, double ref_aff_b,
                        float ref_exposure, const int *n, const float *const *pc_u,
                        const float *const *pc_v, const float *const *pc_idepth,
                        const float *const *pc_color) {
  if (!t || !n || !pc_u || !pc_v || !pc_idepth || !pc_color) return invalid("dsm_tracker_set_ref: null argument");
  dsm_context *ctx = t->ctx;
  DSM_HIP(hipSetDevice(ctx->device));
  for (int l = 0; l < t->nlevels; l++)
    if (n[l] < 0 || n[l] > t->pts_cap[l]) return invalid("dsm_tracker_set_ref: n[lvl] out of range");
  CallArena A; // `work` alone: the four staged lists of a level
  A.work.take(sizeof(float) * 4 * (size_t)t->w * t->h);
  int rc = A.bind(ctx);
  if (rc) return rc;
  if ((rc = t->announce_template_write(ctx->stream, dsm_tracker::kFactArm))) return rc; // interleave_kernel sees every entry it writes
  for (int l = 0; l < t->nlevels; l++) {
    const size_t nl = n[l];
    float *su = A.dev_work<float>(), *sv = su + nl, *si = sv + nl, *sc = si + nl;
    if (nl) {
      DSM_HIP(hipMemcpyAsync(su, pc_u[l], nl * 4, hipMemcpyHostToDevice, ctx->stream));
      DSM_HIP(hipMemcpyAsync(sv, pc_v[l], nl * 4, hipMemcpyHostToDevice, ctx->stream));
      DSM_HIP(hipMemcpyAsync(si, pc_idepth[l], nl * 4, hipMemcpyHostToDevice, ctx->stream));
      DSM_HIP(hipMemcpyAsync(sc, pc_color[l], nl * 4, hipMemcpyHostToDevice, ctx->stream));
      launch_interleave_template(ctx->stream, (int)nl, su, sv, si, sc, t->d_pts[l], t->template_fact_words() ? t->template_fact_words() + l : nullptr);
    }
    DSM_HIP(hipStreamSynchronize(ctx->stream)); // staging buffer is reused by the next level
    t->desc.lv[l].n = (int)nl;
  }
  t->desc.ref_a = ref_aff_a; // :323-324
  t->desc.ref_b = ref_aff_b;
  t->desc.ref_exposure = ref_exposure;
  t->ref_frame_id = ref_frame_id;
  t->have_ref = true;
  t->desc_dirty = true;
  return DSM_OK;
}

int dsm_set_refs_from_points(dsm_context *ctx, int n_jobs, const dsm_ref_job *jobs) {
  if (!ctx || n_jobs < 0 || (n_jobs && !jobs)) return invalid("dsm_set_refs_from_points: bad argument");
  if (!n_jobs) return DSM_OK;
  DSM_HIP(hipSetDevice(ctx->device));
  std::vector<size_t> off((size_t)n_jobs + 1, 0);
  for (int j = 0; j < n_jobs; j++) {
    const dsm_ref_job &J = jobs[j];
    dsm_tracker *t = J.t, *fo = J.frame_owner;
    if (!t || !fo || J.slot < 0 || J.slot > 1 || J.npts < 0 || (J.npts > 0 && (!J.pu || !J.pv || !J.pidepth || !J.pweight)))
      return invalid("dsm_tracker_set_ref_from_points: bad argument");
    if (t->ctx != ctx || fo->ctx != ctx || fo->w != t->w || fo->h != t->h || fo->nlevels != t->nlevels)
      return invalid("dsm_tracker_set_ref_from_points: the frame owner must share context, size and levels");
    if (!fo->have_frame[J.slot]) {
      set_error("dsm_tracker_set_ref_from_points: the keyframe's pyramid has not been uploaded to that slot");
      return DSM_ERR_STATE;
    }
    for (int l = 0; l < t->nlevels; l++)
      if ((long long)((t->w >> l) - 4) * ((t->h >> l) - 4) > t->pts_cap[l]) return invalid("template capacity too small");
    for (int k = 0; k < j; k++)
      if (jobs[k].t == t) return invalid("dsm_set_refs_from_points: a tracker takes one reference per call");
    const size_t floats = make_coarse_depth_workspace_floats(t->w, t->h, t->nlevels, J.npts);
    off[j + 1] = off[j] + ((floats + 63) & ~(size_t)63);
  }
  // ONE launch sequence for all jobs (template_kernels.hip: blockIdx.y = job), ONE host->device copy for their points and the job table
  // (staged in page-locked memory), ONE copy back for their counts.  The arena's regions: in = [points of every job | job table],
  // work = the jobs' workspaces, out = the counts.
  dsm_tracker *t0 = jobs[0].t;
  for (int j = 1; j < n_jobs; j++)
    if (jobs[j].t->w != t0->w || jobs[j].t->h != t0->h || jobs[j].t->nlevels != t0->nlevels)
      return invalid("dsm_set_refs_from_points: trackers of different geometry in one call");
  std::vector<size_t> poff((size_t)n_jobs + 1, 0);
  int max_npts = 0;
  for (int j = 0; j < n_jobs; j++) {
    poff[j + 1] = poff[j] + ((4 * (size_t)jobs[j].npts + 3) & ~(size_t)3);
    if (jobs[j].npts > max_npts) max_npts = jobs[j].npts;
  }
  const size_t cnt_bytes = sizeof(int) * (size_t)n_jobs * (DSM_MAX_LEVELS + 2);
  CallArena A;
  A.in.take(sizeof(float) * poff[n_jobs]);
  const size_t tab_off = A.in.take(sizeof(TplJob) * (size_t)n_jobs);
  A.work.take(sizeof(float) * off[n_jobs]);
  A.out.take(cnt_bytes);
  int rc = A.bind(ctx);
  if (rc) return rc;
  float *d_ws = A.dev_work<float>(), *d_pt = A.dev_in<float>();
  int *d_cnt = A.dev_out<int>();
  TplJob *d_tab = A.dev_in<TplJob>(tab_off);
  float *h_pt = A.host_in<float>();
  TplJob *h_tab = A.host_in<TplJob>(tab_off);
  for (int j = 0; j < n_jobs; j++) {
    const dsm_ref_job &J = jobs[j];
    dsm_tracker *t = J.t;
    t->have_ref = false; // (until its counts are back)
    const size_t np_ = (size_t)J.npts;
    float *hp = h_pt + poff[j];
    if (np_) {
      memcpy(hp, J.pu, sizeof(float) * np_);
      memcpy(hp + np_, J.pv, sizeof(float) * np_);
      memcpy(hp + 2 * np_, J.pidepth, sizeof(float) * np_);
      memcpy(hp + 3 * np_, J.pweight, sizeof(float) * np_);
    }
    TplJob &T = h_tab[j];
    memset(&T, 0, sizeof T);
    T.npts = J.npts;
    T.pt = d_pt + poff[j];
    T.ws = d_ws + off[j];
    T.d_n = d_cnt + (size_t)j * (DSM_MAX_LEVELS + 2);
    for (int l = 0; l < t->nlevels; l++) T.ref[l] = J.frame_owner->d_img[J.slot][l], T.pts[l] = t->d_pts[l];
    if ((rc = t->announce_template_write(ctx->stream, dsm_tracker::kFactArm))) return rc; // tpl_emit_write_kernel sees every entry it writes
    T.facts = t->template_fact_words();
  }
  if ((rc = A.upload())) return rc;
  launch_make_coarse_depth(ctx->stream, t0->w, t0->h, t0->nlevels, d_tab, n_jobs, max_npts, kTexel);
  DSM_HIP(hipGetLastError());
  if ((rc = A.fetch(cnt_bytes))) return rc;
  const int *h_cnt = A.host_out<int>();
  std::vector<int> h_n((size_t)n_jobs * (DSM_MAX_LEVELS + 1), 0);
  for (int j = 0; j < n_jobs; j++)
    for (int l = 0; l <= jobs[j].t->nlevels; l++) h_n[(size_t)j * (DSM_MAX_LEVELS + 1) + l] = h_cnt[(size_t)j * (DSM_MAX_LEVELS + 2) + l];
  for (int j = 0; j < n_jobs; j++)
    if (h_n[(size_t)j * (DSM_MAX_LEVELS + 1) + jobs[j].t->nlevels]) { // a point projected outside the image: the reference would corrupt memory (:160)
      for (int k = 0; k < n_jobs; k++) (void)jobs[k].t->announce_template_write(ctx->stream, dsm_tracker::kFactClear); // (the counts are not taken over)
      return invalid("dsm_tracker_set_ref_from_points: point outside the level-0 image");
    }
  for (int j = 0; j < n_jobs; j++) {
    const dsm_ref_job &J = jobs[j];
    dsm_tracker *t = J.t;
    const int *hn = h_n.data() + (size_t)j * (DSM_MAX_LEVELS + 1);
    for (int l = 0; l < t->nlevels; l++) {
      t->desc.lv[l].n = hn[l];
      if (J.n_out) J.n_out[l] = hn[l];
    }
    t->desc.ref_a = J.ref_aff_a; // :323-324
    t->desc.ref_b = J.ref_aff_b;
    t->desc.ref_exposure = J.ref_exposure;
    t->ref_frame_id = J.ref_frame_id;
    t->have_ref = true;
    t->desc_dirty = true;
  }
  return DSM_OK;
}

int dsm_tracker_set_ref_from_points(dsm_tracker *t, dsm_tracker *frame_owner, int slot, int ref_frame_id, double ref_aff_a,
                                    double ref_aff_b, float ref_exposure, int npts, const float *pu, const float *pv,
                                    const float *pidepth, const float *pweight, int *n_out) {
  if (!t) return invalid("dsm_tracker_set_ref_from_points: bad argument");
  dsm_ref_job J;
  J.t = t, J.frame_owner = frame_owner, J.slot = slot, J.ref_frame_id = ref_frame_id, J.ref_aff_a = ref_aff_a, J.ref_aff_b = ref_aff_b;
  J.ref_exposure = ref_exposure, J.npts = npts, J.pu = pu, J.pv = pv, J.pidepth = pidepth, J.pweight = pweight, J.n_out = n_out;
  return dsm_set_refs_from_points(t->ctx, 1, &J);
}

int dsm_tracker_scale_depth(dsm_tracker *t, float scale) {
  if (!t) return invalid("null tracker");
  if (!t->have_ref) {
    set_error("dsm_tracker_scale_depth before set_ref");
    return DSM_ERR_STATE;
  }
  DSM_HIP(hipSetDevice(t->ctx->device));
  // one launch over all levels, enqueued on the context's stream and NOT waited for: everything that reads the template afterwards --
  // evaluations, the streaming form's advances (their stream groups fork from this stream), dsm_tracker_get_template -- is ordered
  // behind it there (eight keyframes' calls were 0.24 of the 1.9 ms between two advances of 128 concurrent sequences)
  // (the new inverse depths need not keep the template fact: cleared; the next reference establishes it again)
  const int frc = t->announce_template_write(t->ctx->stream, dsm_tracker::kFactClear);
  if (frc) return frc;
  ScaleDepthArgs a;
  a.nlevels = t->nlevels;
  int max_n = 0;
  for (int l = 0; l < t->nlevels; l++) {
    a.n[l] = t->desc.lv[l].n, a.pts[l] = t->d_pts[l];
    if (a.n[l] > max_n) max_n = a.n[l];
  }
  launch_scale_depth_levels(t->ctx->stream, a, max_n, scale);
  DSM_HIP(hipGetLastError());
  return DSM_OK;
}

int dsm_tracker_get_template(dsm_tracker *t, int lvl, int *n, float *pc_u, float *pc_v, float *pc_idepth,
                             float *pc_color) {
  if (!t || !n || lvl < 0 || lvl >= t->nlevels) return invalid("dsm_tracker_get_template: bad argument");
  dsm_context *ctx = t->ctx;
  DSM_HIP(hipSetDevice(ctx->device));
  const size_t nl = t->desc.lv[lvl].n;
  *n = (int)nl;
  if (!pc_u && !pc_v && !pc_idepth && !pc_color) return DSM_OK;
  if (!pc_u || !pc_v || !pc_idepth || !pc_color) return invalid("dsm_tracker_get_template: all four outputs or none");
  if (!nl) return DSM_OK;
  CallArena A; // `work` alone: the four lists on their way out
  A.work.take(sizeof(float) * 4 * nl);
  int rc = A.bind(ctx);
  if (rc) return rc;
  float *su = A.dev_work<float>(), *sv = su + nl, *si = sv + nl, *sc = si + nl;
  launch_deinterleave_template(ctx->stream, (int)nl, t->d_pts[lvl], su, sv, si, sc);
  DSM_HIP(hipMemcpyAsync(pc_u, su, nl * 4, hipMemcpyDeviceToHost, ctx->stream));
  DSM_HIP(hipMemcpyAsync(pc_v, sv, nl * 4, hipMemcpyDeviceToHost, ctx->stream));
  DSM_HIP(hipMemcpyAsync(pc_idepth, si, nl * 4, hipMemcpyDeviceToHost, ctx->stream));
  DSM_HIP(hipMemcpyAsync(pc_color, sc, nl * 4, hipMemcpyDeviceToHost, ctx->stream));
  DSM_HIP(hipStreamSynchronize(ctx->stream));
  return DSM_OK;
}

int dsm_tracker_upload_frame(dsm_tracker *t, int slot, const float *const *dIp, float ab_exposure) {
  if (!t || !dIp || slot < 0 || slot > 1) return invalid("dsm_tracker_upload_frame: bad argument");
  dsm_context *ctx = t->ctx;
  DSM_HIP(hipSetDevice(ctx->device));
  // The device keeps channel 0 only; channels 1 and 2 must be what FrameHessian::makeImages derives
  // from it -- which is all the reference ever passes -- and that is checked (dsm_params.frame_check, frame_grad_tol), not
  // assumed: per level the number of offending texels and the first of them.
  const size_t npx0 = (size_t)t->w * t->h;
  CallArena A; // `work` alone: one level's staged texels, then the check's counters
  A.work.take(sizeof(float) * (3 * npx0 + 4 * DSM_MAX_LEVELS));
  int rc = A.bind(ctx);
  if (rc) return rc;
  float *const d_stage = A.dev_work<float>();
  int *d_bad = (int *)(d_stage + 3 * npx0); // [level]{count, first index}
  int h_bad[2 * DSM_MAX_LEVELS];
  for (int l = 0; l < DSM_MAX_LEVELS; l++) h_bad[2 * l] = 0, h_bad[2 * l + 1] = 0x7FFFFFFF;
  const bool check = t->params.frame_check != 0;
  if (check) DSM_HIP(hipMemcpyAsync(d_bad, h_bad, sizeof h_bad, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = t->announce_plane_write(slot, ctx->stream, dsm_tracker::kFactClear))) return rc; // dip_import_kernel keeps no fact
  for (int l = 0; l < t->nlevels; l++) {
    const int wl = t->w >> l, hl = t->h >> l;
    DSM_HIP(hipMemcpyAsync(d_stage, dIp[l], (size_t)wl * hl * 12, hipMemcpyHostToDevice, ctx->stream));
    launch_dip_import(ctx->stream, wl, hl, d_stage, t->d_img[slot][l], check ? d_bad + 2 * l : nullptr, t->params.frame_grad_tol);
  }
  if (check) DSM_HIP(hipMemcpyAsync(h_bad, d_bad, sizeof h_bad, hipMemcpyDeviceToHost, ctx->stream));
  DSM_HIP(hipStreamSynchronize(ctx->stream));
  for (int l = 0; check && l < t->nlevels; l++)
    if (h_bad[2 * l]) {
      t->have_frame[slot] = false;
      const int wl = t->w >> l, idx = h_bad[2 * l + 1];
      char msg[320];
      snprintf(msg, sizeof msg,
               "dsm_tracker_upload_frame: level %d: %d texel(s) whose gradient channels are not the central differences of channel 0 "
               "(makeImages), the first at index %d (x = %d, y = %d); see dsm_params.frame_check / frame_grad_tol",
               l, h_bad[2 * l], idx, idx % wl, idx / wl);
      return invalid(msg);
    }
  t->desc.exposure[slot] = ab_exposure;
  t->have_frame[slot] = true;
  t->desc_dirty = true;
  return DSM_OK;
}

int dsm_tracker_upload_intensity(dsm_tracker *t, int slot, const float *const *I, float ab_exposure) {
  if (!t || !I || slot < 0 || slot > 1) return invalid("dsm_tracker_upload_intensity: bad argument");
  dsm_context *ctx = t->ctx;
  DSM_HIP(hipSetDevice(ctx->device));
  const int frc = t->announce_plane_write(slot, ctx->stream, dsm_tracker::kFactClear); // raw copies: nobody looks at the pixels
  if (frc) return frc;
  for (int l = 0; l < t->nlevels; l++) {
    if (!I[l]) return invalid("dsm_tracker_upload_intensity: null level");
    DSM_HIP(hipMemcpyAsync(t->d_img[slot][l], I[l], sizeof(float) * (size_t)(t->w >> l) * (t->h >> l), hipMemcpyHostToDevice, ctx->stream));
  }
  DSM_HIP(hipStreamSynchronize(ctx->stream));
  t->desc.exposure[slot] = ab_exposure;
  t->have_frame[slot] = true;
  t->desc_dirty = true;
  return DSM_OK;
}

int dsm_tracker_upload_image(dsm_tracker *t, int slot, const float *image, float ab_exposure) {
  if (!t || !image || slot < 0 || slot > 1) return invalid("dsm_tracker_upload_image: bad argument");
  dsm_context *ctx = t->ctx;
  DSM_HIP(hipSetDevice(ctx->device));
  const size_t npx0 = (size_t)t->w * t->h;
  // the raw image is staged in a buffer of this tracker and slot, so that nothing but the host->device copy has to finish
  // before the call returns (the caller's buffer is free again); the pyramid kernels run on behind it.  With a pinned
  // caller buffer (dsm_host_alloc) the copy is a straight DMA.
  if (!t->d_raw[slot]) DSM_HIP(hipMalloc(&t->d_raw[slot], npx0 * sizeof(float)));
  DSM_HIP(hipMemcpyAsync(t->d_raw[slot], image, npx0 * 4, hipMemcpyHostToDevice, ctx->stream));
  DSM_HIP(hipEventRecord(ctx->handover.copy_event, ctx->stream));
  const int frc = t->announce_plane_write(slot, ctx->stream, dsm_tracker::kFactArm); // pyr_level_fused_kernel sees every pixel it writes
  if (frc) return frc;
  launch_pyramid(ctx->stream, t->w, t->h, t->nlevels, t->d_raw[slot], t->d_img[slot], t->plane_fact_words(slot));
  DSM_HIP(hipGetLastError());
  DSM_HIP(hipEventSynchronize(ctx->handover.copy_event));
  t->desc.exposure[slot] = ab_exposure;
  t->have_frame[slot] = true;
  t->desc_dirty = true;
  return DSM_OK;
}

int dsm_tracker_get_frame(dsm_tracker *t, int slot, int lvl, float *dIp_out) {
  if (!t || !dIp_out || slot < 0 || slot > 1 || lvl < 0 || lvl >= t->nlevels) return invalid("dsm_tracker_get_frame: bad argument");
  dsm_context *ctx = t->ctx;
  DSM_HIP(hipSetDevice(ctx->device));
  const int wl = t->w >> lvl, hl = t->h >> lvl;
  const size_t npx = (size_t)wl * hl;
  CallArena A; // `work` alone: the level's texels on their way out
  A.work.take(sizeof(float) * 3 * npx);
  int rc = A.bind(ctx);
  if (rc) return rc;
  launch_dip_export(ctx->stream, wl, hl, t->d_img[slot][lvl], A.dev_work<float>());
  DSM_HIP(hipMemcpyAsync(dIp_out, A.dev_work<float>(), npx * 12, hipMemcpyDeviceToHost, ctx->stream));
  DSM_HIP(hipStreamSynchronize(ctx->stream));
  return DSM_OK;
}

int dsm_tracker_ref_frame_id(dsm_tracker *t) { return t ? t->ref_frame_id : -1; }

int dsm_reduction_geometry(dsm_tracker *t, int lvl, int n, int *threads, int *pts_per_thread_out, int *chunks) {
  (void)lvl;
  if (!t) return invalid("dsm_reduction_geometry: null tracker");
  if (threads) *threads = kThreads;
  if (pts_per_thread_out) *pts_per_thread_out = pts_per_thread(n, t->desc.p.geometry);
  if (chunks) *chunks = num_chunks(n, t->desc.p.geometry);
  return DSM_OK;
}

} // extern "C"
