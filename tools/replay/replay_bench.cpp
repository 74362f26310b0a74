// replay_bench.cpp -- replay-mode, per-stage benchmark of the hot path as a drop-in user runs it:
// ONE sequence, one frame in flight, driven from the C++ adaptors (direct_stereo_slam_amd/host/TrackerAndScaler.hpp,
// LoopDetection.hpp) the way FrontEnd / LoopHandler drive the reference:
//   per frame      camera bytes in (mono8, main.cpp:216-217) -> pyramid on the device -> the full hypothesis loop of
//                  FrontEnd::trackNewCoarse (FrontEnd.cpp:132-256: constant / double / half / zero motion, zero motion from the
//                  keyframe, 26 rotations x 4 magnitudes) via dsm_host::trackHypotheses;
//   per keyframe   semi-dense template from the window's active points on the device (makeCoarseDepthL0 +
//                  setCoarseTrackingRef, TrackerAndScaler.cpp:143-327), right image in, FrontEnd::optimizeScale
//                  (FrontEnd.cpp:975-1064: the eight initial guesses until "trapped", then one), scaleCoarseDepthL0, tracker swap
//                  (FrontEnd.cpp:627-632);
//   per marginalised keyframe (LoopHandler.cpp:186-262)  generate_spherical_points + ScanContext::generate, search_ringkey,
//                  search_sc;  dslam.txt written at the end (LoopHandler.cpp:59-80).
// The SAME driver then runs on the CPU path -- the oracle's restatement of the reference (oracle/dsm_oracle.c, SSE-intrinsics
// calcGSSSE*, built -O3 -march=native) with the loop descriptors by the product's host functions -- and both print mean ms per
// stage under the reference's own names (main.cpp:181-201: scale_opt, pts_generation, sc_generation, search_ringkey, search_sc,
// per_frame).  Bench infrastructure (bench.py --replay builds and runs it; it links the oracle, so it lives outside the package).
//
//   replay_bench <pack.bin> <out_prefix> [gpu|cpu|both]
// pack.bin (written by bench.py): "DSMRPLY1", int32 w h nl n_frames kf_every n_active, float K[4], double T_stereo[16],
//   double lidar_range; per frame: double gt[7] (x_cam = R x_w + t as {qx qy qz qw tx ty tz}), u8 left[w h]; per keyframe
//   (frame % kf_every == 0) additionally: u8 right[w h], float pu[n] pv[n] pidepth[n] pweight[n].
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../direct_stereo_slam_amd/host/LoopDetection.hpp"
#include "../../direct_stereo_slam_amd/host/TrackerAndScaler.hpp"
#include "../../oracle/dsm_oracle.h"

using dsm_host::AffLight;
using dsm_host::SE3;
using dsm_host::SigType;

// ---- a minimal SE3 (Sophus semantics: unit quaternion x y z w + translation) ----
static void q_mul(const double a[4], const double b[4], double o[4]) {
  o[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
  o[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
  o[1] = a[3] * b[1] - a[0] * b[2] + a[1] * b[3] + a[2] * b[0];
  o[2] = a[3] * b[2] + a[0] * b[1] - a[1] * b[0] + a[2] * b[3];
}
static void q_rot(const double q[4], const double v[3], double o[3]) { // o = R(q) v
  const double x = q[0], y = q[1], z = q[2], w = q[3];
  const double tx = 2 * (y * v[2] - z * v[1]), ty = 2 * (z * v[0] - x * v[2]), tz = 2 * (x * v[1] - y * v[0]);
  o[0] = v[0] + w * tx + (y * tz - z * ty);
  o[1] = v[1] + w * ty + (z * tx - x * tz);
  o[2] = v[2] + w * tz + (x * ty - y * tx);
}
static SE3 se3_mul(const SE3 &a, const SE3 &b) { // a * b
  SE3 o;
  q_mul(a.q, b.q, o.q);
  const double n = std::sqrt(o.q[0] * o.q[0] + o.q[1] * o.q[1] + o.q[2] * o.q[2] + o.q[3] * o.q[3]);
  for (double &c : o.q) c /= n;
  double r[3];
  q_rot(a.q, b.t, r);
  for (int i = 0; i < 3; i++) o.t[i] = r[i] + a.t[i];
  return o;
}
static SE3 se3_inv(const SE3 &a) {
  SE3 o;
  o.q[0] = -a.q[0], o.q[1] = -a.q[1], o.q[2] = -a.q[2], o.q[3] = a.q[3];
  double r[3];
  q_rot(o.q, a.t, r);
  for (int i = 0; i < 3; i++) o.t[i] = -r[i];
  return o;
}
static void so3_log(const double q[4], double w[3]) {
  const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
  double f;
  if (n < 1e-10)
    f = 2.0 / q[3] - 2.0 / 3.0 * n * n / (q[3] * q[3] * q[3]);
  else if (std::fabs(q[3]) < 1e-10)
    f = (q[3] > 0 ? M_PI : -M_PI) / n;
  else
    f = 2.0 * std::atan(n / q[3]) / n;
  for (int i = 0; i < 3; i++) w[i] = f * q[i];
}
static void hat_mul(const double w[3], const double v[3], double o[3]) { o[0] = w[1] * v[2] - w[2] * v[1], o[1] = w[2] * v[0] - w[0] * v[2], o[2] = w[0] * v[1] - w[1] * v[0]; }
// Sophus SE3::log: (upsilon, omega)
static void se3_log(const SE3 &T, double xi[6]) {
  double w[3];
  so3_log(T.q, w);
  const double th = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  double wt[3], wwt[3];
  hat_mul(w, T.t, wt);
  hat_mul(w, wt, wwt);
  double c;
  if (th < 1e-10)
    c = 1.0 / 12.0;
  else
    c = (1.0 - th * std::cos(0.5 * th) / (2.0 * std::sin(0.5 * th))) / (th * th);
  for (int i = 0; i < 3; i++) xi[i] = T.t[i] - 0.5 * wt[i] + c * wwt[i], xi[3 + i] = w[i];
}
static SE3 se3_exp(const double xi[6]) {
  const double *u = xi, *w = xi + 3;
  const double th = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  SE3 o;
  double a, b, c; // q.xyz = a w ; V = I + b W + c W^2
  if (th < 1e-10) {
    a = 0.5 - th * th / 48.0, b = 0.5, c = 1.0 / 6.0;
    o.q[3] = 1.0 - th * th / 8.0;
  } else {
    a = std::sin(0.5 * th) / th, b = (1 - std::cos(th)) / (th * th), c = (th - std::sin(th)) / (th * th * th);
    o.q[3] = std::cos(0.5 * th);
  }
  for (int i = 0; i < 3; i++) o.q[i] = a * w[i];
  double wu[3], wwu[3];
  hat_mul(w, u, wu);
  hat_mul(w, wu, wwu);
  for (int i = 0; i < 3; i++) o.t[i] = u[i] + b * wu[i] + c * wwu[i];
  return o;
}
static SE3 from7(const double *p) {
  SE3 o;
  for (int i = 0; i < 4; i++) o.q[i] = p[i];
  for (int i = 0; i < 3; i++) o.t[i] = p[4 + i];
  return o;
}

// ---- the pack ----
struct KeyframeData {
  std::vector<unsigned char> right;
  std::vector<float> pu, pv, pid, pw;
};
struct Pack {
  int w = 0, h = 0, nl = 0, n_frames = 0, kf_every = 5, n_active = 0;
  float K[4];
  double T[16], lidar_range = 40;
  std::vector<SE3> gt;
  std::vector<std::vector<unsigned char>> left;
  std::map<int, KeyframeData> kf;
};
template <typename T>
static void rd(FILE *f, T *p, size_t n) {
  if (n && fread(p, sizeof(T), n, f) != n) {
    fprintf(stderr, "replay_bench: short read\n");
    exit(2);
  }
}
static Pack load_pack(const char *path) {
  FILE *f = fopen(path, "rb");
  if (!f) {
    fprintf(stderr, "replay_bench: cannot open %s\n", path);
    exit(2);
  }
  char magic[8];
  rd(f, magic, 8);
  if (memcmp(magic, "DSMRPLY1", 8) != 0) {
    fprintf(stderr, "replay_bench: not a replay pack\n");
    exit(2);
  }
  Pack P;
  int hdr[6];
  rd(f, hdr, 6);
  P.w = hdr[0], P.h = hdr[1], P.nl = hdr[2], P.n_frames = hdr[3], P.kf_every = hdr[4], P.n_active = hdr[5];
  rd(f, P.K, 4);
  rd(f, P.T, 16);
  rd(f, &P.lidar_range, 1);
  const size_t px = (size_t)P.w * P.h;
  for (int i = 0; i < P.n_frames; i++) {
    double g[7];
    rd(f, g, 7);
    P.gt.push_back(from7(g));
    P.left.emplace_back(px);
    rd(f, P.left.back().data(), px);
    if (i % P.kf_every == 0) {
      KeyframeData &k = P.kf[i];
      k.right.resize(px);
      rd(f, k.right.data(), px);
      for (std::vector<float> *v : {&k.pu, &k.pv, &k.pid, &k.pw}) {
        v->resize(P.n_active);
        rd(f, v->data(), P.n_active);
      }
    }
  }
  fclose(f);
  return P;
}

// ---- timers under the reference's stage names ----
struct Timers {
  std::map<std::string, std::pair<double, int>> t;
  void add(const std::string &k, double ms) {
    t[k].first += ms;
    t[k].second++;
  }
};
typedef std::chrono::steady_clock Clock;
static double ms_since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }

struct TrackOut {
  bool haveOneGood = false;
  SE3 lastF_2_fh;
  AffLight aff;
  double achievedRes[5];
  int tries = 0;
};

// ---- backend 1: the product through the C++ adaptors ----
// dsm_params.chunk_geometry of every tracker of the replay: 2 (one frame of a sequence is in flight at a time: the latency table above 4096
// points, one chunk below) unless DSM_REPLAY_GEOMETRY says otherwise; the one-sequence run and the concurrent run share it, so their
// results stay comparable bit for bit.  dsm_params.persistent_coarse: -1 (the one-chunk levels' LM loop as a chain, one launch) unless
// DSM_REPLAY_COARSE says otherwise.
static int g_geometry_override = -1; // (the concurrent leg's table while that leg and its one-sequence reference run)
static int replay_geometry() {
  if (g_geometry_override >= 0) return g_geometry_override;
  const char *e = getenv("DSM_REPLAY_GEOMETRY");
  return e ? atoi(e) : 2;
}
// the concurrent leg (many sequences through one stream: bound by the host's calls, its levels evaluated beside other sequences') keeps the
// latency table, measured 4-5 % faster there than the tables with one-chunk small levels; DSM_REPLAY_CONC_GEOMETRY says otherwise
static int replay_concurrent_geometry() {
  const char *e = getenv("DSM_REPLAY_CONC_GEOMETRY");
  return e ? atoi(e) : 1;
}
static int replay_coarse() {
  const char *e = getenv("DSM_REPLAY_COARSE");
  return e ? atoi(e) : -1;
}

struct GpuBackend {
  const Pack &P;
  dsm_context *ctx = nullptr;
  std::unique_ptr<dsm_host::TrackerAndScaler> a, b;
  dsm_host::TrackerAndScaler *cur, *nxt; // coarse_tracker_ / coarse_tracker_for_new_kf_ (FrontEnd.h:187-190)
  std::deque<dsm_host::FrameView> views;
  dsm_host::FrameView fv;
  std::unique_ptr<dsm_host::RingKeyIndex> ring;
  dsm_host::ScanContext sc;
  explicit GpuBackend(const Pack &p) : P(p) {
    dsm_host::check(dsm_context_create(0, &ctx), "dsm_context_create");
    dsm_params prm;
    dsm_host::check(DSM_PARAMS_INIT(&prm), "DSM_PARAMS_INIT");
    prm.chunk_geometry = replay_geometry();
    prm.persistent_coarse = replay_coarse();
    std::vector<double> tv(P.T, P.T + 16);
    a.reset(new dsm_host::TrackerAndScaler(ctx, P.w, P.h, P.nl, tv, P.K, &prm));
    b.reset(new dsm_host::TrackerAndScaler(ctx, P.w, P.h, P.nl, tv, P.K, &prm));
    a->makeK(P.K[0], P.K[1], P.K[2], P.K[3]);
    b->makeK(P.K[0], P.K[1], P.K[2], P.K[3]);
    cur = a.get(), nxt = b.get();
    ring.reset(new dsm_host::RingKeyIndex(ctx, (int)sc.getHeight()));
  }
  ~GpuBackend() {
    ring.reset();
    a.reset();
    b.reset();
    dsm_context_destroy(ctx);
  }
  const char *name() const { return "gpu"; }
  void new_left(int i) {
    cur->uploadImage(DSM_SLOT_NEW_LEFT, P.left[i].data(), DSM_PIXEL_U8, 1.0f, i);
    fv = dsm_host::FrameView();
    fv.shell_id = i, fv.unique_id = i;
  }
  TrackOut track(const std::vector<SE3> &tries, const AffLight &aff, double last_rmse0) {
    dsm_host::HypothesesResult R = dsm_host::trackHypotheses(ctx, *cur, fv, tries, aff, P.nl - 1, last_rmse0);
    TrackOut o;
    o.haveOneGood = R.haveOneGood, o.lastF_2_fh = R.lastF_2_fh, o.aff = R.aff_g2l, o.tries = R.triesUsed;
    memcpy(o.achievedRes, R.achievedRes, sizeof o.achievedRes);
    return o;
  }
  void make_keyframe(int i, const AffLight &aff, const KeyframeData &k) { // the new keyframe's pyramid sits in cur's NEW_LEFT slot
    views.emplace_back();
    dsm_host::FrameView &ref = views.back();
    ref.shell_id = i, ref.unique_id = i, ref.aff_g2l = aff;
    nxt->setCoarseTrackingRef(ref, *cur, (int)k.pu.size(), k.pu.data(), k.pv.data(), k.pid.data(), k.pw.data());
  }
  float scale_opt(int i, const KeyframeData &k, bool trapped, float &new_scale) {
    nxt->uploadImage(DSM_SLOT_NEW_RIGHT, k.right.data(), DSM_PIXEL_U8, 1.0f, 1000000 + i);
    dsm_host::FrameView fh1;
    fh1.shell_id = i, fh1.unique_id = 1000000 + i;
    if (trapped) {
      new_scale = 1.0f;
      return nxt->optimizeScale(fh1, new_scale, P.nl - 1); // FrontEnd.cpp:991-993
    }
    return nxt->optimizeScaleGuesses(fh1, {0.1f, 1, 5, 10, 15, 25, 30, 50}, new_scale, P.nl - 1); // :995-1003
  }
  void scale_depth(float s) { nxt->scaleCoarseDepthL0(s); }
  void swap_trackers() { std::swap(cur, nxt); }
  // generate_spherical_points + ScanContext::generate on the device (dsm_loop_descriptors_batch, one job)
  void descriptors(std::vector<int> &kf_ids, std::vector<double> &kf_pose_wc, const double cur_cw[12], std::vector<int> &pt_kf,
                   std::vector<double> &pt_xyz, std::vector<float> &ringkey, SigType &sig, Timers &tm) {
    const int n_kf = (int)kf_ids.size(), n_pts = (int)pt_kf.size();
    std::vector<int> keep(n_kf), sel(n_pts), sidx(60 * 20);
    std::vector<double> sph(3 * (size_t)n_pts), sval(60 * 20);
    int n_out = 0, n_sig = 0;
    double tfm[16];
    ringkey.assign(20, 0.f);
    dsm_loop_job job;
    memset(&job, 0, sizeof job);
    job.n_kf = n_kf, job.kf_ids = kf_ids.data(), job.kf_pose_wc = kf_pose_wc.data(), job.cur_cw = cur_cw;
    job.n_pts = n_pts, job.pt_kf_id = pt_kf.data(), job.pt_xyz = pt_xyz.data();
    job.kf_keep = keep.data(), job.n_out = &n_out, job.sel_idx = sel.data(), job.pts_spherical = sph.data();
    job.ringkey = ringkey.data(), job.sig_idx = sidx.data(), job.sig_val = sval.data(), job.n_sig = &n_sig, job.tfm_pca_rig = tfm;
    const auto t0 = Clock::now();
    dsm_host::loop_check(dsm_loop_descriptors_batch(ctx, 1, &job, P.lidar_range, 60, 20), "dsm_loop_descriptors_batch");
    tm.add("pts_generation+sc_generation", ms_since(t0));
    sig.clear();
    for (int i = 0; i < n_sig; i++) sig.push_back({sidx[i], sval[i]});
  }
  void search_ringkey(const std::vector<float> &key, std::vector<int> &cand) { ring->search_ringkey(key.data(), cand); }
  void search_sc(const SigType &sig, const std::vector<SigType> &all, const std::vector<int> &cand, int &idx, float &diff) {
    dsm_host::search_sc(sig, [&](int i) -> const SigType & { return all[i]; }, cand, 60, idx, diff);
  }
  // the keyframe's whole chain -- generate_spherical_points, ScanContext::generate, search_ringkey -- as ONE enqueue and ONE read-back
  // (dsm_loop_detect_batch, one job; the selected points stay on the device: nothing downstream of the hot path reads them here)
  static constexpr bool kFusedLoopChain = true;
  void descriptors_and_search(std::vector<int> &kf_ids, std::vector<double> &kf_pose_wc, const double cur_cw[12], std::vector<int> &pt_kf,
                              std::vector<double> &pt_xyz, std::vector<float> &ringkey, SigType &sig, std::vector<int> &cand, Timers &tm) {
    const int n_kf = (int)kf_ids.size(), n_pts = (int)pt_kf.size();
    std::vector<int> keep(n_kf), sidx(60 * 20);
    std::vector<double> sval(60 * 20);
    int n_out = 0, n_sig = 0, ncand = 0, cands[4] = {0, 0, 0, 0};
    double tfm[16];
    ringkey.assign(20, 0.f);
    dsm_loop_job job;
    memset(&job, 0, sizeof job);
    job.n_kf = n_kf, job.kf_ids = kf_ids.data(), job.kf_pose_wc = kf_pose_wc.data(), job.cur_cw = cur_cw;
    job.n_pts = n_pts, job.pt_kf_id = pt_kf.data(), job.pt_xyz = pt_xyz.data();
    job.kf_keep = keep.data(), job.n_out = &n_out;
    job.ringkey = ringkey.data(), job.sig_idx = sidx.data(), job.sig_val = sval.data(), job.n_sig = &n_sig, job.tfm_pca_rig = tfm;
    const auto t0 = Clock::now();
    dsm_host::loop_check(dsm_loop_detect_batch(ctx, ring->handle(), 1, &job, P.lidar_range, 60, 20, cands, &ncand), "dsm_loop_detect_batch");
    tm.add("pts_generation+sc_generation+search_ringkey (one call)", ms_since(t0));
    sig.clear();
    for (int i = 0; i < n_sig; i++) sig.push_back({sidx[i], sval[i]});
    cand.assign(cands, cands + ncand);
  }
};

// ---- backend 2: the CPU path (oracle restatement of the reference; host functions of the product for the loop descriptors) ----
struct CpuBackend {
  static constexpr bool kFusedLoopChain = false;
  const Pack &P;
  orc_tracker *a, *b, *cur, *nxt;
  orc_ringdb *ring;
  std::vector<std::vector<float>> pyr_left, pyr_right, pyr_kf; // borrowed by the trackers: kept alive here
  std::vector<std::vector<float>> tu, tv, tid, tc;
  explicit CpuBackend(const Pack &p) : P(p) {
    orc_params prm;
    orc_params_default(&prm);
    a = orc_tracker_create(P.w, P.h, P.nl, P.T, P.K, &prm);
    b = orc_tracker_create(P.w, P.h, P.nl, P.T, P.K, &prm);
    for (orc_tracker *t : {a, b}) {
      orc_tracker_make_k(t, P.K[0], P.K[1], P.K[2], P.K[3]);
      orc_tracker_use_sse(t, 1);
    }
    cur = a, nxt = b;
    std::vector<float> dummy(20, 0.f);
    ring = orc_ringdb_create(20, dsm_host::kLoopMargin, dsm_host::kFlannNN, dsm_host::kRingkeyThres, dummy.data());
    for (auto *v : {&pyr_left, &pyr_right, &pyr_kf}) {
      v->resize(P.nl);
      for (int l = 0; l < P.nl; l++) (*v)[l].resize(3 * (size_t)(P.w >> l) * (P.h >> l));
    }
    for (auto *v : {&tu, &tv, &tid, &tc}) {
      v->resize(P.nl);
      for (int l = 0; l < P.nl; l++) (*v)[l].resize((size_t)(P.w >> l) * (P.h >> l));
    }
  }
  ~CpuBackend() {
    orc_tracker_destroy(a);
    orc_tracker_destroy(b);
    orc_ringdb_destroy(ring);
  }
  const char *name() const { return "cpu"; }
  void make_images(const std::vector<unsigned char> &img, std::vector<std::vector<float>> &pyr) {
    std::vector<float> f(img.begin(), img.end());
    std::vector<float *> out(P.nl);
    for (int l = 0; l < P.nl; l++) out[l] = pyr[l].data();
    orc_make_images(f.data(), P.w, P.h, P.nl, out.data());
  }
  static std::vector<const float *> ptrs(const std::vector<std::vector<float>> &v) {
    std::vector<const float *> p;
    for (auto &x : v) p.push_back(x.data());
    return p;
  }
  void new_left(int i) {
    make_images(P.left[i], pyr_left); // FrameHessian::makeImages (FrontEnd.cpp:605)
    orc_tracker_set_frame(cur, 0, ptrs(pyr_left).data(), 1.0f);
  }
  // FrontEnd.cpp:194-256 as written: one trackNewestCoarse after the other
  TrackOut track(const std::vector<SE3> &tries, const AffLight &aff_last, double last_rmse0) {
    TrackOut o;
    double achieved[DSM_MAX_LEVELS];
    for (double &v : achieved) v = NAN;
    for (size_t i = 0; i < tries.size(); i++) {
      double pose[7] = {tries[i].q[0], tries[i].q[1], tries[i].q[2], tries[i].q[3], tries[i].t[0], tries[i].t[1], tries[i].t[2]};
      double aff[2] = {aff_last.a, aff_last.b}, cur_res[DSM_MAX_LEVELS], flow[3];
      const bool good = orc_track(cur, pose, aff, P.nl - 1, achieved, cur_res, flow) != 0;
      o.tries++;
      if (good && std::isfinite((float)cur_res[0]) && !(cur_res[0] >= achieved[0])) {
        o.aff = AffLight(aff[0], aff[1]);
        o.lastF_2_fh = from7(pose);
        o.haveOneGood = true;
      }
      if (o.haveOneGood)
        for (int l = 0; l < 5; l++)
          if (!std::isfinite((float)achieved[l]) || achieved[l] > cur_res[l]) achieved[l] = cur_res[l];
      if (o.haveOneGood && achieved[0] < last_rmse0 * 1.5) break;
    }
    if (!o.haveOneGood) o.lastF_2_fh = tries[0], o.aff = aff_last;
    memcpy(o.achievedRes, achieved, sizeof o.achievedRes);
    return o;
  }
  void make_keyframe(int i, const AffLight &aff, const KeyframeData &k) {
    pyr_kf = pyr_left; // the keyframe's pyramid stays alive as the reference of the next frames
    std::vector<float *> pu, pv, pid, pc;
    for (int l = 0; l < P.nl; l++) pu.push_back(tu[l].data()), pv.push_back(tv[l].data()), pid.push_back(tid[l].data()), pc.push_back(tc[l].data());
    int n[DSM_MAX_LEVELS] = {0};
    orc_make_coarse_depth_l0(nxt, (int)k.pu.size(), k.pu.data(), k.pv.data(), k.pid.data(), k.pw.data(), ptrs(pyr_kf).data(), n, pu.data(), pv.data(),
                             pid.data(), pc.data());
    orc_tracker_set_ref(nxt, i, aff.a, aff.b, 1.0f, n, ptrs(tu).data(), ptrs(tv).data(), ptrs(tid).data(), ptrs(tc).data());
  }
  float scale_opt(int, const KeyframeData &k, bool trapped, float &new_scale) {
    make_images(k.right, pyr_right);
    orc_tracker_set_frame(nxt, 1, ptrs(pyr_right).data(), 1.0f);
    if (trapped) {
      new_scale = 1.0f;
      return orc_optimize_scale(nxt, &new_scale, P.nl - 1);
    }
    float err = -1;
    new_scale = 1.0f;
    for (float g : {0.1f, 1.f, 5.f, 10.f, 15.f, 25.f, 30.f, 50.f}) {
      float s = g;
      const float e = orc_optimize_scale(nxt, &s, P.nl - 1);
      if (e > 0 && (err < 0 || err > e)) err = e, new_scale = s;
    }
    return err;
  }
  void scale_depth(float s) { orc_tracker_scale_depth(nxt, s); }
  void swap_trackers() { std::swap(cur, nxt); }
  void descriptors(std::vector<int> &kf_ids, std::vector<double> &kf_pose_wc, const double cur_cw[12], std::vector<int> &pt_kf,
                   std::vector<double> &pt_xyz, std::vector<float> &ringkey, SigType &sig, Timers &tm) {
    const int n_kf = (int)kf_ids.size(), n_pts = (int)pt_kf.size();
    std::vector<int> keep(n_kf), sel(n_pts), sidx(60 * 20);
    std::vector<double> sph(3 * (size_t)n_pts), sval(60 * 20);
    int n_out = 0, n_sig = 0;
    double tfm[16];
    ringkey.assign(20, 0.f);
    auto t0 = Clock::now();
    dsm_host::loop_check(dsm_generate_spherical_points(n_kf, kf_ids.data(), kf_pose_wc.data(), cur_cw, P.lidar_range, n_pts, pt_kf.data(), pt_xyz.data(),
                                                       keep.data(), &n_out, sel.data(), sph.data()),
                         "generate_spherical_points");
    const double t_pts = ms_since(t0);
    t0 = Clock::now();
    dsm_host::loop_check(dsm_scancontext_generate(sph.data(), n_out, P.lidar_range, 60, 20, ringkey.data(), sidx.data(), sval.data(), &n_sig, tfm),
                         "ScanContext::generate");
    const double t_sc = ms_since(t0);
    tm.add("pts_generation", t_pts);
    tm.add("sc_generation", t_sc);
    tm.add("pts_generation+sc_generation", t_pts + t_sc);
    sig.clear();
    for (int i = 0; i < n_sig; i++) sig.push_back({sidx[i], sval[i]});
  }
  void search_ringkey(const std::vector<float> &key, std::vector<int> &cand) {
    int c[8], n = 0;
    orc_ringdb_query_then_enqueue(ring, key.data(), c, &n);
    for (int i = 0; i < n; i++) cand.push_back(c[i]);
  }
  void search_sc(const SigType &sig, const std::vector<SigType> &all, const std::vector<int> &cand, int &idx, float &diff) {
    std::vector<int> ai;
    std::vector<double> av;
    for (auto &p : sig) ai.push_back(p.first), av.push_back(p.second);
    std::vector<std::vector<int>> bi(cand.size());
    std::vector<std::vector<double>> bv(cand.size());
    std::vector<const int *> bip;
    std::vector<const double *> bvp;
    std::vector<int> bn;
    for (size_t c = 0; c < cand.size(); c++) {
      for (auto &p : all[cand[c]]) bi[c].push_back(p.first), bv[c].push_back(p.second);
      bip.push_back(bi[c].data()), bvp.push_back(bv[c].data()), bn.push_back((int)bi[c].size());
    }
    orc_search_sc(ai.data(), av.data(), (int)ai.size(), (int)cand.size(), cand.data(), bip.data(), bvp.data(), bn.data(), 60, &idx, &diff);
  }
};

// ---- the driver: FrontEnd + LoopHandler reduced to the calls that reach the hot path ----
struct LoopQuery { // what one marginalised keyframe hands to the loop detector (LoopHandler.cpp:186-262), and the ring key it got
  std::vector<int> ids, pk;
  std::vector<double> poses, xyz;
  double cw[12];
  std::vector<float> key;
};
struct RunResult {
  Timers tm;
  std::vector<SE3> est; // x_cam = T x_w per frame
  std::vector<LoopQuery> queries;
  std::vector<std::vector<int>> candidates;
  std::vector<int> matched;
  std::vector<float> scales;
  int tries_total = 0, frames_with_retries = 0, lost = 0;
};

static std::vector<SE3> hypothesis_list(const std::vector<SE3> &est, const SE3 &T_kf) { // FrontEnd.cpp:132-192
  std::vector<SE3> tries;
  const size_t n = est.size(); // frames before the new one
  if (n < 2) {
    tries.push_back(SE3());
    return tries;
  }
  const SE3 &T_slast = est[n - 1], &T_sprelast = est[n - 2];
  // camToWorld = T^-1:  slast_2_sprelast = sprelast.camToWorld^-1 slast.camToWorld ; lastF_2_slast = slast.camToWorld^-1 lastF.camToWorld
  const SE3 slast_2_sprelast = se3_mul(T_sprelast, se3_inv(T_slast));
  const SE3 lastF_2_slast = se3_mul(T_slast, se3_inv(T_kf));
  const SE3 fh_2_slast = slast_2_sprelast;
  const SE3 inv = se3_inv(fh_2_slast);
  const SE3 constant = se3_mul(inv, lastF_2_slast);
  tries.push_back(constant);                              // constant motion
  tries.push_back(se3_mul(inv, se3_mul(inv, lastF_2_slast))); // double motion
  double xi[6];
  se3_log(fh_2_slast, xi);
  for (double &v : xi) v *= 0.5;
  tries.push_back(se3_mul(se3_inv(se3_exp(xi)), lastF_2_slast)); // half motion
  tries.push_back(lastF_2_slast);                         // zero motion
  tries.push_back(SE3());                                 // zero motion from the keyframe
  static const float rs[26][3] = {{1, 0, 0},   {0, 1, 0},   {0, 0, 1},   {-1, 0, 0},   {0, -1, 0},  {0, 0, -1},  {1, 1, 0},   {0, 1, 1},  {1, 0, 1},
                                  {-1, 1, 0},  {0, -1, 1},  {-1, 0, 1},  {1, -1, 0},   {0, 1, -1},  {1, 0, -1},  {-1, -1, 0}, {0, -1, -1}, {-1, 0, -1},
                                  {-1, -1, -1}, {-1, -1, 1}, {-1, 1, -1}, {-1, 1, 1},  {1, -1, -1}, {1, -1, 1},  {1, 1, -1},  {1, 1, 1}};
  for (float rot_delta = 0.02; rot_delta < 0.05; rot_delta += 0.01)
    for (int k = 0; k < 26; k++) {
      SE3 d;
      d.q[3] = 1, d.q[0] = rs[k][0] * rot_delta, d.q[1] = rs[k][1] * rot_delta, d.q[2] = rs[k][2] * rot_delta;
      const double nn = std::sqrt(d.q[0] * d.q[0] + d.q[1] * d.q[1] + d.q[2] * d.q[2] + d.q[3] * d.q[3]);
      for (double &c : d.q) c /= nn;
      tries.push_back(se3_mul(constant, d));
    }
  return tries;
}

struct WindowKf {
  int id;
  SE3 T; // estimated pose
  std::vector<double> world_pts;
};

// Lap one: the sequence is treated as the SECOND pass over the same places; the first pass's descriptors (the same clouds
// under 2 cm of noise) are searched and enqueued before the clock starts, followed by LOOP_MARGIN filler keys that flush
// the delay queue (search_place.h:41-56), so that the timed pass finds candidates and runs search_sc.
template <class B>
static void seed_first_pass(B &be, const Pack &P, std::vector<SigType> &signatures) {
  {
    unsigned lcg = 12345u;
    auto noise = [&]() {
      lcg = lcg * 1664525u + 1013904223u;
      return ((double)(lcg >> 8) / (double)(1u << 24) - 0.5) * 0.07; // uniform, sigma ~ 2 cm
    };
    std::deque<WindowKf> win;
    Timers scratch;
    for (int i = 0; i < P.n_frames; i += P.kf_every) {
      const KeyframeData &k = P.kf.at(i);
      WindowKf wk;
      wk.id = i, wk.T = P.gt[i];
      const SE3 Tinv = se3_inv(P.gt[i]);
      for (size_t j = 0; j < k.pu.size(); j++) {
        const double z = 1.0 / k.pid[j];
        const double pc[3] = {(k.pu[j] - P.K[2]) / P.K[0] * z, (k.pv[j] - P.K[3]) / P.K[1] * z, z};
        double pw[3];
        q_rot(Tinv.q, pc, pw);
        for (int c = 0; c < 3; c++) wk.world_pts.push_back(pw[c] + Tinv.t[c] + noise());
      }
      win.push_back(std::move(wk));
      if (win.size() > 7) {
        std::vector<int> ids, pk;
        std::vector<double> poses, xyz;
        for (const WindowKf &q : win) {
          ids.push_back(q.id);
          double xi[6];
          se3_log(se3_inv(q.T), xi);
          poses.insert(poses.end(), xi, xi + 6);
          for (size_t j = 0; j < q.world_pts.size() / 3; j++) pk.push_back(q.id);
          xyz.insert(xyz.end(), q.world_pts.begin(), q.world_pts.end());
        }
        const SE3 &Tm = win.front().T;
        double cw[12]; // row-major 3x4 [R | t] of the marginalised keyframe
        {
          const double *q = Tm.q;
          const double x = q[0], y = q[1], z = q[2], w = q[3];
          const double Rm[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                                2 * (y * z - x * w),     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)};
          for (int r = 0; r < 3; r++) cw[4 * r] = Rm[3 * r], cw[4 * r + 1] = Rm[3 * r + 1], cw[4 * r + 2] = Rm[3 * r + 2], cw[4 * r + 3] = Tm.t[r];
        }
        std::vector<float> key;
        SigType sig;
        be.descriptors(ids, poses, cw, pk, xyz, key, sig, scratch);
        std::vector<int> cand;
        be.search_ringkey(key, cand);
        signatures.push_back(sig);
        win.pop_front();
      }
    }
    for (int f = 0; f < dsm_host::kLoopMargin; f++) { // fillers: far from every real key
      std::vector<float> key(20);
      for (int j = 0; j < 20; j++) key[j] = 5.0f + 0.01f * (float)((f * 7 + j * 13) % 97);
      std::vector<int> cand;
      be.search_ringkey(key, cand);
      signatures.push_back(SigType());
    }
  }
}

template <class B>
static RunResult run(B &be, const Pack &P) {
  RunResult R;
  SE3 T_kf;
  AffLight aff_last;
  double last_rmse0 = 100;
  bool trapped = false;
  int scale_fails = 0, n_kf = 0;
  std::deque<WindowKf> window;
  std::vector<SigType> signatures; // loop_frames_[i]->signature in search order
  seed_first_pass(be, P, signatures);
  for (int i = 0; i < P.n_frames; i++) {
    const auto t_frame = Clock::now();
    auto t0 = Clock::now();
    be.new_left(i);
    R.tm.add("image_handover+pyramid", ms_since(t0));
    SE3 est;
    AffLight aff_now = aff_last;
    if (i == 0) {
      est = P.gt[0]; // the initializer is out of scope: the first frame is at its true pose
    } else {
      const std::vector<SE3> tries = hypothesis_list(R.est, T_kf);
      t0 = Clock::now();
      const TrackOut o = be.track(tries, aff_last, last_rmse0);
      R.tm.add("trackNewCoarse", ms_since(t0));
      R.tries_total += o.tries;
      R.frames_with_retries += o.tries > 1;
      R.lost += !o.haveOneGood;
      last_rmse0 = o.achievedRes[0];
      est = se3_mul(o.lastF_2_fh, T_kf);
      aff_now = o.aff;
    }
    R.est.push_back(est);
    aff_last = aff_now;
    if (i % P.kf_every == 0) { // makeKeyFrame (FrontEnd.cpp:789-811)
      const KeyframeData &k = P.kf.at(i);
      t0 = Clock::now();
      be.make_keyframe(i, aff_now, k);
      R.tm.add("setCoarseTrackingRef", ms_since(t0));
      n_kf++;
      if (n_kf > 4) { // :806 all_keyframes_history_.size() > 4
        t0 = Clock::now();
        float new_scale = 1.0f;
        float err = be.scale_opt(i, k, trapped, new_scale);
        R.tm.add("scale_opt", ms_since(t0));
        R.scales.push_back(new_scale);
        bool ok = err < 15.0f; // scale_opt_thres (main.cpp:302)
        if (trapped && std::fabs(new_scale - 1.0f) > 0.5f) ok = false;
        scale_fails = ok ? 0 : scale_fails + 1;
        if (scale_fails > 5) trapped = false;
        if (ok) {
          be.scale_depth(new_scale);
          trapped = true;
        }
      }
      be.swap_trackers(); // FrontEnd.cpp:627-632
      T_kf = est;
      last_rmse0 = 100; // a new reference: firstCoarseRMSE / last_coarse_rmse_ start over
      // LoopHandler: the window's oldest keyframe is marginalised once eight are alive (LoopHandler.cpp:186-262)
      WindowKf wk;
      wk.id = i, wk.T = est;
      const SE3 Tinv = se3_inv(est);
      for (size_t j = 0; j < k.pu.size(); j++) {
        const double z = 1.0 / k.pid[j];
        const double pc[3] = {(k.pu[j] - P.K[2]) / P.K[0] * z, (k.pv[j] - P.K[3]) / P.K[1] * z, z};
        double pw[3];
        q_rot(Tinv.q, pc, pw);
        for (int c = 0; c < 3; c++) wk.world_pts.push_back(pw[c] + Tinv.t[c]);
      }
      window.push_back(std::move(wk));
      if (window.size() > 7) {
        std::vector<int> ids, pk;
        std::vector<double> poses, xyz;
        for (const WindowKf &q : window) {
          ids.push_back(q.id);
          double xi[6];
          se3_log(se3_inv(q.T), xi);
          poses.insert(poses.end(), xi, xi + 6);
          for (size_t j = 0; j < q.world_pts.size() / 3; j++) pk.push_back(q.id);
          xyz.insert(xyz.end(), q.world_pts.begin(), q.world_pts.end());
        }
        const SE3 &Tm = window.front().T;
        double cw[12];
        {
          const double *q = Tm.q;
          const double x = q[0], y = q[1], z = q[2], w = q[3];
          const double Rm[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                                2 * (y * z - x * w),     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)};
          for (int r = 0; r < 3; r++) cw[4 * r] = Rm[3 * r], cw[4 * r + 1] = Rm[3 * r + 1], cw[4 * r + 2] = Rm[3 * r + 2], cw[4 * r + 3] = Tm.t[r];
        }
        std::vector<float> key;
        SigType sig;
        std::vector<int> cand;
        if constexpr (B::kFusedLoopChain) {
          be.descriptors_and_search(ids, poses, cw, pk, xyz, key, sig, cand, R.tm);
        } else {
          be.descriptors(ids, poses, cw, pk, xyz, key, sig, R.tm);
          t0 = Clock::now();
          be.search_ringkey(key, cand);
          R.tm.add("search_ringkey", ms_since(t0));
        }
        {
          LoopQuery lq;
          lq.ids = ids, lq.pk = pk, lq.poses = poses, lq.xyz = xyz, lq.key = key;
          memcpy(lq.cw, cw, sizeof lq.cw);
          R.queries.push_back(std::move(lq));
        }
        int matched = -1;
        float diff = -1;
        if (!cand.empty()) {
          t0 = Clock::now();
          be.search_sc(sig, signatures, cand, matched, diff);
          R.tm.add("search_sc", ms_since(t0));
        }
        signatures.push_back(sig);
        R.candidates.push_back(cand);
        R.matched.push_back(matched);
        window.pop_front();
      }
    }
    R.tm.add("per_frame", ms_since(t_frame));
  }
  return R;
}

// ---- concurrent mode: S sequences share the GPU through ONE dsm_host::Stream ("one (or many batched) independent
// sequence(s) per GPU"; BASELINE configs[3], [4]) ----
// Every sequence is the driver above reduced to the tracker's calls -- hand-over, trackNewCoarse, makeKeyFrame, optimizeScale, tracker
// swap (the loop descriptors stay with the one-sequence run) -- and has ONE problem in flight: its frame's first hypothesis (the
// constant-motion guess; a frame it does not settle goes through the whole list synchronously, as trackHypotheses does) or its
// keyframe's scale guesses.  With DSM_REPLAY_HYPOTHESES=stream a frame's whole hypothesis list is ONE group of the stream instead
// (Stream::submitHypotheses): a frame that needs retries no longer holds up the other sequences.  All sequences submit into one stream; an advance moves every resident problem.  Results equal the
// one-sequence run's bit for bit (the stream is scheduling only), which main() checks.
struct ConcurrentResult {
  int sequences = 0, advances = 0, fallbacks = 0, lost = 0;
  long long frames = 0;
  double wall_ms = 0, latency_ms_sum = 0, latency_ms_max = 0;
  std::vector<std::vector<SE3>> est;
  std::vector<std::vector<float>> scales;
  std::map<std::string, double> host_ms; // host wall time inside each kind of call, summed over the run
};

// DSM_REPLAY_HYPOTHESES=stream: the concurrent leg submits every frame's hypothesis list as one stream group
static bool replay_hypotheses_in_stream() {
  const char *e = getenv("DSM_REPLAY_HYPOTHESES");
  return e && strcmp(e, "stream") == 0;
}

static ConcurrentResult run_concurrent(const Pack &P, int S, bool pipelined) {
  struct Seq {
    std::unique_ptr<dsm_host::TrackerAndScaler> a, b;
    dsm_host::TrackerAndScaler *cur = nullptr, *nxt = nullptr;
    std::deque<dsm_host::FrameView> views;
    std::vector<SE3> est;
    std::vector<float> scales;
    SE3 T_kf, est_now;
    AffLight aff_last, aff_now;
    double last_rmse0 = 100;
    bool trapped = false;
    int scale_fails = 0, n_kf = 0, frame = 0, lag = 0, scale_pending = 0;
    enum { IDLE, TRACKING, SCALING, DONE } state = IDLE;
    std::vector<SE3> tries;
    std::vector<uint64_t> scale_tickets;
    std::vector<float> scale_val, scale_err;
    Clock::time_point t_start;
  };
  ConcurrentResult R;
  R.sequences = S;
  auto timed = [&R](const char *what, auto &&fn) {
    const auto t0 = Clock::now();
    fn();
    R.host_ms[what] += ms_since(t0);
  };
  dsm_context *ctx = nullptr;
  dsm_host::check(dsm_context_create(0, &ctx), "dsm_context_create");
  // the camera frames in page-locked memory (dsm_host_alloc), as a node's capture buffers would be: the hand-over of the frames that
  // arrived together is one DMA, not a staged copy of pageable memory (which alone was 2 ms per advance at 128 sequences)
  const size_t px = (size_t)P.w * P.h;
  unsigned char *pinned = nullptr;
  dsm_host::check(dsm_host_alloc(px * ((size_t)P.n_frames + P.kf.size()), (void **)&pinned), "dsm_host_alloc");
  std::vector<const unsigned char *> left_px((size_t)P.n_frames);
  std::map<int, const unsigned char *> right_px;
  {
    unsigned char *w = pinned;
    for (int i = 0; i < P.n_frames; i++, w += px) memcpy(w, P.left[i].data(), px), left_px[i] = w;
    for (const auto &kv : P.kf) memcpy(w, kv.second.right.data(), px), right_px[kv.first] = w, w += px;
  }
  {
    dsm_params prm;
    dsm_host::check(DSM_PARAMS_INIT(&prm), "DSM_PARAMS_INIT");
    prm.chunk_geometry = replay_geometry();
    prm.persistent_coarse = replay_coarse();
    std::vector<double> tv(P.T, P.T + 16);
    std::vector<Seq> seqs((size_t)S);
    for (int s = 0; s < S; s++) {
      Seq &q = seqs[s];
      q.a.reset(new dsm_host::TrackerAndScaler(ctx, P.w, P.h, P.nl, tv, P.K, &prm));
      q.b.reset(new dsm_host::TrackerAndScaler(ctx, P.w, P.h, P.nl, tv, P.K, &prm));
      q.a->makeK(P.K[0], P.K[1], P.K[2], P.K[3]);
      q.b->makeK(P.K[0], P.K[1], P.K[2], P.K[3]);
      q.cur = q.a.get(), q.nxt = q.b.get();
      q.lag = s % (2 * P.kf_every); // the sequences' keyframes do not fall on the same iteration
    }
    dsm_host::Stream stream(ctx, S, std::min(8 * S, 256));
    if (!pipelined) dsm_host::check(dsm_stream_set_pipelined(stream.handle(), 0), "dsm_stream_set_pipelined");
    if (const char *e = getenv("DSM_REPLAY_CHAIN")) stream.setChain(atoi(e)); // (experiments: the library's default otherwise)
    if (const char *e = getenv("DSM_REPLAY_TICKS")) dsm_host::check(dsm_stream_set_engine(stream.handle(), 1, atoi(e)), "dsm_stream_set_engine");
    std::map<uint64_t, std::pair<int, int>> owner; // ticket -> (sequence, index of the scale guess or -1 for the frame's tracking)
    const bool hyp_groups = replay_hypotheses_in_stream();
    int n_done = 0;
    auto left_id = [&](int s, int i) { return (long long)s * 100000000LL + i; };
    auto frame_done = [&](Seq &q) {
      const double ms = ms_since(q.t_start);
      R.latency_ms_sum += ms, R.latency_ms_max = std::max(R.latency_ms_max, ms);
      R.frames++;
      q.frame++;
      q.state = q.frame < P.n_frames ? Seq::IDLE : Seq::DONE;
      n_done += q.state == Seq::DONE;
    };
    auto finish_kf = [&](Seq &q) {
      std::swap(q.cur, q.nxt); // FrontEnd.cpp:627-632
      q.T_kf = q.est_now;
      q.last_rmse0 = 100;
      frame_done(q);
    };
    // frames that became keyframes (their templates are built in ONE call: make_keyframes) and keyframes whose right image is
    // still to be handed over (batched as well: submit_scales)
    std::vector<int> want_kf, want_scale;
    auto finish_track = [&](int s, Seq &q) {
      q.est.push_back(q.est_now);
      q.aff_last = q.aff_now;
      if (q.frame % P.kf_every != 0) return frame_done(q);
      q.state = Seq::SCALING; // (busy until its keyframe is through)
      want_kf.push_back(s);
    };
    auto make_keyframes = [&]() { // makeKeyFrame (FrontEnd.cpp:789-811) for every sequence whose frame just became one
      if (want_kf.empty()) return;
      std::vector<dsm_host::RefRequest> reqs;
      for (int s : want_kf) {
        Seq &q = seqs[s];
        const KeyframeData &k = P.kf.at(q.frame);
        q.views.emplace_back();
        dsm_host::FrameView &ref = q.views.back();
        ref.shell_id = q.frame, ref.unique_id = left_id(s, q.frame), ref.aff_g2l = q.aff_now;
        reqs.push_back(dsm_host::RefRequest{q.nxt, &ref, q.cur, (int)k.pu.size(), k.pu.data(), k.pv.data(), k.pid.data(), k.pw.data()});
      }
      timed("setCoarseTrackingRefs", [&] { dsm_host::setCoarseTrackingRefs(ctx, reqs); });
      const std::vector<int> made = want_kf;
      want_kf.clear();
      for (int s : made) {
        Seq &q = seqs[s];
        q.n_kf++;
        if (q.n_kf <= 4)
          finish_kf(q); // :806
        else
          want_scale.push_back(s);
      }
    };
    auto submit_scales = [&]() { // the right images of this iteration's new keyframes in ONE hand-over, then their scale guesses
      if (want_scale.empty()) return;
      std::vector<dsm_host::TrackerAndScaler *> ts;
      std::vector<int> slots;
      std::vector<const void *> px;
      std::vector<float> ex;
      std::vector<long long> ids;
      for (int s : want_scale) {
        Seq &q = seqs[s];
        ts.push_back(q.nxt), slots.push_back(DSM_SLOT_NEW_RIGHT), px.push_back(right_px.at(q.frame)), ex.push_back(1.0f);
        ids.push_back(left_id(s, q.frame) + 50000000LL);
      }
      timed("hand-over right images", [&] { dsm_host::uploadImages(ctx, ts, slots, px, DSM_PIXEL_U8, ex, ids, 0, true); });
      for (int s : want_scale) {
        Seq &q = seqs[s];
        if (q.trapped)
          q.scale_val = {1.0f}; // FrontEnd.cpp:991-993
        else
          q.scale_val = {0.1f, 1, 5, 10, 15, 25, 30, 50}; // :995-1003
        q.scale_err.assign(q.scale_val.size(), -1.0f);
        q.scale_pending = (int)q.scale_val.size();
        for (size_t g = 0; g < q.scale_val.size(); g++) owner[stream.submitScale(*q.nxt, q.scale_val[g], P.nl - 1)] = {s, (int)g};
      }
      want_scale.clear();
    };
    auto start_frames = [&](int iter) { // every idle sequence's next frame: ONE hand-over for all of them, then their first hypotheses
      for (int guard = 0; guard < 3; guard++) { // (a sequence's frame 0 completes on the spot: its frame 1 follows in the next round)
        std::vector<int> who;
        for (int s = 0; s < S; s++)
          if (seqs[s].state == Seq::IDLE && iter >= seqs[s].lag) who.push_back(s);
        if (who.empty()) return;
        std::vector<dsm_host::TrackerAndScaler *> ts;
        std::vector<int> slots;
        std::vector<const void *> px;
        std::vector<float> ex;
        std::vector<long long> ids;
        const auto t0 = Clock::now();
        for (int s : who) {
          Seq &q = seqs[s];
          q.t_start = t0;
          ts.push_back(q.cur), slots.push_back(DSM_SLOT_NEW_LEFT), px.push_back(left_px[q.frame]), ex.push_back(1.0f), ids.push_back(left_id(s, q.frame));
        }
        timed("hand-over left images", [&] { dsm_host::uploadImages(ctx, ts, slots, px, DSM_PIXEL_U8, ex, ids, 0, true); });
        bool again = false;
        for (int s : who) {
          Seq &q = seqs[s];
          q.aff_now = q.aff_last;
          if (q.frame == 0) {
            q.est_now = P.gt[0]; // the initializer is out of scope: the first frame is at its true pose
            finish_track(s, q);
            again = true;
            continue;
          }
          q.tries = hypothesis_list(q.est, q.T_kf);
          if (hyp_groups)
            owner[stream.submitHypotheses(*q.cur, q.tries, q.aff_last, P.nl - 1, q.last_rmse0)] = {s, -1};
          else
            owner[stream.submitTrack(*q.cur, q.tries[0], q.aff_last, P.nl - 1, nullptr)] = {s, -1};
          q.state = Seq::TRACKING;
        }
        make_keyframes();
        if (!again) return;
      }
    };
    auto settle = [&](int s, Seq &q, const SE3 &pose, const AffLight &aff, double res0, bool have) {
      R.lost += !have;
      q.last_rmse0 = res0;
      q.est_now = se3_mul(pose, q.T_kf);
      q.aff_now = aff;
      finish_track(s, q);
    };
    auto on_track = [&](int s, Seq &q, const dsm_stream_result &r) {
      // the first try of trackHypotheses (FrontEnd.cpp:204-247): nothing achieved yet, so no abort threshold
      const bool good = r.good != 0 && std::isfinite((float)r.last_residuals[0]);
      SE3 pose;
      AffLight aff = q.aff_last;
      double res0 = NAN;
      bool have = false;
      if (good && r.last_residuals[0] < q.last_rmse0 * 1.5) { // settled by the first try (:245-247)
        for (int k = 0; k < 4; k++) pose.q[k] = r.pose[k];
        for (int k = 0; k < 3; k++) pose.t[k] = r.pose[4 + k];
        aff = AffLight(r.aff[0], r.aff[1]);
        res0 = r.last_residuals[0];
        have = true;
      } else { // the rest of the list, as the one-sequence driver runs it
        dsm_host::FrameView fv;
        fv.shell_id = q.frame, fv.unique_id = left_id(s, q.frame);
        const dsm_host::HypothesesResult H = dsm_host::trackHypotheses(ctx, *q.cur, fv, q.tries, q.aff_last, P.nl - 1, q.last_rmse0);
        pose = H.lastF_2_fh, aff = H.aff_g2l, res0 = H.achievedRes[0], have = H.haveOneGood;
        R.fallbacks++;
      }
      settle(s, q, pose, aff, res0, have);
    };
    auto on_hypotheses = [&](int s, Seq &q, const dsm_host::HypothesesResult &H) { // the whole list came back as one group
      R.fallbacks += H.triesUsed > 1;
      settle(s, q, H.lastF_2_fh, H.aff_g2l, H.achievedRes[0], H.haveOneGood);
    };
    auto on_scale = [&](Seq &q, int g, const dsm_stream_result &r) {
      q.scale_val[g] = r.scale, q.scale_err[g] = r.err;
      if (--q.scale_pending > 0) return;
      float new_scale = 1.0f, err = -1.0f;
      if (q.trapped)
        new_scale = q.scale_val[0], err = q.scale_err[0];
      else
        for (size_t j = 0; j < q.scale_val.size(); j++) // the smallest positive error wins, the first on ties (:998-1001)
          if (q.scale_err[j] > 0 && (err < 0 || err > q.scale_err[j])) err = q.scale_err[j], new_scale = q.scale_val[j];
      q.scales.push_back(new_scale);
      bool ok = err < 15.0f; // scale_opt_thres (main.cpp:302)
      if (q.trapped && std::fabs(new_scale - 1.0f) > 0.5f) ok = false;
      q.scale_fails = ok ? 0 : q.scale_fails + 1;
      if (q.scale_fails > 5) q.trapped = false;
      if (ok) {
        timed("scaleCoarseDepthL0", [&] { q.nxt->scaleCoarseDepthL0(new_scale); });
        q.trapped = true;
      }
      finish_kf(q);
    };
    std::vector<dsm_stream_result> res;
    std::vector<std::pair<uint64_t, dsm_host::HypothesesResult>> hres;
    const auto t_all = Clock::now();
    for (int iter = 0; n_done < S; iter++) {
      if (iter > 100 * P.n_frames * 8) throw std::runtime_error("concurrent replay: no progress");
      start_frames(iter);
      submit_scales();
      timed("stream.advance", [&] { stream.advance(); });
      R.advances++;
      res.clear();
      timed("stream.results", [&] { stream.results(res); });
      for (const dsm_stream_result &r : res) {
        const auto it = owner.find(r.ticket);
        if (it == owner.end()) throw std::runtime_error("concurrent replay: unknown ticket");
        const int s = it->second.first, g = it->second.second;
        owner.erase(it);
        if (g < 0)
          on_track(s, seqs[s], r);
        else
          on_scale(seqs[s], g, r);
      }
      if (hyp_groups) {
        hres.clear();
        timed("stream.hypothesesResults", [&] { stream.hypothesesResults(hres); });
        for (const auto &h : hres) {
          const auto it = owner.find(h.first);
          if (it == owner.end()) throw std::runtime_error("concurrent replay: unknown group ticket");
          const int s = it->second.first;
          owner.erase(it);
          on_hypotheses(s, seqs[s], h.second);
        }
      }
      make_keyframes(); // (the frames of this advance's results that became keyframes)
      submit_scales();
    }
    R.wall_ms = ms_since(t_all);
    for (Seq &q : seqs) R.est.push_back(q.est), R.scales.push_back(q.scales);
  }
  dsm_host_free(pinned);
  dsm_context_destroy(ctx);
  return R;
}

// The loop detector alone, on the inputs ANOTHER run recorded: descriptors, search_ringkey, search_sc query by query from the same seeded
// index.  With the CPU path's clouds the device search must return the CPU path's ring keys, candidates and matches bit for bit --
// end-to-end search parity on equal inputs (search_place.h:25-84, ScanContext.cpp:96-141); the candidates of a full replay differ
// only where the two paths' own trajectories (micrometres apart) put a point on either side of a bin edge.
struct LoopReplay {
  std::vector<std::vector<float>> keys;
  std::vector<std::vector<int>> candidates;
  std::vector<int> matched;
};
template <class B>
static LoopReplay replay_loop(B &be, const Pack &P, const std::vector<LoopQuery> &qs) {
  LoopReplay L;
  std::vector<SigType> signatures;
  seed_first_pass(be, P, signatures);
  Timers scratch;
  for (const LoopQuery &q0 : qs) {
    LoopQuery q = q0;
    std::vector<float> key;
    SigType sig;
    be.descriptors(q.ids, q.poses, q.cw, q.pk, q.xyz, key, sig, scratch);
    std::vector<int> cand;
    be.search_ringkey(key, cand);
    int matched = -1;
    float diff = -1;
    if (!cand.empty()) be.search_sc(sig, signatures, cand, matched, diff);
    signatures.push_back(sig);
    L.keys.push_back(key), L.candidates.push_back(cand), L.matched.push_back(matched);
  }
  return L;
}

// Which point changed which polar bin: the two paths' inputs of one query through the product's HOST functions (generate_spherical_points,
// the PCA frame of ScanContext::generate) and ScanContext.cpp:96-117's binning restated with the frame those functions return.
struct BinOfPoint {
  int si, ri;
  double theta_s, rho_r, x, y, z; // position in units of a sector / a ring, and in the window's frame
};
static bool bins_of_query(const LoopQuery &q, double lidar_range, std::vector<BinOfPoint> &out, std::string &why) {
  const int n_kf = (int)q.ids.size(), n_pts = (int)q.pk.size();
  std::vector<int> keep(n_kf), sel(n_pts);
  std::vector<double> sph(3 * (size_t)n_pts);
  int n_out = 0;
  if (dsm_generate_spherical_points(n_kf, q.ids.data(), q.poses.data(), q.cw, lidar_range, n_pts, q.pk.data(), q.xyz.data(), keep.data(), &n_out, sel.data(),
                                    sph.data()) != DSM_OK || n_out < 1) {
    why = "generate_spherical_points failed";
    return false;
  }
  std::vector<float> key(20);
  std::vector<int> sidx(1200);
  std::vector<double> sval(1200);
  int n_sig = 0;
  double tfm[16];
  if (dsm_scancontext_generate(sph.data(), n_out, lidar_range, 60, 20, key.data(), sidx.data(), sval.data(), &n_sig, tfm) != DSM_OK) {
    why = "scancontext_generate failed";
    return false;
  }
  double mx = 0, my = 0, mz = 0; // (as dsm_scancontext_generate: align_points_PCA, ScanContext.cpp:19-66)
  for (int i = 0; i < n_out; i++) mx += sph[3 * i], my += sph[3 * i + 1], mz += sph[3 * i + 2];
  mx /= n_out, my /= n_out, mz /= n_out;
  double V[9];
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) V[c * 3 + r] = tfm[r * 4 + c];
  out.clear();
  for (int i = 0; i < n_out; i++) {
    const double x = sph[3 * i] - mx, y = sph[3 * i + 1] - my, z = sph[3 * i + 2] - mz;
    const double yp = x * V[1] + y * V[4] + z * V[7], zp = x * V[2] + y * V[5] + z * V[8];
    const double rho = std::sqrt(yp * yp + zp * zp);
    double theta = std::atan2(zp, yp);
    while (theta < 0) theta += 2.0 * M_PI;
    while (theta >= 2.0 * M_PI) theta -= 2.0 * M_PI;
    BinOfPoint b;
    b.theta_s = theta / (2.0 * M_PI) * 60, b.rho_r = rho / lidar_range * 20;
    b.si = (int)b.theta_s, b.ri = (int)b.rho_r;
    b.x = sph[3 * i], b.y = sph[3 * i + 1], b.z = sph[3 * i + 2];
    out.push_back(b);
  }
  return true;
}
static void print_candidate_difference(size_t qi, const LoopQuery &g, const LoopQuery &c, double lidar_range) {
  printf("{\"query\": %d, \"ringkey_entries_that_differ\": [", (int)qi);
  bool first = true;
  for (size_t r = 0; r < g.key.size() && r < c.key.size(); r++)
    if (g.key[r] != c.key[r]) printf("%s{\"ring\": %d, \"occupied_sectors_gpu\": %d, \"occupied_sectors_cpu\": %d}", first ? "" : ", ", (int)r, (int)std::lround(g.key[r] * 60),
                                     (int)std::lround(c.key[r] * 60)), first = false;
  printf("], \"points\": [");
  std::vector<BinOfPoint> bg, bc;
  std::string why;
  if (!bins_of_query(g, lidar_range, bg, why) || !bins_of_query(c, lidar_range, bc, why)) {
    printf("], \"note\": \"%s\"}", why.c_str());
    return;
  }
  // occupancy of the 60 x 20 polar grid on both paths; for every bin only one path fills: its point there and the nearest point of the other path
  std::vector<int> og(1200, 0), oc(1200, 0);
  for (const BinOfPoint &b : bg)
    if (b.ri < 20 && b.si < 60) og[b.si * 20 + b.ri]++;
  for (const BinOfPoint &b : bc)
    if (b.ri < 20 && b.si < 60) oc[b.si * 20 + b.ri]++;
  first = true;
  int shown = 0;
  for (int bin = 0; bin < 1200 && shown < 6; bin++) {
    if ((og[bin] > 0) == (oc[bin] > 0)) continue;
    const bool on_gpu = og[bin] > 0;
    const std::vector<BinOfPoint> &A = on_gpu ? bg : bc, &B = on_gpu ? bc : bg;
    for (const BinOfPoint &a : A) {
      if (a.ri >= 20 || a.si * 20 + a.ri != bin) continue;
      double best = 1e300;
      const BinOfPoint *nb = nullptr;
      for (const BinOfPoint &b : B) {
        const double d = (a.x - b.x) * (a.x - b.x) + (a.y - b.y) * (a.y - b.y) + (a.z - b.z) * (a.z - b.z);
        if (d < best) best = d, nb = &b;
      }
      if (!nb) continue;
      printf("%s{\"bin_sector_ring\": [%d, %d], \"filled_on\": \"%s\", \"sector_coordinate\": %.9f, \"ring_coordinate\": %.9f, "
             "\"same_point_on_the_other_path\": {\"moved_m\": %.3g, \"bin_sector_ring\": [%d, %d], \"sector_coordinate\": %.9f, \"ring_coordinate\": %.9f}}",
             first ? "" : ", ", a.si, a.ri, on_gpu ? "gpu" : "cpu", a.theta_s, a.rho_r, std::sqrt(best), nb->si, nb->ri, nb->theta_s, nb->rho_r);
      first = false;
      shown++;
      break;
    }
  }
  printf("], \"spherical_points_gpu\": %d, \"spherical_points_cpu\": %d}", (int)bg.size(), (int)bc.size());
}

static double ate(const std::vector<SE3> &a, const std::vector<SE3> &b) {
  double s = 0;
  for (size_t i = 0; i < a.size(); i++) {
    const SE3 ai = se3_inv(a[i]), bi = se3_inv(b[i]); // camera centres
    for (int c = 0; c < 3; c++) s += (ai.t[c] - bi.t[c]) * (ai.t[c] - bi.t[c]);
  }
  return std::sqrt(s / (double)a.size());
}

// Relative pose error over a step of one frame (the RPE of the TUM / KITTI trajectory tools, delta = 1): with camera-to-world poses
// P_i = est_i^-1 and Q_i = gt_i^-1, E_i = (Q_i^-1 Q_{i+1})^-1 (P_i^-1 P_{i+1}); RMSE of |trans(E_i)| and of the rotation angle of E_i.
// What dslam.txt is compared by next to the ATE (README.md:73-75; the trajectory itself: LoopHandler.cpp:60-80).
struct Rpe {
  double trans_m, rot_deg;
};
static Rpe rpe(const std::vector<SE3> &est, const std::vector<SE3> &gt) {
  double st = 0, sr = 0;
  size_t n = 0;
  for (size_t i = 0; i + 1 < est.size() && i + 1 < gt.size(); i++, n++) {
    const SE3 dp = se3_mul(est[i], se3_inv(est[i + 1])); // P_i^-1 P_{i+1} with P = est^-1
    const SE3 dq = se3_mul(gt[i], se3_inv(gt[i + 1]));
    const SE3 e = se3_mul(se3_inv(dq), dp);
    st += e.t[0] * e.t[0] + e.t[1] * e.t[1] + e.t[2] * e.t[2];
    const double sn = std::sqrt(e.q[0] * e.q[0] + e.q[1] * e.q[1] + e.q[2] * e.q[2]);
    const double ang = 2.0 * std::atan2(sn, std::fabs(e.q[3]));
    sr += ang * ang;
  }
  if (!n) return Rpe{0, 0};
  return Rpe{std::sqrt(st / (double)n), std::sqrt(sr / (double)n) * 180.0 / M_PI};
}

static void print_result(const char *name, const RunResult &R, const Pack &P, const std::string &traj_path) {
  printf("\"%s\": {\"stages_mean_ms\": {", name);
  bool first = true;
  for (auto &kv : R.tm.t) {
    printf("%s\"%s\": {\"mean_ms\": %.5f, \"calls\": %d}", first ? "" : ", ", kv.first.c_str(), kv.second.first / kv.second.second, kv.second.second);
    first = false;
  }
  int with_cand = 0, twin = 0;
  for (size_t i = 0; i < R.candidates.size(); i++) {
    with_cand += !R.candidates[i].empty();
    twin += R.matched[i] == (int)i; // the first pass's keyframe of the same place
  }
  const Rpe rp = rpe(R.est, P.gt);
  printf("}, \"frames\": %d, \"keyframes\": %d, \"hypothesis_tries\": %d, \"frames_needing_retries\": %d, \"frames_lost\": %d, \"ate_vs_ground_truth_m\": %.6g, "
         "\"rpe_vs_ground_truth\": {\"delta_frames\": 1, \"trans_rmse_m\": %.6g, \"rot_rmse_deg\": %.6g}, "
         "\"loop_queries\": %d, \"queries_with_candidates\": %d, \"search_sc_matches_the_first_pass_twin\": %d, \"trajectory\": \"%s\"}",
         P.n_frames, (P.n_frames + P.kf_every - 1) / P.kf_every, R.tries_total, R.frames_with_retries, R.lost, ate(R.est, P.gt), rp.trans_m, rp.rot_deg,
         (int)R.candidates.size(), with_cand, twin, traj_path.c_str());
}

int main(int argc, char **argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: %s pack.bin out_prefix [gpu|cpu|both [concurrent_sequences [pipelined 0|1]]]\n", argv[0]);
    return 2;
  }
  const std::string which = argc > 3 ? argv[3] : "both";
  const Pack P = load_pack(argv[1]);
  const std::string prefix = argv[2];
  const int n_concurrent = argc > 4 ? atoi(argv[4]) : 0;
  const bool conc_pipelined = argc > 5 ? atoi(argv[5]) != 0 : true;
  RunResult rg, rc, rg_conc; // (rg_conc: the one-sequence reference of the concurrent leg, under that leg's chunk table)
  LoopReplay eq;
  bool have_eq = false;
  ConcurrentResult cc;
  bool have_g = false, have_c = false;
  std::vector<int> ids(P.n_frames);
  for (int i = 0; i < P.n_frames; i++) ids[i] = i;
  auto centres = [](const std::vector<SE3> &est) {
    std::vector<double> t;
    for (const SE3 &T : est) {
      const SE3 inv = se3_inv(T);
      t.insert(t.end(), inv.t, inv.t + 3);
    }
    return t;
  };
  try {
    if (which != "cpu") {
      GpuBackend be(P);
      { // one untimed pass warms the launch schedules and the allocators, as a long-running node would be
        RunResult warm = run(be, P);
        (void)warm;
      }
    }
    if (which != "cpu") {
      GpuBackend be(P);
      rg = run(be, P);
      have_g = true;
      dsm_host::save_trajectory((prefix + "_dslam_gpu.txt").c_str(), ids, centres(rg.est)); // LoopHandler.cpp:59-80
    }
    if (which != "cpu" && n_concurrent > 0) {
      const int cg = replay_concurrent_geometry();
      if (cg != replay_geometry()) { // another chunk table than the one-sequence run's: the float sums' last bits differ, so the leg is
                                     // compared (bit for bit) with a one-sequence run under ITS table (untimed)
        g_geometry_override = cg;
        GpuBackend be(P);
        rg_conc = run(be, P);
      } else {
        rg_conc = rg;
      }
      (void)run_concurrent(P, n_concurrent, conc_pipelined); // untimed: schedules, allocators, the stream's learnt life of a problem
      cc = run_concurrent(P, n_concurrent, conc_pipelined);
      g_geometry_override = -1;
    }
    if (which != "gpu") {
      CpuBackend be(P);
      rc = run(be, P);
      have_c = true;
      dsm_host::save_trajectory((prefix + "_dslam_cpu.txt").c_str(), ids, centres(rc.est));
    }
    if (have_g && have_c) { // the device loop detector on the CPU path's recorded clouds
      GpuBackend be(P);
      eq = replay_loop(be, P, rc.queries);
      have_eq = true;
    }
  } catch (const std::exception &e) {
    fprintf(stderr, "replay_bench: %s\n", e.what());
    return 3;
  }
  printf("{\"workload\": \"one synthetic stereo sequence, %d frames %dx%d, %d pyramid levels, keyframe every %d frames, %d active points per keyframe (semi-dense template), "
         "one frame in flight, driven from the C++ adaptors\", ",
         P.n_frames, P.w, P.h, P.nl, P.kf_every, P.n_active);
  if (have_g) print_result("gpu", rg, P, prefix + "_dslam_gpu.txt");
  if (have_g && have_c) printf(", ");
  if (have_c) print_result("cpu", rc, P, prefix + "_dslam_cpu.txt");
  if (have_g && have_c) {
    double dmax = 0;
    for (size_t i = 0; i < rg.est.size(); i++) {
      const SE3 a = se3_inv(rg.est[i]), b = se3_inv(rc.est[i]);
      for (int c = 0; c < 3; c++) dmax = std::fmax(dmax, std::fabs(a.t[c] - b.t[c]));
    }
    // (each path describes the places from ITS OWN estimated poses: where the two trajectories differ in the last digits a point
    // can change its polar bin, so the candidate lists are compared query by query, not required to be equal)
    int same_cand = 0, same_match = 0;
    for (size_t i = 0; i < rg.candidates.size() && i < rc.candidates.size(); i++) {
      same_cand += rg.candidates[i] == rc.candidates[i];
      same_match += rg.matched[i] == rc.matched[i];
    }
    const Rpe rpg = rpe(rg.est, P.gt), rpc = rpe(rc.est, P.gt), rpd = rpe(rg.est, rc.est); // (rpd: the GPU path's steps against the CPU path's own)
    printf(", \"gpu_vs_cpu\": {\"max_abs_trajectory_diff_m\": %.6g, \"ate_ratio_gpu_over_cpu\": %.6f, \"rpe_trans_ratio_gpu_over_cpu\": %.6f, "
           "\"rpe_rot_ratio_gpu_over_cpu\": %.6f, \"rpe_gpu_against_cpu_trans_m\": %.6g, \"rpe_gpu_against_cpu_rot_deg\": %.6g, \"loop_queries\": %d, "
           "\"queries_with_identical_candidates\": %d, \"queries_with_identical_search_sc_match\": %d}",
           dmax, ate(rg.est, P.gt) / std::fmax(ate(rc.est, P.gt), 1e-30), rpg.trans_m / std::fmax(rpc.trans_m, 1e-30), rpg.rot_deg / std::fmax(rpc.rot_deg, 1e-30),
           rpd.trans_m, rpd.rot_deg, (int)rg.candidates.size(), same_cand, same_match);
    if (have_eq) {
      int keys_eq = 0, cand_eq = 0, match_eq = 0;
      for (size_t i = 0; i < eq.candidates.size() && i < rc.candidates.size(); i++) {
        keys_eq += eq.keys[i].size() == rc.queries[i].key.size() && memcmp(eq.keys[i].data(), rc.queries[i].key.data(), sizeof(float) * eq.keys[i].size()) == 0;
        cand_eq += eq.candidates[i] == rc.candidates[i];
        match_eq += eq.matched[i] == rc.matched[i];
      }
      printf(", \"device_search_on_the_cpu_paths_clouds\": {\"what\": \"descriptors + search_ringkey + search_sc of the device path fed with the inputs the CPU path recorded "
             "(equal inputs: must be equal bit for bit)\", \"queries\": %d, \"ring_keys_bit_equal\": %d, \"identical_candidates\": %d, \"identical_search_sc_match\": %d}",
             (int)eq.candidates.size(), keys_eq, cand_eq, match_eq);
    }
    printf(", \"candidate_differences_of_the_full_replay\": [");
    bool first_diff = true;
    for (size_t i = 0; i < rg.candidates.size() && i < rc.candidates.size(); i++)
      if (rg.candidates[i] != rc.candidates[i] || rg.queries[i].key != rc.queries[i].key) {
        if (!first_diff) printf(", ");
        first_diff = false;
        print_candidate_difference(i, rg.queries[i], rc.queries[i], P.lidar_range);
      }
    printf("]");
  }
  if (have_g && cc.sequences > 0) {
    double dmax = 0, ate_max = 0;
    bool scales_equal = true;
    for (const std::vector<SE3> &e : cc.est) {
      ate_max = std::fmax(ate_max, ate(e, P.gt));
      for (size_t i = 0; i < e.size() && i < rg_conc.est.size(); i++) {
        const SE3 a = se3_inv(e[i]), b = se3_inv(rg_conc.est[i]);
        for (int c = 0; c < 3; c++) dmax = std::fmax(dmax, std::fabs(a.t[c] - b.t[c]));
      }
    }
    for (const std::vector<float> &sc : cc.scales) scales_equal = scales_equal && sc == rg_conc.scales;
    printf(", \"concurrent\": {\"what\": \"%d sequences (the same frames, keyframes out of phase) through ONE dsm_host::Stream from C++: per sequence one problem in flight "
           "(a frame's first hypothesis, or its keyframe's scale guesses), hand-over, setCoarseTrackingRef and tracker swap as in the one-sequence run; no loop descriptors; "
           "chunk table %d (compared bit for bit with a one-sequence run under the same table)\", "
           "\"sequences\": %d, \"pipelined_advances\": %s, \"frames\": %lld, \"wall_ms\": %.3f, \"frames_per_s\": %.1f, \"ms_per_frame_of_one_sequence\": %.4f, "
           "\"mean_frame_latency_ms\": %.4f, \"max_frame_latency_ms\": %.4f, \"advances\": %d, \"frames_through_the_whole_hypothesis_list\": %d, \"frames_lost\": %d, "
           "\"max_ate_vs_ground_truth_m\": %.6g, \"max_abs_trajectory_diff_vs_the_one_sequence_run_m\": %.6g, \"scales_equal_the_one_sequence_run\": %s",
           cc.sequences, replay_concurrent_geometry(), cc.sequences, conc_pipelined ? "true" : "false", cc.frames, cc.wall_ms, 1e3 * (double)cc.frames / cc.wall_ms,
           cc.wall_ms * cc.sequences / (double)cc.frames, cc.latency_ms_sum / (double)cc.frames, cc.latency_ms_max, cc.advances, cc.fallbacks, cc.lost, ate_max, dmax,
           scales_equal ? "true" : "false");
    if (replay_hypotheses_in_stream()) printf(", \"hypothesis_lists_as_stream_groups\": true");
    printf(", \"host_ms_per_advance_by_call\": {");
    bool first = true;
    for (const auto &kv : cc.host_ms) printf("%s\"%s\": %.4f", first ? "" : ", ", kv.first.c_str(), kv.second / std::max(1, cc.advances)), first = false;
    printf("%s\"whole loop\": %.4f}}", first ? "" : ", ", cc.wall_ms / std::max(1, cc.advances));
  }
  printf("}\n");
  return 0;
}
