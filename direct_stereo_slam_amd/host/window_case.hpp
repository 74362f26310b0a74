// window_case.hpp -- the binary case files of the window-optimisation family, read in one place: what the demos of this directory and
// the stand-alone CPU programs under tools/ take as input.  tests/_window_files.py writes them; the two are the definition of the format.
// Plain C++11; needs nothing but include/dsm_hotpath.h.  window_case_requests.hpp turns a Case into the adaptors' requests.
//
// A file is a sequence of sections (native byte order; nf frames, n points, nr residuals, N = 4 + 8 nf):
//   kind         sections
//   WINDOW       prefix
//   HESSIAN      prefix, hessian tail of 8 floats per point
//   SOLVE        prefix, hessian tail (8), solve tail in the solve form
//   NULLSPACE    prefix, hessian tail (8), solve tail in the solve form, two pose records
//   STEP         prefix, hessian tail (8), solve tail in the step form, step tail.  cam, the precalc rows and the points' depths are zeros
//                in such a file, and delta is not used: the call forms them (formed())
//   FINISH       a STEP file, then the finish tail
//   MARGINALIZE  prefix, hessian tail of 2 floats per point, marginalize tail
// Each read_* below reads one section and is the description of its layout.
//
// Every array ends up in a heap block of exactly its length: Reader::take mallocs n elements and reads into them, the records of a
// section are split into one such block per field, and a plane is a block of its own.  Nothing is pooled or rounded up, so a sanitizer
// build of a program that hands these blocks to the library sees an access one element past any end.  Nothing is freed.
#pragma once
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/dsm_hotpath.h"

namespace window_case {

inline static uint64_t fnv1a(const void *p, size_t n, uint64_t hsh = 1469598103934665603ull) {
  for (size_t i = 0; i < n; i++) hsh = (hsh ^ ((const unsigned char *)p)[i]) * 1099511628211ull;
  return hsh;
}
template <typename T>
uint64_t vhash(const std::vector<T> &v, uint64_t hsh = 1469598103934665603ull) {
  return fnv1a(v.data(), sizeof(T) * v.size(), hsh);
}

template <typename T>
T *block(size_t n) { // exactly n elements, so that the sanitizer sees every access past an end
  return (T *)malloc(n ? n * sizeof(T) : 1);
}
template <typename T>
T *block(size_t n, T fill) {
  T *p = block<T>(n);
  for (size_t i = 0; i < n; i++) p[i] = fill;
  return p;
}
template <typename T>
T *read_block(FILE *f, size_t n, const char *program) {
  T *p = block<T>(n);
  if (n && fread(p, sizeof(T), n, f) != n) {
    fprintf(stderr, "%s: short file\n", program);
    exit(2);
  }
  return p;
}
template <typename T>
bool rd(FILE *f, std::vector<T> &v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

// rows / columns 0..3 and those of the frames in `stay`, of an N-vector or an N x N matrix (empty stays empty)
inline std::vector<double> cut(const std::vector<double> &v, const std::vector<int> &stay, size_t N, bool matrix) {
  std::vector<int> idx = {0, 1, 2, 3};
  for (int f : stay)
    for (int k = 0; k < 8; k++) idx.push_back(4 + 8 * f + k);
  std::vector<double> out;
  if (v.empty()) return out;
  for (int i : idx) {
    if (!matrix) out.push_back(v[i]);
    else
      for (int j : idx) out.push_back(v[(size_t)i * N + j]);
  }
  return out;
}
template <typename T>
std::vector<T> per_frame(const std::vector<T> &v, const std::vector<int> &stay, size_t width) {
  std::vector<T> out;
  for (int f : stay) out.insert(out.end(), v.begin() + f * width, v.begin() + (f + 1) * width);
  return out;
}

// once a read came short or a count was out of range, nothing more is read and every later block is empty
struct Reader {
  FILE *f;
  bool ok;
  explicit Reader(const char *path) : f(path ? fopen(path, "rb") : nullptr), ok(f != nullptr) {}
  ~Reader() {
    if (f) fclose(f);
  }
  template <typename T>
  T *take(size_t n) {
    T *p = block<T>(ok ? n : 0);
    if (ok && n && fread(p, sizeof(T), n, f) != n) ok = false;
    return p;
  }
  template <typename T>
  T one() {
    T v = T();
    if (ok && fread(&v, sizeof(T), 1, f) != 1) ok = false;
    return ok ? v : T();
  }
  size_t count(int lo, int hi) { // an int32 in lo..hi; otherwise the read has failed, and lo
    const int v = one<int>();
    if (ok && (v < lo || v > hi)) ok = false;
    return (size_t)(ok ? v : lo);
  }
  bool flag() { return one<int>() != 0; }
  // field `at` .. `at + width` of n records of `stride` words, as a block of its own
  template <typename T>
  static T *column(const float *records, size_t n, size_t stride, size_t at, size_t width = 1) {
    T *p = block<T>(n * width);
    for (size_t i = 0; i < n; i++) memcpy(p + i * width, records + i * stride + at, 4 * width);
    return p;
  }
  static unsigned char *bytes(const float *records, size_t n, size_t stride, size_t at) { // an int32 field, narrowed
    unsigned char *p = block<unsigned char>(n);
    for (size_t i = 0; i < n; i++) {
      int v;
      memcpy(&v, records + i * stride + at, 4);
      p[i] = (unsigned char)v;
    }
    return p;
  }
};

enum Kind { WINDOW, HESSIAN, SOLVE, NULLSPACE, STEP, FINISH, MARGINALIZE };

struct Pose {
  double *world_to_cam_eval, *state_zero; // nf * 7, nf * 8
  float *exposure;                        // nf
};

struct Case {
  Kind kind;
  size_t nf, n, nr, N, nm;
  // prefix
  int w, h, fix_linearization;
  float *cam; // cam[4], cam_inv[2]
  int *frame_ids;
  const float **planes;
  float *pre[6]; // pre_RTll_0, pre_tTll_0, pre_KRKiTll, pre_KtTll, pre_aff_mode, pre_b0_mode
  float *frame_energy_th;
  int *host, *point, *target;
  float *u, *v, *idepth_scaled, *idepth_zero_scaled, *color, *weights, *energy_in;
  unsigned char *state_in, *is_new;
  // hessian tail
  double *ad_host, *ad_target;
  float *prior, *delta, *hdd_lin, *bd_lin, *hcd_lin;
  int shift_prior_to_zero;
  // solve tail (H_M, b_M also of the marginalize tail; null where the file has none)
  double *H_L, *b_L, *H_M, *b_M, *delta_x, *null_basis, *null_pinv, lambda;
  int n_null;
  // step tail (the priors null where the file has none)
  double *world_to_cam_eval, *state_zero, *state_backup, *frame_step, *calib_zero, *calib_backup, *calib_step, *state_prior, *state_prior_zero;
  float *idepth_backup, *idepth_step, *exposure, *stepfac;
  // finish tail
  int *n_good_residuals_in, *last_res;
  float *max_rel_baseline_in;
  unsigned char *last_state_in;
  // marginalize tail
  unsigned char *flagged, *last_state;
  int *n_good_residuals, *marg_frames;
  float *idepth_hessian, *ad_ht_delta, *c_delta;
  double *frame_prior, *frame_delta_prior;
  // the nullspace demo's pose records
  Pose poses[2];

  Case() { memset(this, 0, sizeof *this); }
  bool formed() const { return kind == STEP || kind == FINISH; } // the call forms cam, the precalc rows, the depths and delta
};

// int32 w, h; float cam[4], cam_inv[2]; int32 nf, fix_linearization; nf int32 frame ids; nf planes of w * h floats; nf * nf precalc rows
// of 27 floats, [host][target]; nf floats frameEnergyTH; int32 n; n point records of 21 words (int32 host; float u, v, idepth_scaled,
// idepth_zero_scaled, color[8], weights[8]); int32 nr; nr residual records of 5 words (int32 point, target, state; float energy; int32 isNew)
inline void read_prefix(Reader &r, Case &c) {
  c.w = (int)r.count(1, INT_MAX), c.h = (int)r.count(1, INT_MAX);
  c.cam = r.take<float>(6);
  c.nf = r.count(1, DSM_WINDOW_MAX_FRAMES), c.fix_linearization = r.one<int>(), c.N = 4 + 8 * c.nf;
  c.frame_ids = r.take<int>(c.nf);
  c.planes = block<const float *>(c.nf);
  for (size_t k = 0; k < c.nf; k++) c.planes[k] = r.take<float>((size_t)c.w * c.h);
  const size_t n2 = c.nf * c.nf, width[6] = {9, 3, 9, 3, 2, 1};
  float *rows = r.take<float>(n2 * 27);
  for (size_t k = 0, at = 0; k < 6; at += width[k], k++) c.pre[k] = Reader::column<float>(rows, r.ok ? n2 : 0, 27, at, width[k]);
  c.frame_energy_th = r.take<float>(c.nf);
  c.n = r.count(0, INT_MAX);
  float *q = r.take<float>(c.n * 21);
  const size_t n = r.ok ? c.n : 0;
  c.host = Reader::column<int>(q, n, 21, 0), c.u = Reader::column<float>(q, n, 21, 1), c.v = Reader::column<float>(q, n, 21, 2);
  c.idepth_scaled = Reader::column<float>(q, n, 21, 3), c.idepth_zero_scaled = Reader::column<float>(q, n, 21, 4);
  c.color = Reader::column<float>(q, n, 21, 5, 8), c.weights = Reader::column<float>(q, n, 21, 13, 8);
  c.nr = r.count(0, INT_MAX);
  float *s = r.take<float>(c.nr * 5);
  const size_t nr = r.ok ? c.nr : 0;
  c.point = Reader::column<int>(s, nr, 5, 0), c.target = Reader::column<int>(s, nr, 5, 1), c.state_in = Reader::bytes(s, nr, 5, 2);
  c.energy_in = Reader::column<float>(s, nr, 5, 3), c.is_new = Reader::bytes(s, nr, 5, 4);
  free(rows), free(q), free(s);
}

// nf * nf * 64 doubles adHost, as many adTarget; per point `width` floats: (priorF, deltaF) for width 2, (priorF, deltaF, Hdd_accLF,
// bd_accLF, Hcd_accLF[4]) for width 8; for width 8 then int32 shiftPriorToZero
inline void read_hessian_tail(Reader &r, Case &c, size_t width) {
  c.ad_host = r.take<double>(c.nf * c.nf * 64), c.ad_target = r.take<double>(c.nf * c.nf * 64);
  float *q = r.take<float>(c.n * width);
  const size_t n = r.ok ? c.n : 0;
  c.prior = Reader::column<float>(q, n, width, 0), c.delta = Reader::column<float>(q, n, width, 1);
  if (width == 8) {
    c.hdd_lin = Reader::column<float>(q, n, 8, 2), c.bd_lin = Reader::column<float>(q, n, 8, 3), c.hcd_lin = Reader::column<float>(q, n, 8, 4, 4);
    c.shift_prior_to_zero = r.one<int>();
  }
  free(q);
}

// N * N doubles H_L, N b_L; in the solve form N * N H_M, N b_M, N deltaX; in the step form an int32 flag and, if it is set, H_M and b_M
// (no deltaX: the call forms it); then one double lambda, int32 n_null <= DSM_SOLVE_MAX_NULL, N * n_null doubles nullBasis, as many nullPinv
inline void read_solve_tail(Reader &r, Case &c, bool step_form) {
  c.H_L = r.take<double>(c.N * c.N), c.b_L = r.take<double>(c.N);
  if (!step_form || r.flag()) c.H_M = r.take<double>(c.N * c.N), c.b_M = r.take<double>(c.N);
  if (!step_form) c.delta_x = r.take<double>(c.N);
  c.lambda = r.one<double>(), c.n_null = (int)r.count(0, DSM_SOLVE_MAX_NULL);
  c.null_basis = r.take<double>(c.N * c.n_null), c.null_pinv = r.take<double>(c.N * c.n_null);
}

// doubles worldToCamEval[nf * 7], stateZero[nf * 8], state_backup[nf * 8], frame_step[nf * 8], calib_zero[4], calib_backup[4],
// calib_step[4]; floats idepth_backup[n], idepth_step[n], exposure[nf], stepfac[5]; an int32 flag and, if it is set, N doubles prior
// and N priorZero
inline void read_step_tail(Reader &r, Case &c) {
  c.world_to_cam_eval = r.take<double>(7 * c.nf), c.state_zero = r.take<double>(8 * c.nf), c.state_backup = r.take<double>(8 * c.nf);
  c.frame_step = r.take<double>(8 * c.nf), c.calib_zero = r.take<double>(4), c.calib_backup = r.take<double>(4), c.calib_step = r.take<double>(4);
  c.idepth_backup = r.take<float>(c.n), c.idepth_step = r.take<float>(c.n), c.exposure = r.take<float>(c.nf), c.stepfac = r.take<float>(5);
  if (r.flag()) c.state_prior = r.take<double>(c.N), c.state_prior_zero = r.take<double>(c.N);
}

// per point int32 numGoodResiduals, float maxRelBaseline, the two int32 last residual indices, the two last states as bytes
inline void read_finish_tail(Reader &r, Case &c) {
  c.n_good_residuals_in = r.take<int>(c.n), c.max_rel_baseline_in = r.take<float>(c.n), c.last_res = r.take<int>(2 * c.n);
  c.last_state_in = r.take<unsigned char>(2 * c.n);
}

// nf bytes flaggedForMarginalization; per point int32 numGoodResiduals, the two last states as bytes, float idepth_hessian; nf * nf * 8
// floats adHTdeltaF; cDeltaF[4]; an int32 flag and, if it is set, H_M and b_M; int32 nm <= nf; nm int32 marginalised frames, 8 nm doubles
// framePrior, as many frameDeltaPrior
inline void read_marginalize_tail(Reader &r, Case &c) {
  c.flagged = r.take<unsigned char>(c.nf), c.n_good_residuals = r.take<int>(c.n), c.last_state = r.take<unsigned char>(2 * c.n);
  c.idepth_hessian = r.take<float>(c.n), c.ad_ht_delta = r.take<float>(c.nf * c.nf * 8), c.c_delta = r.take<float>(4);
  if (r.flag()) c.H_M = r.take<double>(c.N * c.N), c.b_M = r.take<double>(c.N);
  c.nm = r.count(0, (int)c.nf), c.marg_frames = r.take<int>(c.nm);
  c.frame_prior = r.take<double>(8 * c.nm), c.frame_delta_prior = r.take<double>(8 * c.nm);
}

// twice: nf * 7 doubles worldToCamEval, nf * 8 stateZero, nf floats exposure
inline void read_poses(Reader &r, Case &c) {
  for (Pose &p : c.poses) p.world_to_cam_eval = r.take<double>(7 * c.nf), p.state_zero = r.take<double>(8 * c.nf), p.exposure = r.take<float>(c.nf);
}

// false: no such file, a short file, or a count out of range
inline bool read_case(const char *path, Kind kind, Case &c) {
  Reader r(path);
  c.kind = kind;
  read_prefix(r, c);
  if (kind != WINDOW) read_hessian_tail(r, c, kind == MARGINALIZE ? 2 : 8);
  if (kind == SOLVE || kind == NULLSPACE || kind == STEP || kind == FINISH) read_solve_tail(r, c, c.formed());
  if (c.formed()) read_step_tail(r, c);
  if (kind == FINISH) read_finish_tail(r, c);
  if (kind == MARGINALIZE) read_marginalize_tail(r, c);
  if (kind == NULLSPACE) read_poses(r, c);
  return r.ok;
}

// ---- the C job structs, for the stand-alone programs --------------------------------------------------------------------------------
// fill(): a job's inputs from the case.  The *_outputs(): a job's outputs, each a block of exactly the length the call may write, filled
// as the ctypes mirror of the tests fills them (bytes 77, numbers -7), so that what a call leaves alone hashes alike.

inline void fill(dsm_linearize_job &J, const Case &c) {
  J.n_frames = (int)c.nf, J.fix_linearization = c.fix_linearization, J.frame_ids = c.frame_ids, J.frame_energy_th = c.frame_energy_th;
  J.n_pts = (int)c.n, J.host = c.host, J.u = c.u, J.v = c.v, J.color = c.color, J.weights = c.weights;
  J.n_res = (int)c.nr, J.point = c.point, J.target = c.target, J.state_in = c.state_in, J.energy_in = c.energy_in, J.is_new = c.is_new;
  if (c.formed()) return;
  memcpy(J.cam, c.cam, 16), memcpy(J.cam_inv, c.cam + 4, 8);
  J.pre_RTll_0 = c.pre[0], J.pre_tTll_0 = c.pre[1], J.pre_KRKiTll = c.pre[2], J.pre_KtTll = c.pre[3], J.pre_aff_mode = c.pre[4], J.pre_b0_mode = c.pre[5];
  J.idepth_scaled = c.idepth_scaled, J.idepth_zero_scaled = c.idepth_zero_scaled;
}
inline void fill(dsm_hessian_job &H, const Case &c) {
  fill(H.lin, c);
  H.ad_host = c.ad_host, H.ad_target = c.ad_target, H.prior = c.prior, H.delta = c.formed() ? nullptr : c.delta;
  H.hdd_lin = c.hdd_lin, H.bd_lin = c.bd_lin, H.hcd_lin = c.hcd_lin, H.shift_prior_to_zero = c.shift_prior_to_zero;
}
inline void fill(dsm_solve_job &S, const Case &c) {
  fill(S.hes, c);
  S.H_L = c.H_L, S.b_L = c.b_L, S.H_M = c.H_M, S.b_M = c.b_M, S.delta_x = c.delta_x, S.lambda = c.lambda, S.n_null = c.n_null;
  S.null_basis = c.null_basis, S.null_pinv = c.null_pinv;
}
// steps: also the file's frame_step, calib_step and idepth_step (a loop forms its own)
inline void fill(dsm_step_job &T, const Case &c, bool steps) {
  fill(T.sol, c);
  T.world_to_cam_eval = c.world_to_cam_eval, T.state_zero = c.state_zero, T.state_backup = c.state_backup, T.calib_zero = c.calib_zero;
  T.calib_backup = c.calib_backup, T.idepth_backup = c.idepth_backup, T.exposure = c.exposure, T.prior = c.state_prior, T.prior_zero = c.state_prior_zero;
  memcpy(T.stepfac, c.stepfac, 20);
  if (steps) T.frame_step = c.frame_step, T.calib_step = c.calib_step, T.idepth_step = c.idepth_step;
}
inline void fill(dsm_finish_job &F, const Case &c) {
  fill(F.opt.step, c, false);
  F.n_good_residuals_in = c.n_good_residuals_in, F.max_rel_baseline_in = c.max_rel_baseline_in, F.last_res = c.last_res, F.last_state_in = c.last_state_in;
}
inline void fill(dsm_marginalize_job &M, const Case &c) {
  fill(M.hes, c);
  M.flagged = c.flagged, M.n_good_residuals = c.n_good_residuals, M.last_state = c.last_state, M.idepth_hessian = c.idepth_hessian;
  M.ad_ht_delta = c.ad_ht_delta, M.c_delta = c.c_delta, M.H_M = c.H_M, M.b_M = c.b_M, M.n_marg_frames = (int)c.nm, M.marg_frames = c.marg_frames;
  M.frame_prior = c.frame_prior, M.frame_delta_prior = c.frame_delta_prior;
}

template <typename T>
T *out(size_t n) {
  return block<T>(n, sizeof(T) == 1 ? (T)77 : (T)-7);
}
inline void linearize_outputs(dsm_linearize_job &J, const Case &c) { // the required ones
  J.new_state = out<unsigned char>(c.nr), J.new_energy = out<float>(c.nr), J.new_energy_with_outlier = out<float>(c.nr);
  J.energy_out = out<double>(1), J.new_frame_energy_th_out = out<float>(1);
}
inline void linearize_optional(dsm_linearize_job &J, const Case &c, bool keep_and_rel_bs, bool rows) {
  J.center_projected_to = out<float>(3 * c.nr), J.projected_to = out<float>(16 * c.nr);
  if (keep_and_rel_bs) J.keep = out<unsigned char>(c.nr), J.rel_bs = out<float>(c.nr);
  if (rows) J.J_out = out<float>((size_t)DSM_LINEARIZE_J_FLOATS * c.nr);
}
inline void hessian_optional(dsm_hessian_job &H, const Case &c, bool raw) { // raw: also the accumulators before stitching
  const size_t N = c.N, n2 = c.nf * c.nf;
  H.H_A = out<double>(N * N), H.b_A = out<double>(N), H.H_sc = out<double>(N * N), H.b_sc = out<double>(N);
  if (raw) {
    H.acc_top = out<double>(n2 * 169), H.acc_D = out<double>(n2 * c.nf * 64), H.acc_E = out<double>(n2 * 32), H.acc_EB = out<double>(n2 * 8);
    H.acc_Hcc = out<double>(16), H.acc_bc = out<double>(4);
  }
  H.active = out<unsigned char>(c.nr), H.JpJdF = out<float>(8 * c.nr);
  H.hdd_acc = out<float>(c.n), H.bd_acc = out<float>(c.n), H.hcd_acc = out<float>(4 * c.n), H.hdi = out<float>(c.n), H.bd_sum = out<float>(c.n);
  H.idepth_hessian = out<float>(c.n);
}
inline void solve_outputs(dsm_solve_job &S, const Case &c) {
  linearize_outputs(S.hes.lin, c);
  S.x = out<double>(c.N), S.step = out<float>(c.n), S.flags = out<int>(1);
}
inline void solve_optional(dsm_solve_job &S, const Case &c) { S.last_HS = out<double>(c.N * c.N), S.last_bS = out<double>(c.N); }
inline void step_outputs(dsm_step_job &T, const Case &c) {
  solve_outputs(T.sol, c);
  T.state_out = out<double>(8 * c.nf), T.calib_out = out<double>(4), T.idepth_out = out<float>(c.n), T.world_to_cam_out = out<double>(7 * c.nf);
  T.can_break = out<int>(1), T.step_sums = out<float>(6), T.energy_m = out<double>(1);
}
inline void step_optional(dsm_step_job &T, const Case &c) {
  const size_t n2 = c.nf * c.nf;
  T.cam_to_world_out = out<double>(7 * c.nf), T.cam_out = out<float>(6);
  T.pre_RTll_0_out = out<float>(9 * n2), T.pre_tTll_0_out = out<float>(3 * n2), T.pre_KRKiTll_out = out<float>(9 * n2);
  T.pre_KtTll_out = out<float>(3 * n2), T.pre_aff_mode_out = out<float>(2 * n2), T.pre_b0_mode_out = out<float>(n2);
  T.delta_x_out = out<double>(c.N), T.H_L_out = out<double>(c.N * c.N), T.b_L_out = out<double>(c.N);
}
inline void optimize_outputs(dsm_optimize_job &O, const Case &c, int max_its) {
  step_outputs(O.step, c);
  const size_t its = (size_t)(max_its > 0 ? max_its : 0), passes = 1 + 2 * its;
  O.max_iterations = max_its, O.n_iterations = out<int>(1), O.n_passes = out<int>(1), O.pattern = out<unsigned char>(its);
  O.pass_energy = out<double>(2 * passes), O.pass_lambda = out<double>(passes), O.iter_stepsize = out<float>(its);
  O.iter_can_break = out<unsigned char>(its), O.last_energy = out<double>(2), O.lambda_out = out<double>(1), O.frame_energy_th_out = out<float>(1);
}
// the six precalc tables of n2 pairs, hashed as the checkers hash them
inline uint64_t tables_hash(const float *RT, const float *tT, const float *KRKi, const float *Kt, const float *aff, const float *b0, size_t n2) {
  return fnv1a(RT, 36 * n2) ^ fnv1a(tT, 12 * n2) ^ fnv1a(KRKi, 36 * n2) ^ fnv1a(Kt, 12 * n2) ^ fnv1a(aff, 8 * n2) ^ fnv1a(b0, 4 * n2);
}

#ifdef WINDOW_CASE_STANDALONE
// a stand-alone program's case: usage and exit status 2 without a file, "short file" and exit status 2 where read_case fails
inline void open_case(const char *program, int argc, char **argv, Kind kind, Case &c) {
  FILE *f = argc > 1 ? fopen(argv[1], "rb") : nullptr;
  if (!f) {
    fprintf(stderr, "usage: %s FILE\n", program);
    exit(2);
  }
  fclose(f);
  if (!read_case(argv[1], kind, c)) {
    fprintf(stderr, "%s: short file\n", program);
    exit(2);
  }
}
#endif

} // namespace window_case

#ifdef WINDOW_CASE_STANDALONE
// what the library's host sources call where a stand-alone program has no context
namespace dsm {
static std::string last_error;
void set_error(const std::string &msg) { last_error = msg; }
int invalid(const char *msg) {
  last_error = msg;
  return DSM_ERR_INVALID;
}
} // namespace dsm
#endif
