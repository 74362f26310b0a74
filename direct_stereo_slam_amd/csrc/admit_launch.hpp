// admit_launch.hpp -- what the two forms of the admission call (admit_kernels.hip, admit_host.cpp) share on the host: the rules V of
// DESIGN.md section 26, the launch geometry, and the device form's layout: where every array of a job stands in the staged block and in
// the read-back block of the call arena (call_arena.hpp), the copies in and the copies out.
#pragma once
#include <algorithm>

#include "dsm_internal.hpp"
// after the runtime's header: the math headers' qualifiers are its
#include "admit_math.hpp"

namespace dsm {

constexpr int kAdmBlock = 256;    // adm_kernel's workgroup
constexpr int kAdmListBlocks = 8; // at most this many workgroups stride over a job's residuals, points and grown matrices

const char *admit_job_error(const dsm_admit_job &J);
// V for the whole call (ctx apart); LP, SP, AP: the caller's parameters, or the defaults for NULL
int admit_check(const char *call, int n_jobs, const dsm_admit_job *jobs, const dsm_linearize_params *lp, const dsm_step_params *sp,
                const dsm_admit_params *ap, dsm_linearize_params &LP, dsm_step_params &SP, adm::Params &AP);

// One job in the arena: offsets in entries of their type into the staged doubles / floats / ints / bytes (q_, f_, i_, b_) and into
// the read-back ones (oq_, of_, oi_, ob_); -1: the optional array is absent
struct AdmJob {
  int n, n_pts, n_res, new_id;
  float new_exposure, new_eth;
  int q_eval, q_state, q_zero, q_ref, q_ctr, q_aff, q_prior_f, q_prior_f0, q_cval, q_czero, q_HM, q_bM, q_HL, q_bL, q_prior, q_prior0;
  int f_exp, f_eth, f_energy;
  int i_id, i_in, i_out, i_last, i_point, i_target;
  int b_last, b_state, b_new;
  int oq_eval, oq_state, oq_zero, oq_W, oq_c2w, oq_dx, oq_adh, oq_adt, oq_HM, oq_bM, oq_HL, oq_bL, oq_prior, oq_prior0, oq_fprior, oq_fdelta, oq_score;
  int of_pre, of_adht, of_dist, of_cam, of_cd, of_exp, of_eth, of_energy;
  int oi_id, oi_point, oi_target, oi_res, oi_new, oi_last, oi_words; // words: n_res_out, n_flagged
  int ob_flagged, ob_state, ob_new, ob_last;
};

struct AdmTotals {
  size_t q = 0, f = 0, i = 0, b = 0, oq = 0, of = 0, oi = 0, ob = 0;
  int max_list = 0; // the longest strided loop of any job
  bool fits() const {
    const size_t lim = 0x7fffffffu;
    return q <= lim && f <= lim && i <= lim && b <= lim && oq <= lim && of <= lim && oi <= lim && ob <= lim;
  }
};

inline void admit_layout(const dsm_admit_job &G, AdmJob &K, AdmTotals &T) {
  const size_t n = G.n_frames, m = n + 1, m2 = m * m, N = 4 + 8 * n, M = N + 8, np = G.n_pts, nr = G.n_res, no = np + nr;
  auto take = [](size_t &at, size_t k) { return at += k, (int)(at - k); };
  K.n = G.n_frames, K.n_pts = G.n_pts, K.n_res = G.n_res, K.new_id = G.new_keyframe_id, K.new_exposure = G.new_exposure, K.new_eth = G.new_frame_energy_th;
  K.q_eval = take(T.q, 7 * n), K.q_state = take(T.q, 8 * n), K.q_zero = take(T.q, 8 * n), K.q_ref = take(T.q, 7), K.q_ctr = take(T.q, 7);
  K.q_aff = take(T.q, 2), K.q_prior_f = take(T.q, 8), K.q_prior_f0 = take(T.q, 8), K.q_cval = take(T.q, 4), K.q_czero = take(T.q, 4);
  K.q_HM = G.H_M ? take(T.q, N * N) : -1, K.q_bM = G.b_M ? take(T.q, N) : -1, K.q_HL = G.H_L ? take(T.q, N * N) : -1, K.q_bL = G.b_L ? take(T.q, N) : -1;
  K.q_prior = G.prior ? take(T.q, N) : -1, K.q_prior0 = G.prior ? take(T.q, N) : -1;
  K.f_exp = take(T.f, n), K.f_eth = take(T.f, n), K.f_energy = take(T.f, nr);
  K.i_id = take(T.i, n), K.i_in = take(T.i, n), K.i_out = take(T.i, n), K.i_last = take(T.i, 2 * np), K.i_point = take(T.i, nr), K.i_target = take(T.i, nr);
  K.b_last = take(T.b, 2 * np), K.b_state = take(T.b, nr), K.b_new = take(T.b, nr);
  K.oq_eval = take(T.oq, 7 * m), K.oq_state = take(T.oq, 8 * m), K.oq_zero = take(T.oq, 8 * m), K.oq_W = take(T.oq, 7 * m), K.oq_c2w = take(T.oq, 7);
  K.oq_dx = take(T.oq, M), K.oq_adh = take(T.oq, 64 * m2), K.oq_adt = take(T.oq, 64 * m2);
  K.oq_HM = G.H_M ? take(T.oq, M * M) : -1, K.oq_bM = G.b_M ? take(T.oq, M) : -1, K.oq_HL = G.H_L ? take(T.oq, M * M) : -1, K.oq_bL = G.b_L ? take(T.oq, M) : -1;
  K.oq_prior = G.prior ? take(T.oq, M) : -1, K.oq_prior0 = G.prior ? take(T.oq, M) : -1;
  K.oq_fprior = take(T.oq, 8), K.oq_fdelta = take(T.oq, 8), K.oq_score = take(T.oq, n);
  K.of_pre = take(T.of, 27 * m2), K.of_adht = take(T.of, 8 * m2), K.of_dist = take(T.of, m2), K.of_cam = take(T.of, 6), K.of_cd = take(T.of, 4);
  K.of_exp = take(T.of, m), K.of_eth = take(T.of, m), K.of_energy = take(T.of, no);
  K.oi_id = take(T.oi, m), K.oi_point = take(T.oi, no), K.oi_target = take(T.oi, no), K.oi_res = take(T.oi, nr), K.oi_new = take(T.oi, np);
  K.oi_last = take(T.oi, 2 * np), K.oi_words = take(T.oi, 2);
  K.ob_flagged = take(T.ob, m), K.ob_state = take(T.ob, no), K.ob_new = take(T.ob, no), K.ob_last = take(T.ob, 2 * np);
  const size_t longest = std::max(std::max(np, nr), (G.H_M || G.H_L) ? M * M : M);
  T.max_list = std::max(T.max_list, (int)longest);
}

// the copies in: hq, hf, hi, hb the staged blocks on the host
inline void admit_stage(const dsm_admit_job &G, const AdmJob &K, double *hq, float *hf, int *hi, unsigned char *hb) {
  const size_t n = K.n, N = 4 + 8 * n, np = K.n_pts, nr = K.n_res;
  auto put = [](void *to, const void *from, size_t bytes) {
    if (bytes) memcpy(to, from, bytes);
  };
  put(hq + K.q_eval, G.world_to_cam_eval, 56 * n), put(hq + K.q_state, G.state, 64 * n), put(hq + K.q_zero, G.state_zero, 64 * n);
  put(hq + K.q_ref, G.ref_cam_to_world, 56), put(hq + K.q_ctr, G.cam_to_tracking_ref, 56), put(hq + K.q_aff, G.aff_g2l, 16);
  put(hq + K.q_prior_f, G.new_frame_prior, 64), put(hq + K.q_prior_f0, G.new_frame_prior_zero, 64);
  put(hq + K.q_cval, G.calib_value, 32), put(hq + K.q_czero, G.calib_zero, 32);
  if (G.H_M) put(hq + K.q_HM, G.H_M, 8 * N * N);
  if (G.b_M) put(hq + K.q_bM, G.b_M, 8 * N);
  if (G.H_L) put(hq + K.q_HL, G.H_L, 8 * N * N);
  if (G.b_L) put(hq + K.q_bL, G.b_L, 8 * N);
  if (G.prior) put(hq + K.q_prior, G.prior, 8 * N), put(hq + K.q_prior0, G.prior_zero, 8 * N);
  put(hf + K.f_exp, G.exposure, 4 * n), put(hf + K.f_eth, G.frame_energy_th, 4 * n), put(hf + K.f_energy, G.energy_in, 4 * nr);
  put(hi + K.i_id, G.keyframe_id, 4 * n), put(hi + K.i_in, G.n_points_in, 4 * n), put(hi + K.i_out, G.n_points_out, 4 * n);
  put(hi + K.i_last, G.last_res, 8 * np), put(hi + K.i_point, G.point, 4 * nr), put(hi + K.i_target, G.target, 4 * nr);
  put(hb + K.b_last, G.last_state, 2 * np), put(hb + K.b_state, G.state_in, nr), put(hb + K.b_new, G.is_new, nr);
}

// the copies out: oq, of, oi, ob the read-back blocks on the host
inline void admit_unstage(const dsm_admit_job &G, const AdmJob &K, const double *oq, const float *of, const int *oi, const unsigned char *ob) {
  const size_t n = K.n, m = n + 1, m2 = m * m, M = 12 + 8 * n, np = K.n_pts, nr = K.n_res, no = np + nr;
  auto get = [](void *to, const void *from, size_t bytes) {
    if (bytes) memcpy(to, from, bytes);
  };
  get(G.world_to_cam_eval_out, oq + K.oq_eval, 56 * m), get(G.state_out, oq + K.oq_state, 64 * m), get(G.state_zero_out, oq + K.oq_zero, 64 * m);
  get(G.world_to_cam_out, oq + K.oq_W, 56 * m), get(G.cam_to_world_out, oq + K.oq_c2w, 56), get(G.delta_x_out, oq + K.oq_dx, 8 * M);
  get(G.ad_host_out, oq + K.oq_adh, 512 * m2), get(G.ad_target_out, oq + K.oq_adt, 512 * m2);
  if (G.H_M) get(G.H_M_out, oq + K.oq_HM, 8 * M * M);
  if (G.b_M) get(G.b_M_out, oq + K.oq_bM, 8 * M);
  if (G.H_L) get(G.H_L_out, oq + K.oq_HL, 8 * M * M);
  if (G.b_L) get(G.b_L_out, oq + K.oq_bL, 8 * M);
  if (G.prior) get(G.prior_out, oq + K.oq_prior, 8 * M), get(G.prior_zero_out, oq + K.oq_prior0, 8 * M);
  get(G.frame_prior_out, oq + K.oq_fprior, 64), get(G.frame_delta_prior_out, oq + K.oq_fdelta, 64), get(G.dist_score_out, oq + K.oq_score, 8 * n);
  const float *q = of + K.of_pre;
  get(G.pre_RTll_0_out, q, 36 * m2), get(G.pre_tTll_0_out, q + 9 * m2, 12 * m2), get(G.pre_KRKiTll_out, q + 12 * m2, 36 * m2);
  get(G.pre_KtTll_out, q + 21 * m2, 12 * m2), get(G.pre_aff_mode_out, q + 24 * m2, 8 * m2), get(G.pre_b0_mode_out, q + 26 * m2, 4 * m2);
  get(G.ad_ht_delta_out, of + K.of_adht, 32 * m2);
  if (G.distance_ll_out) get(G.distance_ll_out, of + K.of_dist, 4 * m2);
  get(G.cam_out, of + K.of_cam, 24), get(G.c_delta_out, of + K.of_cd, 16), get(G.exposure_out, of + K.of_exp, 4 * m);
  get(G.frame_energy_th_out, of + K.of_eth, 4 * m), get(G.energy_out, of + K.of_energy, 4 * no);
  get(G.keyframe_id_out, oi + K.oi_id, 4 * m), get(G.point_out, oi + K.oi_point, 4 * no), get(G.target_out, oi + K.oi_target, 4 * no);
  get(G.res_index_out, oi + K.oi_res, 4 * nr), get(G.new_res_index_out, oi + K.oi_new, 4 * np), get(G.last_res_out, oi + K.oi_last, 8 * np);
  *G.n_res_out = oi[K.oi_words], *G.n_flagged = oi[K.oi_words + 1];
  get(G.flagged_out, ob + K.ob_flagged, m), get(G.res_state_out, ob + K.ob_state, no), get(G.is_new_out, ob + K.ob_new, no);
  get(G.last_state_out, ob + K.ob_last, 2 * np);
}

} // namespace dsm
