// finish_host_standalone.cpp -- dsm_window_finish_host as a stand-alone CPU program, for a sanitizer run of the host form (DESIGN.md
// section 22): reads a finish file (tests/_finish_ref.py, write_case: a step file with the finish's inputs behind it), puts every plane
// and every array into a heap block of exactly its size, runs the call once with the required outputs alone and once with every
// optional output, and prints one JSON line with the pattern, the counts and the FNV-1a hashes of the outputs, for a comparison with the
// checker tests/_finish_ref.py (hashes).  Build, from the repository root:
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       tools/finish_host_standalone.cpp direct_stereo_slam_amd/csrc/points_host.cpp direct_stereo_slam_amd/csrc/solve_host.cpp \
//       direct_stereo_slam_amd/csrc/step_host.cpp direct_stereo_slam_amd/csrc/optimize_host.cpp direct_stereo_slam_amd/csrc/finish_host.cpp \
//       -o finish_host_standalone
// Usage: finish_host_standalone FILE [MAX_ITERATIONS = 6] [FORCE_ACCEPT = 0]; tools/finish_host_standalone_check.py BINARY writes the
// cases of the checker's scenes, runs the binary over them and compares the hashes.  The program frees none of its blocks: run it with
// ASAN_OPTIONS=detect_leaks=0.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../include/dsm_hotpath.h"

namespace dsm {
static std::string last_error;
void set_error(const std::string &msg) { last_error = msg; }
} // namespace dsm

template <typename T>
static T *block(size_t n) { // exactly n elements, so that the sanitizer sees every access past an end
  return (T *)malloc(n ? n * sizeof(T) : 1);
}
template <typename T>
static T *read_block(FILE *f, size_t n) {
  T *p = block<T>(n);
  if (n && fread(p, sizeof(T), n, f) != n) {
    fprintf(stderr, "finish_host_standalone: short file\n");
    exit(2);
  }
  return p;
}
static uint64_t fnv(const void *p, size_t n) {
  uint64_t h = 1469598103934665603ull;
  for (size_t i = 0; i < n; i++) h = (h ^ ((const unsigned char *)p)[i]) * 1099511628211ull;
  return h;
}

int main(int argc, char **argv) {
  FILE *f = argc > 1 ? fopen(argv[1], "rb") : nullptr;
  if (!f) {
    fprintf(stderr, "usage: finish_host_standalone FILE\n");
    return 2;
  }
  int *wh = read_block<int>(f, 2);
  read_block<float>(f, 6); // cam, cam_inv: not read by this call
  int *nff = read_block<int>(f, 2);
  const size_t nf = nff[0], npx = (size_t)wh[0] * wh[1], N = 4 + 8 * nf, n2 = nf * nf;
  const int max_its = argc > 2 ? atoi(argv[2]) : 6;
  dsm_finish_job F;
  memset(&F, 0, sizeof F);
  dsm_optimize_job &O = F.opt;
  dsm_step_job &T = O.step;
  dsm_solve_job &S = T.sol;
  dsm_hessian_job &H = S.hes;
  dsm_linearize_job &J = H.lin;
  J.n_frames = (int)nf, J.fix_linearization = nff[1], J.frame_ids = read_block<int>(f, nf);
  const float **planes = block<const float *>(nf);
  for (size_t k = 0; k < nf; k++) planes[k] = read_block<float>(f, npx);
  read_block<float>(f, n2 * 27); // the precalc tables: formed by this call
  J.frame_energy_th = read_block<float>(f, nf);
  const size_t n = *read_block<int>(f, 1);
  float *prec = read_block<float>(f, n * 21);
  const size_t nr = *read_block<int>(f, 1);
  float *rrec = read_block<float>(f, nr * 5);
  int *host = block<int>(n), *point = block<int>(nr), *target = block<int>(nr);
  float *u = block<float>(n), *v = block<float>(n), *color = block<float>(8 * n), *wts = block<float>(8 * n);
  for (size_t i = 0; i < n; i++) {
    const float *q = prec + 21 * i;
    memcpy(host + i, q, 4), u[i] = q[1], v[i] = q[2];
    memcpy(color + 8 * i, q + 5, 32), memcpy(wts + 8 * i, q + 13, 32);
  }
  unsigned char *sin = block<unsigned char>(nr), *isnew = block<unsigned char>(nr);
  float *ein = block<float>(nr);
  for (size_t i = 0; i < nr; i++) {
    const float *q = rrec + 5 * i;
    int s, w;
    memcpy(point + i, q, 4), memcpy(target + i, q + 1, 4), memcpy(&s, q + 2, 4), memcpy(&w, q + 4, 4);
    sin[i] = (unsigned char)s, isnew[i] = (unsigned char)w, ein[i] = q[3];
  }
  J.n_pts = (int)n, J.host = host, J.u = u, J.v = v, J.color = color, J.weights = wts;
  J.n_res = (int)nr, J.point = point, J.target = target, J.state_in = sin, J.energy_in = ein, J.is_new = isnew;
  J.new_state = block<unsigned char>(nr), J.new_energy = block<float>(nr), J.new_energy_with_outlier = block<float>(nr);
  double energy;
  float th;
  J.energy_out = &energy, J.new_frame_energy_th_out = &th;
  H.ad_host = read_block<double>(f, n2 * 64), H.ad_target = read_block<double>(f, n2 * 64);
  float *pin = read_block<float>(f, n * 8);
  float *per[4], *hcd_lin = block<float>(4 * n);
  for (int k = 0; k < 4; k++) {
    per[k] = block<float>(n);
    for (size_t i = 0; i < n; i++) per[k][i] = pin[8 * i + k];
  }
  for (size_t i = 0; i < n; i++) memcpy(hcd_lin + 4 * i, pin + 8 * i + 4, 16);
  H.prior = per[0], H.hdd_lin = per[2], H.bd_lin = per[3], H.hcd_lin = hcd_lin; // per[1], delta: formed by this call
  H.shift_prior_to_zero = *read_block<int>(f, 1);
  S.H_L = read_block<double>(f, N * N), S.b_L = read_block<double>(f, N);
  if (*read_block<int>(f, 1)) S.H_M = read_block<double>(f, N * N), S.b_M = read_block<double>(f, N);
  S.lambda = *read_block<double>(f, 1), S.n_null = *read_block<int>(f, 1);
  S.null_basis = read_block<double>(f, N * S.n_null), S.null_pinv = read_block<double>(f, N * S.n_null);
  T.world_to_cam_eval = read_block<double>(f, 7 * nf), T.state_zero = read_block<double>(f, 8 * nf), T.state_backup = read_block<double>(f, 8 * nf);
  read_block<double>(f, 8 * nf); // frame_step: formed by the loop
  T.calib_zero = read_block<double>(f, 4), T.calib_backup = read_block<double>(f, 4);
  read_block<double>(f, 4), T.idepth_backup = read_block<float>(f, n), read_block<float>(f, n); // calib_step, idepth_step: formed by the loop
  T.exposure = read_block<float>(f, nf);
  memcpy(T.stepfac, read_block<float>(f, 5), 20);
  if (*read_block<int>(f, 1)) T.prior = read_block<double>(f, N), T.prior_zero = read_block<double>(f, N);
  // the finish's inputs, appended to the step file (tests/_finish_ref.py, write_case)
  F.n_good_residuals_in = read_block<int>(f, n), F.max_rel_baseline_in = read_block<float>(f, n), F.last_res = read_block<int>(f, 2 * n);
  F.last_state_in = read_block<unsigned char>(f, 2 * n);
  fclose(f);
  int flags = -1, can_break = -1;
  double energy_m;
  S.x = block<double>(N), S.step = block<float>(n), S.flags = &flags;
  T.state_out = block<double>(8 * nf), T.calib_out = block<double>(4), T.idepth_out = block<float>(n), T.world_to_cam_out = block<double>(7 * nf);
  T.can_break = &can_break, T.step_sums = block<float>(6), T.energy_m = &energy_m;
  const size_t its = (size_t)(max_its > 0 ? max_its : 0), passes = 1 + 2 * its;
  int n_iterations = -1, n_passes = -1;
  double lambda_out;
  float eth_out;
  O.max_iterations = max_its, O.n_iterations = &n_iterations, O.n_passes = &n_passes, O.pattern = block<unsigned char>(its);
  O.pass_energy = block<double>(2 * passes), O.pass_lambda = block<double>(passes), O.iter_stepsize = block<float>(its);
  O.iter_can_break = block<unsigned char>(its), O.last_energy = block<double>(2), O.lambda_out = &lambda_out, O.frame_energy_th_out = &eth_out;
  dsm_linearize_params lp;
  dsm_step_params sp;
  dsm_optimize_params op;
  dsm_linearize_params_default(&lp), dsm_step_params_default(&sp), dsm_optimize_params_default(&op);
  op.force_accept = argc > 3 ? atoi(argv[3]) : 0;
  // the finish's outputs: every array exactly as long as the call may write
  double fin_energy;
  float fin_th, rmse;
  int n_res_out = -1, n_pts_out = -1, lost = -1;
  F.world_to_cam_eval_out = block<double>(7 * nf), F.state_zero_out = block<double>(8 * nf), F.state_out = block<double>(8 * nf);
  F.ad_host_out = block<double>(64 * n2), F.ad_target_out = block<double>(64 * n2), F.ad_ht_delta_out = block<float>(8 * n2);
  F.c_delta_out = block<float>(4), F.delta_x_out = block<double>(N), F.cam_out = block<float>(6);
  F.pre_RTll_0_out = block<float>(9 * n2), F.pre_tTll_0_out = block<float>(3 * n2), F.pre_KRKiTll_out = block<float>(9 * n2);
  F.pre_KtTll_out = block<float>(3 * n2), F.pre_aff_mode_out = block<float>(2 * n2), F.pre_b0_mode_out = block<float>(n2);
  F.new_state = block<unsigned char>(nr), F.new_energy = block<float>(nr), F.new_energy_with_outlier = block<float>(nr);
  F.keep = block<unsigned char>(nr), F.rel_bs = block<float>(nr), F.energy = &fin_energy, F.frame_energy_th_out = &fin_th;
  F.n_good_residuals_out = block<int>(n), F.max_rel_baseline_out = block<float>(n), F.last_res_out = block<int>(2 * n);
  F.last_state_out = block<unsigned char>(2 * n), F.n_res_kept = block<int>(n), F.point_dropped = block<unsigned char>(n);
  F.res_index_out = block<int>(nr), F.point_index_out = block<int>(n), F.n_res_out = &n_res_out, F.n_pts_out = &n_pts_out;
  F.rmse = &rmse, F.lost = &lost;
  // the required outputs alone
  int rc = dsm_window_finish_host(wh[0], wh[1], &F, planes, &lp, &sp, &op);
  const uint64_t x_lean = fnv(S.x, 8 * N), keep_lean = fnv(F.keep, nr), dp_lean = fnv(F.ad_ht_delta_out, 32 * n2);
  // every optional output, the loop's and the finish's
  T.cam_to_world_out = block<double>(7 * nf), T.cam_out = block<float>(6);
  T.pre_RTll_0_out = block<float>(9 * n2), T.pre_tTll_0_out = block<float>(3 * n2), T.pre_KRKiTll_out = block<float>(9 * n2);
  T.pre_KtTll_out = block<float>(3 * n2), T.pre_aff_mode_out = block<float>(2 * n2), T.pre_b0_mode_out = block<float>(n2);
  T.delta_x_out = block<double>(N), T.H_L_out = block<double>(N * N), T.b_L_out = block<double>(N);
  J.J_out = block<float>((size_t)DSM_LINEARIZE_J_FLOATS * nr);
  J.center_projected_to = block<float>(3 * nr), J.projected_to = block<float>(16 * nr);
  H.H_A = block<double>(N * N), H.b_A = block<double>(N), H.H_sc = block<double>(N * N), H.b_sc = block<double>(N);
  H.active = block<unsigned char>(nr), H.JpJdF = block<float>(8 * nr);
  H.hdd_acc = block<float>(n), H.bd_acc = block<float>(n), H.hcd_acc = block<float>(4 * n), H.hdi = block<float>(n), H.bd_sum = block<float>(n);
  H.idepth_hessian = block<float>(n);
  F.cam_to_world_out = block<double>(7 * nf), F.J_out = block<float>((size_t)DSM_LINEARIZE_J_FLOATS * nr);
  if (!rc) rc = dsm_window_finish_host(wh[0], wh[1], &F, planes, &lp, &sp, &op);
  if (rc) {
    fprintf(stderr, "finish_host_standalone: %d %s\n", rc, dsm::last_error.c_str());
    return 1;
  }
  const bool same = x_lean == fnv(S.x, 8 * N) && keep_lean == fnv(F.keep, nr) && dp_lean == fnv(F.ad_ht_delta_out, 32 * n2);
  auto hx = [](uint64_t h) { return (unsigned long long)h; };
  const std::string pattern((const char *)O.pattern, (size_t)n_iterations);
  printf("{\"n_res\": %zu, \"pattern\": \"%s\", \"passes\": %d, \"n_res_out\": %d, \"n_pts_out\": %d, \"lost\": %d, \"x\": \"%016llx\", "
         "\"eval\": \"%016llx\", \"state\": \"%016llx\", \"ad_host\": \"%016llx\", \"ad_target\": \"%016llx\", \"ad_ht_delta\": \"%016llx\", "
         "\"delta_x\": \"%016llx\", \"tables\": \"%016llx\", \"new_state\": \"%016llx\", \"new_energy\": \"%016llx\", \"keep\": \"%016llx\", "
         "\"rel_bs\": \"%016llx\", \"energy\": \"%016llx\", \"n_good\": \"%016llx\", \"max_rel_baseline\": \"%016llx\", \"last_res\": \"%016llx\", "
         "\"last_state\": \"%016llx\", \"res_index\": \"%016llx\", \"point_index\": \"%016llx\", \"cam_to_world\": \"%016llx\", \"lean_equal\": %d}\n",
         nr, pattern.c_str(), n_passes, n_res_out, n_pts_out, lost, hx(fnv(S.x, 8 * N)), hx(fnv(F.world_to_cam_eval_out, 56 * nf)), hx(fnv(F.state_out, 64 * nf)),
         hx(fnv(F.ad_host_out, 512 * n2)), hx(fnv(F.ad_target_out, 512 * n2)), hx(fnv(F.ad_ht_delta_out, 32 * n2)), hx(fnv(F.delta_x_out, 8 * N)),
         hx(fnv(F.pre_RTll_0_out, 36 * n2) ^ fnv(F.pre_tTll_0_out, 12 * n2) ^ fnv(F.pre_KRKiTll_out, 36 * n2) ^ fnv(F.pre_KtTll_out, 12 * n2) ^
            fnv(F.pre_aff_mode_out, 8 * n2) ^ fnv(F.pre_b0_mode_out, 4 * n2)),
         hx(fnv(F.new_state, nr)), hx(fnv(F.new_energy, 4 * nr)), hx(fnv(F.keep, nr)), hx(fnv(F.rel_bs, 4 * nr)), hx(fnv(&fin_energy, 8)),
         hx(fnv(F.n_good_residuals_out, 4 * n)), hx(fnv(F.max_rel_baseline_out, 4 * n)), hx(fnv(F.last_res_out, 8 * n)), hx(fnv(F.last_state_out, 2 * n)),
         hx(fnv(F.res_index_out, 4 * nr)), hx(fnv(F.point_index_out, 4 * n)), hx(fnv(F.cam_to_world_out, 56 * nf)), (int)same);
  return same ? 0 : 1;
}
