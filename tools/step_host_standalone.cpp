// step_host_standalone.cpp -- dsm_window_step_host as a stand-alone CPU program, for a sanitizer run of the host form (DESIGN.md
// section 19): reads a step file (tests/_step_ref.py, write_case: the window file of host/solve_demo.cpp without what the call forms,
// then the step's inputs), puts every plane and every array into a heap block of exactly its size, runs the job once with every
// optional output and once with none, and prints one JSON line with the FNV-1a hashes of the outputs, which tests/_step_ref.py's
// hashes() reproduces from the checker.  Build, from the repository root:
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       tools/step_host_standalone.cpp direct_stereo_slam_amd/csrc/points_host.cpp direct_stereo_slam_amd/csrc/solve_host.cpp \
//       direct_stereo_slam_amd/csrc/step_host.cpp -o step_host_standalone
// The program frees none of its blocks: run it with ASAN_OPTIONS=detect_leaks=0.
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
    fprintf(stderr, "step_host_standalone: short file\n");
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
    fprintf(stderr, "usage: step_host_standalone FILE\n");
    return 2;
  }
  int *wh = read_block<int>(f, 2);
  read_block<float>(f, 6); // cam, cam_inv: not read by this call
  int *nff = read_block<int>(f, 2);
  const size_t nf = nff[0], npx = (size_t)wh[0] * wh[1], N = 4 + 8 * nf, n2 = nf * nf;
  dsm_step_job T;
  memset(&T, 0, sizeof T);
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
  T.frame_step = read_block<double>(f, 8 * nf), T.calib_zero = read_block<double>(f, 4), T.calib_backup = read_block<double>(f, 4);
  T.calib_step = read_block<double>(f, 4), T.idepth_backup = read_block<float>(f, n), T.idepth_step = read_block<float>(f, n);
  T.exposure = read_block<float>(f, nf);
  memcpy(T.stepfac, read_block<float>(f, 5), 20);
  if (*read_block<int>(f, 1)) T.prior = read_block<double>(f, N), T.prior_zero = read_block<double>(f, N);
  fclose(f);
  int flags = -1, can_break = -1;
  double energy_m;
  S.x = block<double>(N), S.step = block<float>(n), S.flags = &flags;
  T.state_out = block<double>(8 * nf), T.calib_out = block<double>(4), T.idepth_out = block<float>(n), T.world_to_cam_out = block<double>(7 * nf);
  T.can_break = &can_break, T.step_sums = block<float>(6), T.energy_m = &energy_m;
  dsm_linearize_params lp;
  dsm_step_params sp;
  dsm_linearize_params_default(&lp), dsm_step_params_default(&sp);
  // the required outputs alone: the host form keeps everything else in room of its own
  int rc = dsm_window_step_host(wh[0], wh[1], &T, planes, &lp, &sp);
  const uint64_t x_lean = fnv(S.x, 8 * N), state_lean = fnv(T.state_out, 64 * nf);
  // every optional output
  T.cam_to_world_out = block<double>(7 * nf), T.cam_out = block<float>(6);
  T.pre_RTll_0_out = block<float>(9 * n2), T.pre_tTll_0_out = block<float>(3 * n2), T.pre_KRKiTll_out = block<float>(9 * n2);
  T.pre_KtTll_out = block<float>(3 * n2), T.pre_aff_mode_out = block<float>(2 * n2), T.pre_b0_mode_out = block<float>(n2);
  T.delta_x_out = block<double>(N), T.H_L_out = block<double>(N * N), T.b_L_out = block<double>(N);
  J.center_projected_to = block<float>(3 * nr), J.projected_to = block<float>(16 * nr), J.keep = block<unsigned char>(nr), J.rel_bs = block<float>(nr);
  H.H_A = block<double>(N * N), H.b_A = block<double>(N), H.H_sc = block<double>(N * N), H.b_sc = block<double>(N);
  H.acc_top = block<double>(n2 * 169), H.acc_D = block<double>(n2 * nf * 64), H.acc_E = block<double>(n2 * 32), H.acc_EB = block<double>(n2 * 8);
  H.acc_Hcc = block<double>(16), H.acc_bc = block<double>(4);
  H.active = block<unsigned char>(nr), H.JpJdF = block<float>(8 * nr);
  H.hdd_acc = block<float>(n), H.bd_acc = block<float>(n), H.hcd_acc = block<float>(4 * n), H.hdi = block<float>(n), H.bd_sum = block<float>(n);
  H.idepth_hessian = block<float>(n);
  S.last_HS = block<double>(N * N), S.last_bS = block<double>(N);
  if (!rc) rc = dsm_window_step_host(wh[0], wh[1], &T, planes, &lp, &sp);
  if (rc) {
    fprintf(stderr, "step_host_standalone: %d %s\n", rc, dsm::last_error.c_str());
    return 1;
  }
  const bool same = x_lean == fnv(S.x, 8 * N) && state_lean == fnv(T.state_out, 64 * nf);
  uint64_t pre = fnv(T.pre_RTll_0_out, 36 * n2) ^ fnv(T.pre_tTll_0_out, 12 * n2) ^ fnv(T.pre_KRKiTll_out, 36 * n2) ^ fnv(T.pre_KtTll_out, 12 * n2) ^
                 fnv(T.pre_aff_mode_out, 8 * n2) ^ fnv(T.pre_b0_mode_out, 4 * n2);
  auto hx = [](uint64_t h) { return (unsigned long long)h; };
  printf("{\"n_res\": %zu, \"state\": \"%016llx\", \"calib\": \"%016llx\", \"idepth\": \"%016llx\", \"world_to_cam\": \"%016llx\", "
         "\"cam_to_world\": \"%016llx\", \"cam\": \"%016llx\", \"pre\": \"%016llx\", \"delta_x\": \"%016llx\", \"H_L\": \"%016llx\", \"b_L\": \"%016llx\", "
         "\"energy_m\": \"%016llx\", \"x\": \"%016llx\", \"step\": \"%016llx\", \"new_energy\": \"%016llx\", \"can_break\": %d, \"flags\": %d, "
         "\"lean_equal\": %d}\n",
         nr, hx(fnv(T.state_out, 64 * nf)), hx(fnv(T.calib_out, 32)), hx(fnv(T.idepth_out, 4 * n)), hx(fnv(T.world_to_cam_out, 56 * nf)),
         hx(fnv(T.cam_to_world_out, 56 * nf)), hx(fnv(T.cam_out, 24)), hx(pre), hx(fnv(T.delta_x_out, 8 * N)), hx(fnv(T.H_L_out, 8 * N * N)),
         hx(fnv(T.b_L_out, 8 * N)), hx(fnv(&energy_m, 8)), hx(fnv(S.x, 8 * N)), hx(fnv(S.step, 4 * n)), hx(fnv(J.new_energy, 4 * nr)), can_break, flags,
         (int)same);
  return same ? 0 : 1;
}
