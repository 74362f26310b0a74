// solve_host_standalone.cpp -- dsm_window_solve_host as a stand-alone CPU program, for a sanitizer run of the host form (DESIGN.md
// section 18): reads a window file in the format of host/solve_demo.cpp, puts every plane and every array into a heap block of exactly
// its size, runs the job once with every optional output and once with none, and prints one JSON line with the FNV-1a hashes of x,
// the steps, last_HS and last_bS, which tests/test_solve_demo.py's fnv1a reproduces from the checker.  Build, from the repository root:
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       tools/solve_host_standalone.cpp direct_stereo_slam_amd/csrc/points_host.cpp direct_stereo_slam_amd/csrc/solve_host.cpp \
//       -o solve_host_standalone
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
    fprintf(stderr, "solve_host_standalone: short file\n");
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
    fprintf(stderr, "usage: solve_host_standalone FILE\n");
    return 2;
  }
  int *wh = read_block<int>(f, 2);
  float *cal = read_block<float>(f, 6);
  int *nff = read_block<int>(f, 2);
  const size_t nf = nff[0], npx = (size_t)wh[0] * wh[1], N = 4 + 8 * nf;
  dsm_solve_job S;
  memset(&S, 0, sizeof S);
  dsm_hessian_job &H = S.hes;
  dsm_linearize_job &J = H.lin;
  memcpy(J.cam, cal, 16), memcpy(J.cam_inv, cal + 4, 8);
  J.n_frames = (int)nf, J.fix_linearization = nff[1], J.frame_ids = read_block<int>(f, nf);
  const float **planes = block<const float *>(nf);
  for (size_t k = 0; k < nf; k++) planes[k] = read_block<float>(f, npx);
  float *pre = read_block<float>(f, nf * nf * 27);
  float *tab[6];
  const int width[6] = {9, 3, 9, 3, 2, 1};
  for (int k = 0, at = 0; k < 6; at += width[k], k++) {
    tab[k] = block<float>(nf * nf * width[k]);
    for (size_t p = 0; p < nf * nf; p++) memcpy(tab[k] + p * width[k], pre + p * 27 + at, 4 * width[k]);
  }
  J.pre_RTll_0 = tab[0], J.pre_tTll_0 = tab[1], J.pre_KRKiTll = tab[2], J.pre_KtTll = tab[3], J.pre_aff_mode = tab[4], J.pre_b0_mode = tab[5];
  J.frame_energy_th = read_block<float>(f, nf);
  const size_t n = *read_block<int>(f, 1);
  float *prec = read_block<float>(f, n * 21);
  const size_t nr = *read_block<int>(f, 1);
  float *rrec = read_block<float>(f, nr * 5);
  int *host = block<int>(n), *point = block<int>(nr), *target = block<int>(nr);
  float *u = block<float>(n), *v = block<float>(n), *id = block<float>(n), *idz = block<float>(n), *color = block<float>(8 * n), *wts = block<float>(8 * n);
  for (size_t i = 0; i < n; i++) {
    const float *q = prec + 21 * i;
    memcpy(host + i, q, 4), u[i] = q[1], v[i] = q[2], id[i] = q[3], idz[i] = q[4];
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
  J.n_pts = (int)n, J.host = host, J.u = u, J.v = v, J.idepth_scaled = id, J.idepth_zero_scaled = idz, J.color = color, J.weights = wts;
  J.n_res = (int)nr, J.point = point, J.target = target, J.state_in = sin, J.energy_in = ein, J.is_new = isnew;
  J.new_state = block<unsigned char>(nr), J.new_energy = block<float>(nr), J.new_energy_with_outlier = block<float>(nr);
  double energy;
  float th;
  J.energy_out = &energy, J.new_frame_energy_th_out = &th;
  H.ad_host = read_block<double>(f, nf * nf * 64), H.ad_target = read_block<double>(f, nf * nf * 64);
  float *pin = read_block<float>(f, n * 8);
  float *per[4], *hcd_lin = block<float>(4 * n);
  for (int k = 0; k < 4; k++) {
    per[k] = block<float>(n);
    for (size_t i = 0; i < n; i++) per[k][i] = pin[8 * i + k];
  }
  for (size_t i = 0; i < n; i++) memcpy(hcd_lin + 4 * i, pin + 8 * i + 4, 16);
  H.prior = per[0], H.delta = per[1], H.hdd_lin = per[2], H.bd_lin = per[3], H.hcd_lin = hcd_lin;
  H.shift_prior_to_zero = *read_block<int>(f, 1);
  S.H_L = read_block<double>(f, N * N), S.b_L = read_block<double>(f, N), S.H_M = read_block<double>(f, N * N), S.b_M = read_block<double>(f, N);
  S.delta_x = read_block<double>(f, N), S.lambda = *read_block<double>(f, 1), S.n_null = *read_block<int>(f, 1);
  S.null_basis = read_block<double>(f, N * S.n_null), S.null_pinv = read_block<double>(f, N * S.n_null);
  fclose(f);
  int flags = -1;
  S.x = block<double>(N), S.step = block<float>(n), S.flags = &flags;
  dsm_linearize_params params;
  dsm_linearize_params_default(&params);
  // the required outputs alone: the host form keeps everything else in room of its own
  int rc = dsm_window_solve_host(wh[0], wh[1], &S, planes, &params);
  const uint64_t x_lean = fnv(S.x, 8 * N), step_lean = fnv(S.step, 4 * n);
  // every optional output
  const size_t n2 = nf * nf;
  J.center_projected_to = block<float>(3 * nr), J.projected_to = block<float>(16 * nr), J.keep = block<unsigned char>(nr), J.rel_bs = block<float>(nr);
  H.H_A = block<double>(N * N), H.b_A = block<double>(N), H.H_sc = block<double>(N * N), H.b_sc = block<double>(N);
  H.acc_top = block<double>(n2 * 169), H.acc_D = block<double>(n2 * nf * 64), H.acc_E = block<double>(n2 * 32), H.acc_EB = block<double>(n2 * 8);
  H.acc_Hcc = block<double>(16), H.acc_bc = block<double>(4);
  H.active = block<unsigned char>(nr), H.JpJdF = block<float>(8 * nr);
  H.hdd_acc = block<float>(n), H.bd_acc = block<float>(n), H.hcd_acc = block<float>(4 * n), H.hdi = block<float>(n), H.bd_sum = block<float>(n);
  H.idepth_hessian = block<float>(n);
  S.last_HS = block<double>(N * N), S.last_bS = block<double>(N);
  if (!rc) rc = dsm_window_solve_host(wh[0], wh[1], &S, planes, &params);
  if (rc) {
    fprintf(stderr, "solve_host_standalone: %d %s\n", rc, dsm::last_error.c_str());
    return 1;
  }
  const bool same = x_lean == fnv(S.x, 8 * N) && step_lean == fnv(S.step, 4 * n);
  printf("{\"n_res\": %zu, \"x\": \"%016llx\", \"step\": \"%016llx\", \"last_HS\": \"%016llx\", \"last_bS\": \"%016llx\", \"flags\": %d, "
         "\"lean_equal\": %d}\n",
         nr, (unsigned long long)fnv(S.x, 8 * N), (unsigned long long)fnv(S.step, 4 * n), (unsigned long long)fnv(S.last_HS, 8 * N * N),
         (unsigned long long)fnv(S.last_bS, 8 * N), flags, (int)same);
  return same ? 0 : 1;
}
