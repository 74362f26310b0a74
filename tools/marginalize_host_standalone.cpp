// marginalize_host_standalone.cpp -- dsm_window_marginalize_host as a stand-alone CPU program, for a sanitizer run of the host form
// (DESIGN.md section 21): reads a window file in the format of tests/_marginalize_ref.py's write_case, puts every plane and every
// array into a heap block of exactly its size, runs the job once with the required outputs alone and once with every optional
// output, and prints one JSON line with the FNV-1a hashes of the outputs, which tests/_marginalize_ref.py's hashes reproduces from
// the checker (every output block starts filled as the ctypes mirror fills it, so that what Z leaves alone hashes alike).
// Build, from the repository root:
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       tools/marginalize_host_standalone.cpp direct_stereo_slam_amd/csrc/points_host.cpp direct_stereo_slam_amd/csrc/marginalize_host.cpp \
//       -o marginalize_host_standalone
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
static T *filled(size_t n, T value) {
  T *p = block<T>(n);
  for (size_t i = 0; i < n; i++) p[i] = value;
  return p;
}
template <typename T>
static T *read_block(FILE *f, size_t n) {
  T *p = block<T>(n);
  if (n && fread(p, sizeof(T), n, f) != n) {
    fprintf(stderr, "marginalize_host_standalone: short file\n");
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
    fprintf(stderr, "usage: marginalize_host_standalone FILE\n");
    return 2;
  }
  int *wh = read_block<int>(f, 2);
  float *cal = read_block<float>(f, 6);
  int *nff = read_block<int>(f, 2);
  const size_t nf = nff[0], npx = (size_t)wh[0] * wh[1], N = 4 + 8 * nf;
  dsm_marginalize_job M;
  memset(&M, 0, sizeof M);
  dsm_hessian_job &H = M.hes;
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
  H.ad_host = read_block<double>(f, nf * nf * 64), H.ad_target = read_block<double>(f, nf * nf * 64);
  float *pin = read_block<float>(f, n * 2);
  float *prior = block<float>(n), *delta = block<float>(n);
  for (size_t i = 0; i < n; i++) prior[i] = pin[2 * i], delta[i] = pin[2 * i + 1];
  H.prior = prior, H.delta = delta;
  M.flagged = read_block<unsigned char>(f, nf), M.n_good_residuals = read_block<int>(f, n), M.last_state = read_block<unsigned char>(f, 2 * n);
  M.idepth_hessian = read_block<float>(f, n), M.ad_ht_delta = read_block<float>(f, nf * nf * 8), M.c_delta = read_block<float>(f, 4);
  if (*read_block<int>(f, 1)) M.H_M = read_block<double>(f, N * N), M.b_M = read_block<double>(f, N);
  const size_t nm = *read_block<int>(f, 1), Nn = N - 8 * nm;
  M.n_marg_frames = (int)nm, M.marg_frames = read_block<int>(f, nm);
  M.frame_prior = read_block<double>(f, 8 * nm), M.frame_delta_prior = read_block<double>(f, 8 * nm);
  fclose(f);
  dsm_linearize_params lp;
  dsm_marginalize_params mp;
  dsm_linearize_params_default(&lp), dsm_marginalize_params_default(&mp);
  double energy;
  float th;
  int n_res_marg = -7;
  auto required = [&]() { // fresh blocks, filled as the mirror fills them
    J.new_state = filled<unsigned char>(nr, 77), J.new_energy = filled<float>(nr, -7.f), J.new_energy_with_outlier = filled<float>(nr, -7.f);
    J.energy_out = &energy, J.new_frame_energy_th_out = &th;
    M.verdict = filled<unsigned char>(n, 77), M.H_M_out = filled<double>(Nn * Nn, -7.0), M.b_M_out = filled<double>(Nn, -7.0), M.n_res_marg = &n_res_marg;
  };
  auto core = [&]() { return fnv(M.verdict, n) ^ fnv(M.H_M_out, 8 * Nn * Nn) ^ fnv(M.b_M_out, 8 * Nn) ^ fnv(J.new_energy, 4 * nr) ^ fnv(&n_res_marg, 4); };
  required(); // the required outputs alone: the host form keeps everything else in room of its own
  int rc = dsm_window_marginalize_host(wh[0], wh[1], &M, planes, &lp, &mp);
  const uint64_t lean = core();
  required(); // every optional output
  const size_t n2 = nf * nf;
  J.center_projected_to = filled<float>(3 * nr, -7.f), J.projected_to = filled<float>(16 * nr, -7.f);
  H.H_A = filled<double>(N * N, -7.0), H.b_A = filled<double>(N, -7.0), H.H_sc = filled<double>(N * N, -7.0), H.b_sc = filled<double>(N, -7.0);
  H.acc_top = filled<double>(n2 * 169, -7.0), H.acc_D = filled<double>(n2 * nf * 64, -7.0), H.acc_E = filled<double>(n2 * 32, -7.0);
  H.acc_EB = filled<double>(n2 * 8, -7.0), H.acc_Hcc = filled<double>(16, -7.0), H.acc_bc = filled<double>(4, -7.0);
  H.active = filled<unsigned char>(nr, 77), H.JpJdF = filled<float>(8 * nr, -7.f);
  H.hdd_acc = filled<float>(n, -7.f), H.bd_acc = filled<float>(n, -7.f), H.hcd_acc = filled<float>(4 * n, -7.f), H.hdi = filled<float>(n, -7.f);
  H.bd_sum = filled<float>(n, -7.f), H.idepth_hessian = filled<float>(n, -7.f);
  M.H_M_points = filled<double>(N * N, -7.0), M.b_M_points = filled<double>(N, -7.0), M.res_to_zero = filled<float>(8 * nr, -7.f);
  if (!rc) rc = dsm_window_marginalize_host(wh[0], wh[1], &M, planes, &lp, &mp);
  if (rc) {
    fprintf(stderr, "marginalize_host_standalone: %d %s\n", rc, dsm::last_error.c_str());
    return 1;
  }
  const bool same = lean == core();
  auto hx = [](const void *p, size_t bytes) { return (unsigned long long)fnv(p, bytes); };
  printf("{\"n_res\": %zu, \"n_res_marg\": %d, \"verdict\": \"%016llx\", \"H_M_out\": \"%016llx\", \"b_M_out\": \"%016llx\", \"H_M_points\": \"%016llx\", "
         "\"b_M_points\": \"%016llx\", \"res_to_zero\": \"%016llx\", \"new_state\": \"%016llx\", \"new_energy\": \"%016llx\", "
         "\"new_energy_with_outlier\": \"%016llx\", \"center_projected_to\": \"%016llx\", \"projected_to\": \"%016llx\", \"active\": \"%016llx\", "
         "\"JpJdF\": \"%016llx\", \"H_A\": \"%016llx\", \"b_A\": \"%016llx\", \"H_sc\": \"%016llx\", \"b_sc\": \"%016llx\", \"acc_top\": \"%016llx\", "
         "\"acc_D\": \"%016llx\", \"acc_E\": \"%016llx\", \"acc_EB\": \"%016llx\", \"acc_Hcc\": \"%016llx\", \"acc_bc\": \"%016llx\", \"hdd_acc\": \"%016llx\", "
         "\"bd_acc\": \"%016llx\", \"hcd_acc\": \"%016llx\", \"hdi\": \"%016llx\", \"bd_sum\": \"%016llx\", \"idepth_hessian\": \"%016llx\", "
         "\"energy\": \"%016llx\", \"new_frame_energy_th\": \"%016llx\", \"lean_equal\": %d}\n",
         nr, n_res_marg, hx(M.verdict, n), hx(M.H_M_out, 8 * Nn * Nn), hx(M.b_M_out, 8 * Nn), hx(M.H_M_points, 8 * N * N), hx(M.b_M_points, 8 * N),
         hx(M.res_to_zero, 32 * nr), hx(J.new_state, nr), hx(J.new_energy, 4 * nr), hx(J.new_energy_with_outlier, 4 * nr),
         hx(J.center_projected_to, 12 * nr), hx(J.projected_to, 64 * nr), hx(H.active, nr), hx(H.JpJdF, 32 * nr), hx(H.H_A, 8 * N * N), hx(H.b_A, 8 * N),
         hx(H.H_sc, 8 * N * N), hx(H.b_sc, 8 * N), hx(H.acc_top, 8 * n2 * 169), hx(H.acc_D, 8 * n2 * nf * 64), hx(H.acc_E, 8 * n2 * 32), hx(H.acc_EB, 8 * n2 * 8),
         hx(H.acc_Hcc, 128), hx(H.acc_bc, 32), hx(H.hdd_acc, 4 * n), hx(H.bd_acc, 4 * n), hx(H.hcd_acc, 16 * n), hx(H.hdi, 4 * n), hx(H.bd_sum, 4 * n),
         hx(H.idepth_hessian, 4 * n), hx(&energy, 8), hx(&th, 4), (int)same);
  return same ? 0 : 1;
}
