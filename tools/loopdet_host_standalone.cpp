// loopdet_host_standalone.cpp -- the host forms of the loop descriptors (dsm_generate_spherical_points, dsm_scancontext_generate:
// csrc/host_capi.cpp) as a stand-alone CPU program, for a sanitizer run ("edges"): the non-finite points of
// tests/_loopdet_cases.py (NaN and +-inf in each coordinate, 1e308 in two, under the identity and under a pose that turns an inf into a
// NaN) between six finite points, then the descriptor at (num_s, num_r) = (256, 256) and at (1, 1).  Every array is a heap block of
// exactly its size.  Exit status 0 and one line "ok ..." when the non-finite points were dropped and the finite ones came through.
// Build, from the repository root:
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined tools/loopdet_host_standalone.cpp direct_stereo_slam_amd/csrc/host_capi.cpp -o loopdet_host_standalone
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>

#define WINDOW_CASE_STANDALONE
#include "../direct_stereo_slam_amd/host/window_case.hpp" // block, fnv1a and the dsm::set_error stub

using window_case::block;

int main() {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  const double finite[6][3] = {{1.3, 0.7, -0.4}, {-0.6, 1.1, 0.9}, {0.4, -1.2, -1.1}, {-1.4, 0.3, -0.7}, {0.8, 0.9, 1.2}, {-0.3, -0.8, 1.4}};
  const double bad_v[3] = {nan, inf, -inf};
  const int n_bad = 11, n = n_bad + 6;
  double *xyz = block<double>(3 * n);
  int *pt_kf = block<int>(n), *is_finite = block<int>(n);
  int nf = 0, nb = 0;
  for (int i = 0; i < n; i++) { // the finite points stand between the others
    pt_kf[i] = 5;
    is_finite[i] = (i % 3 == 1 && nf < 6);
    if (is_finite[i]) {
      memcpy(xyz + 3 * i, finite[nf++], sizeof finite[0]);
      continue;
    }
    double p[3] = {0.3, 0.3, 0.3};
    if (nb < 9) p[nb % 3] = bad_v[nb / 3];
    else if (nb == 9) p[0] = 1e308, p[1] = 1e308, p[2] = 0.0;
    else p[0] = -1e308, p[1] = 0.0, p[2] = 1e308;
    nb++;
    memcpy(xyz + 3 * i, p, sizeof p);
  }
  if (nf != 6 || nb != n_bad) return 2;
  const int kf_ids[1] = {5};
  const double pose[6] = {0, 0, 0, 0, 0, 0};
  const double c = std::cos(0.1), s = std::sin(0.1);
  const double cws[2][12] = {{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, {c, 0, s, 0.05, 0, 1, 0, -0.02, -s, 0, c, 0.03}};
  int total_sig = 0;
  for (int pass = 0; pass < 2; pass++) {
    int keep[1], n_out = -1;
    int *sel = block<int>(n);
    double *sph = block<double>(3 * n);
    if (dsm_generate_spherical_points(1, kf_ids, pose, cws[pass], 2.0, n, pt_kf, xyz, keep, &n_out, sel, sph) != DSM_OK) return 3;
    if (n_out != 6 || keep[0] != 1) return 4;
    for (int k = 0; k < n_out; k++)
      if (!is_finite[sel[k]] || !std::isfinite(sph[3 * k]) || !std::isfinite(sph[3 * k + 1]) || !std::isfinite(sph[3 * k + 2])) return 5;
    const int shapes[2][2] = {{256, 256}, {1, 1}};
    for (int q = 0; q < 2; q++) {
      const int num_s = shapes[q][0], num_r = shapes[q][1];
      float *ringkey = block<float>(num_r);
      int *sig_idx = block<int>((size_t)num_s * num_r), n_sig = -1;
      double *sig_val = block<double>((size_t)num_s * num_r), *tfm = block<double>(16);
      if (dsm_scancontext_generate(sph, n_out, 2.0, num_s, num_r, ringkey, sig_idx, sig_val, &n_sig, tfm) != DSM_OK) return 6;
      if (n_sig < 1 || n_sig > n_out) return 7;
      for (int k = 0; k < n_sig; k++)
        if (sig_idx[k] < 0 || sig_idx[k] >= num_s * num_r) return 8;
      total_sig += n_sig;
      free(ringkey), free(sig_idx), free(sig_val), free(tfm);
    }
    free(sel), free(sph);
  }
  free(xyz), free(pt_kf), free(is_finite);
  printf("ok: %d non-finite points dropped twice, %d signature entries\n", n_bad, total_sig);
  return 0;
}
