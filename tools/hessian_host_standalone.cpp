// hessian_host_standalone.cpp -- dsm_window_hessian_host as a stand-alone CPU program, for a sanitizer run of the host form (DESIGN.md
// section 17): reads a hessian file (direct_stereo_slam_amd/host/window_case.hpp, which puts every plane and every array into a heap
// block of exactly its size), asks for every optional output, and prints one JSON line with the FNV-1a hashes of H_A, b_A, H_sc, b_sc
// and of the raw accumulators, which tests/_window_files.py's fnv1a reproduces from the checker.  Build, from the repository root:
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       tools/hessian_host_standalone.cpp direct_stereo_slam_amd/csrc/points_host.cpp -o hessian_host_standalone
// The program frees none of its blocks: run it with ASAN_OPTIONS=detect_leaks=0.
#define WINDOW_CASE_STANDALONE
#include "../direct_stereo_slam_amd/host/window_case.hpp"

using namespace window_case;

int main(int argc, char **argv) {
  Case c;
  open_case("hessian_host_standalone", argc, argv, HESSIAN, c);
  dsm_hessian_job H;
  memset(&H, 0, sizeof H);
  fill(H, c);
  linearize_outputs(H.lin, c), linearize_optional(H.lin, c, true, false), hessian_optional(H, c, true);
  dsm_linearize_params params;
  dsm_linearize_params_default(&params);
  const int rc = dsm_window_hessian_host(c.w, c.h, &H, c.planes, &params);
  if (rc) {
    fprintf(stderr, "hessian_host_standalone: %d %s\n", rc, dsm::last_error.c_str());
    return 1;
  }
  const size_t N = c.N, n2 = c.nf * c.nf;
  size_t n_active = 0;
  for (size_t i = 0; i < c.nr; i++) n_active += H.active[i];
  printf("{\"n_res\": %zu, \"n_active\": %zu, \"H_A\": \"%016llx\", \"b_A\": \"%016llx\", \"H_sc\": \"%016llx\", \"b_sc\": \"%016llx\", "
         "\"acc_top\": \"%016llx\", \"acc_D\": \"%016llx\", \"hdi\": \"%016llx\"}\n",
         c.nr, n_active, (unsigned long long)fnv1a(H.H_A, 8 * N * N), (unsigned long long)fnv1a(H.b_A, 8 * N), (unsigned long long)fnv1a(H.H_sc, 8 * N * N),
         (unsigned long long)fnv1a(H.b_sc, 8 * N), (unsigned long long)fnv1a(H.acc_top, 8 * n2 * 169), (unsigned long long)fnv1a(H.acc_D, 8 * n2 * c.nf * 64),
         (unsigned long long)fnv1a(H.hdi, 4 * c.n));
  return 0;
}
