// marginalize_host_standalone.cpp -- dsm_window_marginalize_host as a stand-alone CPU program, for a sanitizer run of the host form
// (DESIGN.md section 21): reads a marginalize file (direct_stereo_slam_amd/host/window_case.hpp, which puts every plane and every array
// into a heap block of exactly its size; tests/_marginalize_ref.py writes the checker's scenes), runs the job once with the required
// outputs alone and once with every optional output, and prints one JSON line with the FNV-1a hashes of the outputs, which
// tests/_marginalize_ref.py's hashes reproduces from the checker (every output block starts filled as the ctypes mirror fills it, so
// that what Z leaves alone hashes alike).
// Build, from the repository root:
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       tools/marginalize_host_standalone.cpp direct_stereo_slam_amd/csrc/points_host.cpp direct_stereo_slam_amd/csrc/marginalize_host.cpp \
//       -o marginalize_host_standalone
// The program frees none of its blocks: run it with ASAN_OPTIONS=detect_leaks=0.
#define WINDOW_CASE_STANDALONE
#include "../direct_stereo_slam_amd/host/window_case.hpp"

using namespace window_case;

int main(int argc, char **argv) {
  Case c;
  open_case("marginalize_host_standalone", argc, argv, MARGINALIZE, c);
  dsm_marginalize_job M;
  memset(&M, 0, sizeof M);
  dsm_hessian_job &H = M.hes;
  dsm_linearize_job &J = H.lin;
  fill(M, c);
  const size_t nf = c.nf, n = c.n, nr = c.nr, N = c.N, Nn = N - 8 * c.nm, n2 = nf * nf;
  dsm_linearize_params lp;
  dsm_marginalize_params mp;
  dsm_linearize_params_default(&lp), dsm_marginalize_params_default(&mp);
  auto required = [&]() { // fresh blocks
    linearize_outputs(J, c);
    M.verdict = out<unsigned char>(n), M.H_M_out = out<double>(Nn * Nn), M.b_M_out = out<double>(Nn), M.n_res_marg = out<int>(1);
  };
  auto core = [&]() { return fnv1a(M.verdict, n) ^ fnv1a(M.H_M_out, 8 * Nn * Nn) ^ fnv1a(M.b_M_out, 8 * Nn) ^ fnv1a(J.new_energy, 4 * nr) ^ fnv1a(M.n_res_marg, 4); };
  required(); // the required outputs alone: the host form keeps everything else in room of its own
  int rc = dsm_window_marginalize_host(c.w, c.h, &M, c.planes, &lp, &mp);
  const uint64_t lean = core();
  required(); // every optional output
  linearize_optional(J, c, false, false), hessian_optional(H, c, true);
  M.H_M_points = out<double>(N * N), M.b_M_points = out<double>(N), M.res_to_zero = out<float>(8 * nr);
  if (!rc) rc = dsm_window_marginalize_host(c.w, c.h, &M, c.planes, &lp, &mp);
  if (rc) {
    fprintf(stderr, "marginalize_host_standalone: %d %s\n", rc, dsm::last_error.c_str());
    return 1;
  }
  const bool same = lean == core();
  auto hx = [](const void *p, size_t bytes) { return (unsigned long long)fnv1a(p, bytes); };
  printf("{\"n_res\": %zu, \"n_res_marg\": %d, \"verdict\": \"%016llx\", \"H_M_out\": \"%016llx\", \"b_M_out\": \"%016llx\", \"H_M_points\": \"%016llx\", "
         "\"b_M_points\": \"%016llx\", \"res_to_zero\": \"%016llx\", \"new_state\": \"%016llx\", \"new_energy\": \"%016llx\", "
         "\"new_energy_with_outlier\": \"%016llx\", \"center_projected_to\": \"%016llx\", \"projected_to\": \"%016llx\", \"active\": \"%016llx\", "
         "\"JpJdF\": \"%016llx\", \"H_A\": \"%016llx\", \"b_A\": \"%016llx\", \"H_sc\": \"%016llx\", \"b_sc\": \"%016llx\", \"acc_top\": \"%016llx\", "
         "\"acc_D\": \"%016llx\", \"acc_E\": \"%016llx\", \"acc_EB\": \"%016llx\", \"acc_Hcc\": \"%016llx\", \"acc_bc\": \"%016llx\", \"hdd_acc\": \"%016llx\", "
         "\"bd_acc\": \"%016llx\", \"hcd_acc\": \"%016llx\", \"hdi\": \"%016llx\", \"bd_sum\": \"%016llx\", \"idepth_hessian\": \"%016llx\", "
         "\"energy\": \"%016llx\", \"new_frame_energy_th\": \"%016llx\", \"lean_equal\": %d}\n",
         nr, *M.n_res_marg, hx(M.verdict, n), hx(M.H_M_out, 8 * Nn * Nn), hx(M.b_M_out, 8 * Nn), hx(M.H_M_points, 8 * N * N), hx(M.b_M_points, 8 * N),
         hx(M.res_to_zero, 32 * nr), hx(J.new_state, nr), hx(J.new_energy, 4 * nr), hx(J.new_energy_with_outlier, 4 * nr),
         hx(J.center_projected_to, 12 * nr), hx(J.projected_to, 64 * nr), hx(H.active, nr), hx(H.JpJdF, 32 * nr), hx(H.H_A, 8 * N * N), hx(H.b_A, 8 * N),
         hx(H.H_sc, 8 * N * N), hx(H.b_sc, 8 * N), hx(H.acc_top, 8 * n2 * 169), hx(H.acc_D, 8 * n2 * nf * 64), hx(H.acc_E, 8 * n2 * 32), hx(H.acc_EB, 8 * n2 * 8),
         hx(H.acc_Hcc, 128), hx(H.acc_bc, 32), hx(H.hdd_acc, 4 * n), hx(H.bd_acc, 4 * n), hx(H.hcd_acc, 16 * n), hx(H.hdi, 4 * n), hx(H.bd_sum, 4 * n),
         hx(H.idepth_hessian, 4 * n), hx(J.energy_out, 8), hx(J.new_frame_energy_th_out, 4), (int)same);
  return same ? 0 : 1;
}
