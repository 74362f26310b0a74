// optimize_host_standalone.cpp -- dsm_window_optimize_host as a stand-alone CPU program, for a sanitizer run of the host form (DESIGN.md
// section 20): reads a step file (direct_stereo_slam_amd/host/window_case.hpp, which puts every plane and every array into a heap block
// of exactly its size; its state_backup, calib_backup and idepth_backup are the state the loop starts from, its steps, factors and lambda
// are not used), runs the loop once with the required outputs alone and once with every optional output, and prints one JSON line with
// the pattern, the passes and the FNV-1a hashes of the outputs, for a comparison with the checker tests/_optimize_ref.py.  Build, from
// the repository root:
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       tools/optimize_host_standalone.cpp direct_stereo_slam_amd/csrc/points_host.cpp direct_stereo_slam_amd/csrc/solve_host.cpp \
//       direct_stereo_slam_amd/csrc/step_host.cpp direct_stereo_slam_amd/csrc/optimize_host.cpp -o optimize_host_standalone
// Usage: optimize_host_standalone FILE [MAX_ITERATIONS = 6] [STEP_MOMENTUM = 0].  The program frees none of its blocks: run it with
// ASAN_OPTIONS=detect_leaks=0.
#define WINDOW_CASE_STANDALONE
#include "../direct_stereo_slam_amd/host/window_case.hpp"

using namespace window_case;

int main(int argc, char **argv) {
  Case c;
  open_case("optimize_host_standalone", argc, argv, STEP, c);
  const int max_its = argc > 2 ? atoi(argv[2]) : 6;
  dsm_optimize_job O;
  memset(&O, 0, sizeof O);
  dsm_step_job &T = O.step;
  dsm_solve_job &S = T.sol;
  fill(T, c, false);
  optimize_outputs(O, c, max_its);
  dsm_linearize_params lp;
  dsm_step_params sp;
  dsm_optimize_params op;
  dsm_linearize_params_default(&lp), dsm_step_params_default(&sp), dsm_optimize_params_default(&op);
  op.step_momentum = argc > 3 ? atoi(argv[3]) : 0;
  // the required outputs alone: the host form keeps everything else in room of its own
  int rc = dsm_window_optimize_host(c.w, c.h, &O, c.planes, &lp, &sp, &op);
  const size_t nf = c.nf, n = c.n, N = c.N;
  const uint64_t x_lean = fnv1a(S.x, 8 * N), state_lean = fnv1a(T.state_out, 64 * nf);
  // every optional output
  step_optional(T, c), linearize_optional(S.hes.lin, c, true, true), hessian_optional(S.hes, c, true), solve_optional(S, c);
  if (!rc) rc = dsm_window_optimize_host(c.w, c.h, &O, c.planes, &lp, &sp, &op);
  if (rc) {
    fprintf(stderr, "optimize_host_standalone: %d %s\n", rc, dsm::last_error.c_str());
    return 1;
  }
  const bool same = x_lean == fnv1a(S.x, 8 * N) && state_lean == fnv1a(T.state_out, 64 * nf);
  auto hx = [](uint64_t h) { return (unsigned long long)h; };
  const size_t n_iterations = (size_t)*O.n_iterations, n_passes = (size_t)*O.n_passes;
  const std::string pattern((const char *)O.pattern, n_iterations);
  const double last = O.last_energy[0] + O.last_energy[1];
  printf("{\"n_res\": %zu, \"pattern\": \"%s\", \"passes\": %d, \"state\": \"%016llx\", \"calib\": \"%016llx\", \"idepth\": \"%016llx\", "
         "\"x\": \"%016llx\", \"step\": \"%016llx\", \"new_energy\": \"%016llx\", \"pass_energy\": \"%016llx\", \"pass_lambda\": \"%016llx\", "
         "\"iter_stepsize\": \"%016llx\", \"last\": \"%016llx\", \"frame_energy_th\": \"%016llx\", \"flags\": %d, \"lean_equal\": %d}\n",
         c.nr, pattern.c_str(), *O.n_passes, hx(fnv1a(T.state_out, 64 * nf)), hx(fnv1a(T.calib_out, 32)), hx(fnv1a(T.idepth_out, 4 * n)), hx(fnv1a(S.x, 8 * N)),
         hx(fnv1a(S.step, 4 * n)), hx(fnv1a(S.hes.lin.new_energy, 4 * c.nr)), hx(fnv1a(O.pass_energy, 16 * n_passes)), hx(fnv1a(O.pass_lambda, 8 * n_passes)),
         hx(fnv1a(O.iter_stepsize, 4 * n_iterations)), hx(fnv1a(&last, 8)), hx(fnv1a(O.frame_energy_th_out, 4)), *S.flags, (int)same);
  return same ? 0 : 1;
}
