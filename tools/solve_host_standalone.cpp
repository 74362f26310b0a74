// solve_host_standalone.cpp -- dsm_window_solve_host as a stand-alone CPU program, for a sanitizer run of the host form (DESIGN.md
// section 18): reads a solve file (direct_stereo_slam_amd/host/window_case.hpp, which puts every plane and every array into a heap block
// of exactly its size), runs the job once with the required outputs alone and once with every optional output, and prints one JSON line
// with the FNV-1a hashes of x, the steps, last_HS and last_bS, which tests/_window_files.py's fnv1a reproduces from the checker.
// Build, from the repository root:
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       tools/solve_host_standalone.cpp direct_stereo_slam_amd/csrc/points_host.cpp direct_stereo_slam_amd/csrc/solve_host.cpp \
//       -o solve_host_standalone
// The program frees none of its blocks: run it with ASAN_OPTIONS=detect_leaks=0.
#define WINDOW_CASE_STANDALONE
#include "../direct_stereo_slam_amd/host/window_case.hpp"

using namespace window_case;

int main(int argc, char **argv) {
  Case c;
  open_case("solve_host_standalone", argc, argv, SOLVE, c);
  dsm_solve_job S;
  memset(&S, 0, sizeof S);
  fill(S, c);
  solve_outputs(S, c);
  dsm_linearize_params params;
  dsm_linearize_params_default(&params);
  // the required outputs alone: the host form keeps everything else in room of its own
  int rc = dsm_window_solve_host(c.w, c.h, &S, c.planes, &params);
  const size_t N = c.N;
  const uint64_t x_lean = fnv1a(S.x, 8 * N), step_lean = fnv1a(S.step, 4 * c.n);
  // every optional output
  linearize_optional(S.hes.lin, c, true, false), hessian_optional(S.hes, c, true), solve_optional(S, c);
  if (!rc) rc = dsm_window_solve_host(c.w, c.h, &S, c.planes, &params);
  if (rc) {
    fprintf(stderr, "solve_host_standalone: %d %s\n", rc, dsm::last_error.c_str());
    return 1;
  }
  const bool same = x_lean == fnv1a(S.x, 8 * N) && step_lean == fnv1a(S.step, 4 * c.n);
  printf("{\"n_res\": %zu, \"x\": \"%016llx\", \"step\": \"%016llx\", \"last_HS\": \"%016llx\", \"last_bS\": \"%016llx\", \"flags\": %d, "
         "\"lean_equal\": %d}\n",
         c.nr, (unsigned long long)fnv1a(S.x, 8 * N), (unsigned long long)fnv1a(S.step, 4 * c.n), (unsigned long long)fnv1a(S.last_HS, 8 * N * N),
         (unsigned long long)fnv1a(S.last_bS, 8 * N), *S.flags, (int)same);
  return same ? 0 : 1;
}
