// step_host_standalone.cpp -- dsm_window_step_host as a stand-alone CPU program, for a sanitizer run of the host form (DESIGN.md
// section 19): reads a step file (direct_stereo_slam_amd/host/window_case.hpp, which puts every plane and every array into a heap block
// of exactly its size; tests/_step_ref.py writes the checker's scenes), runs the job once with the required outputs alone and once with
// every optional output, and prints one JSON line with the FNV-1a hashes of the outputs, which tests/_step_ref.py's hashes() reproduces
// from the checker.  Build, from the repository root:
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       tools/step_host_standalone.cpp direct_stereo_slam_amd/csrc/points_host.cpp direct_stereo_slam_amd/csrc/solve_host.cpp \
//       direct_stereo_slam_amd/csrc/step_host.cpp -o step_host_standalone
// The program frees none of its blocks: run it with ASAN_OPTIONS=detect_leaks=0.
#define WINDOW_CASE_STANDALONE
#include "../direct_stereo_slam_amd/host/window_case.hpp"

using namespace window_case;

int main(int argc, char **argv) {
  Case c;
  open_case("step_host_standalone", argc, argv, STEP, c);
  dsm_step_job T;
  memset(&T, 0, sizeof T);
  dsm_solve_job &S = T.sol;
  fill(T, c, true);
  step_outputs(T, c);
  dsm_linearize_params lp;
  dsm_step_params sp;
  dsm_linearize_params_default(&lp), dsm_step_params_default(&sp);
  // the required outputs alone: the host form keeps everything else in room of its own
  int rc = dsm_window_step_host(c.w, c.h, &T, c.planes, &lp, &sp);
  const size_t nf = c.nf, n = c.n, N = c.N;
  const uint64_t x_lean = fnv1a(S.x, 8 * N), state_lean = fnv1a(T.state_out, 64 * nf);
  // every optional output
  step_optional(T, c), linearize_optional(S.hes.lin, c, true, false), hessian_optional(S.hes, c, true), solve_optional(S, c);
  if (!rc) rc = dsm_window_step_host(c.w, c.h, &T, c.planes, &lp, &sp);
  if (rc) {
    fprintf(stderr, "step_host_standalone: %d %s\n", rc, dsm::last_error.c_str());
    return 1;
  }
  const bool same = x_lean == fnv1a(S.x, 8 * N) && state_lean == fnv1a(T.state_out, 64 * nf);
  const uint64_t pre = tables_hash(T.pre_RTll_0_out, T.pre_tTll_0_out, T.pre_KRKiTll_out, T.pre_KtTll_out, T.pre_aff_mode_out, T.pre_b0_mode_out, nf * nf);
  auto hx = [](uint64_t h) { return (unsigned long long)h; };
  printf("{\"n_res\": %zu, \"state\": \"%016llx\", \"calib\": \"%016llx\", \"idepth\": \"%016llx\", \"world_to_cam\": \"%016llx\", "
         "\"cam_to_world\": \"%016llx\", \"cam\": \"%016llx\", \"pre\": \"%016llx\", \"delta_x\": \"%016llx\", \"H_L\": \"%016llx\", \"b_L\": \"%016llx\", "
         "\"energy_m\": \"%016llx\", \"x\": \"%016llx\", \"step\": \"%016llx\", \"new_energy\": \"%016llx\", \"can_break\": %d, \"flags\": %d, "
         "\"lean_equal\": %d}\n",
         c.nr, hx(fnv1a(T.state_out, 64 * nf)), hx(fnv1a(T.calib_out, 32)), hx(fnv1a(T.idepth_out, 4 * n)), hx(fnv1a(T.world_to_cam_out, 56 * nf)),
         hx(fnv1a(T.cam_to_world_out, 56 * nf)), hx(fnv1a(T.cam_out, 24)), hx(pre), hx(fnv1a(T.delta_x_out, 8 * N)), hx(fnv1a(T.H_L_out, 8 * N * N)),
         hx(fnv1a(T.b_L_out, 8 * N)), hx(fnv1a(T.energy_m, 8)), hx(fnv1a(S.x, 8 * N)), hx(fnv1a(S.step, 4 * n)), hx(fnv1a(S.hes.lin.new_energy, 4 * c.nr)),
         *T.can_break, *S.flags, (int)same);
  return same ? 0 : 1;
}
