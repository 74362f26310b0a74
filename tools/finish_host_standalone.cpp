// finish_host_standalone.cpp -- dsm_window_finish_host as a stand-alone CPU program, for a sanitizer run of the host form (DESIGN.md
// section 22): reads a finish file (direct_stereo_slam_amd/host/window_case.hpp, which puts every plane and every array into a heap
// block of exactly its size; tests/_finish_ref.py writes the checker's scenes), runs the call once with the required outputs alone and
// once with every optional output, and prints one JSON line with the pattern, the counts and the FNV-1a hashes of the outputs, for a
// comparison with the checker tests/_finish_ref.py (hashes).  Build, from the repository root:
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       tools/finish_host_standalone.cpp direct_stereo_slam_amd/csrc/points_host.cpp direct_stereo_slam_amd/csrc/solve_host.cpp \
//       direct_stereo_slam_amd/csrc/step_host.cpp direct_stereo_slam_amd/csrc/optimize_host.cpp direct_stereo_slam_amd/csrc/finish_host.cpp \
//       -o finish_host_standalone
// Usage: finish_host_standalone FILE [MAX_ITERATIONS = 6] [FORCE_ACCEPT = 0]; tools/host_standalone_check.py DIRECTORY writes the
// cases of the checker's scenes, runs the binary over them and compares the hashes.  The program frees none of its blocks: run it with
// ASAN_OPTIONS=detect_leaks=0.
#define WINDOW_CASE_STANDALONE
#include "../direct_stereo_slam_amd/host/window_case.hpp"

using namespace window_case;

int main(int argc, char **argv) {
  Case c;
  open_case("finish_host_standalone", argc, argv, FINISH, c);
  const int max_its = argc > 2 ? atoi(argv[2]) : 6;
  dsm_finish_job F;
  memset(&F, 0, sizeof F);
  dsm_optimize_job &O = F.opt;
  dsm_step_job &T = O.step;
  dsm_solve_job &S = T.sol;
  fill(F, c);
  optimize_outputs(O, c, max_its);
  dsm_linearize_params lp;
  dsm_step_params sp;
  dsm_optimize_params op;
  dsm_linearize_params_default(&lp), dsm_step_params_default(&sp), dsm_optimize_params_default(&op);
  op.force_accept = argc > 3 ? atoi(argv[3]) : 0;
  // the finish's outputs: every array exactly as long as the call may write
  const size_t nf = c.nf, n = c.n, nr = c.nr, N = c.N, n2 = nf * nf;
  F.world_to_cam_eval_out = out<double>(7 * nf), F.state_zero_out = out<double>(8 * nf), F.state_out = out<double>(8 * nf);
  F.ad_host_out = out<double>(64 * n2), F.ad_target_out = out<double>(64 * n2), F.ad_ht_delta_out = out<float>(8 * n2);
  F.c_delta_out = out<float>(4), F.delta_x_out = out<double>(N), F.cam_out = out<float>(6);
  F.pre_RTll_0_out = out<float>(9 * n2), F.pre_tTll_0_out = out<float>(3 * n2), F.pre_KRKiTll_out = out<float>(9 * n2);
  F.pre_KtTll_out = out<float>(3 * n2), F.pre_aff_mode_out = out<float>(2 * n2), F.pre_b0_mode_out = out<float>(n2);
  F.new_state = out<unsigned char>(nr), F.new_energy = out<float>(nr), F.new_energy_with_outlier = out<float>(nr);
  F.keep = out<unsigned char>(nr), F.rel_bs = out<float>(nr), F.energy = out<double>(1), F.frame_energy_th_out = out<float>(1);
  F.n_good_residuals_out = out<int>(n), F.max_rel_baseline_out = out<float>(n), F.last_res_out = out<int>(2 * n);
  F.last_state_out = out<unsigned char>(2 * n), F.n_res_kept = out<int>(n), F.point_dropped = out<unsigned char>(n);
  F.res_index_out = out<int>(nr), F.point_index_out = out<int>(n), F.n_res_out = out<int>(1), F.n_pts_out = out<int>(1);
  F.rmse = out<float>(1), F.lost = out<int>(1);
  // the required outputs alone
  int rc = dsm_window_finish_host(c.w, c.h, &F, c.planes, &lp, &sp, &op);
  const uint64_t x_lean = fnv1a(S.x, 8 * N), keep_lean = fnv1a(F.keep, nr), dp_lean = fnv1a(F.ad_ht_delta_out, 32 * n2);
  // every optional output, the loop's and the finish's
  step_optional(T, c), linearize_optional(S.hes.lin, c, false, true), hessian_optional(S.hes, c, false);
  F.cam_to_world_out = out<double>(7 * nf), F.J_out = out<float>((size_t)DSM_LINEARIZE_J_FLOATS * nr);
  if (!rc) rc = dsm_window_finish_host(c.w, c.h, &F, c.planes, &lp, &sp, &op);
  if (rc) {
    fprintf(stderr, "finish_host_standalone: %d %s\n", rc, dsm::last_error.c_str());
    return 1;
  }
  const bool same = x_lean == fnv1a(S.x, 8 * N) && keep_lean == fnv1a(F.keep, nr) && dp_lean == fnv1a(F.ad_ht_delta_out, 32 * n2);
  auto hx = [](uint64_t h) { return (unsigned long long)h; };
  const std::string pattern((const char *)O.pattern, (size_t)*O.n_iterations);
  printf("{\"n_res\": %zu, \"pattern\": \"%s\", \"passes\": %d, \"n_res_out\": %d, \"n_pts_out\": %d, \"lost\": %d, \"x\": \"%016llx\", "
         "\"eval\": \"%016llx\", \"state\": \"%016llx\", \"ad_host\": \"%016llx\", \"ad_target\": \"%016llx\", \"ad_ht_delta\": \"%016llx\", "
         "\"delta_x\": \"%016llx\", \"tables\": \"%016llx\", \"new_state\": \"%016llx\", \"new_energy\": \"%016llx\", \"keep\": \"%016llx\", "
         "\"rel_bs\": \"%016llx\", \"energy\": \"%016llx\", \"n_good\": \"%016llx\", \"max_rel_baseline\": \"%016llx\", \"last_res\": \"%016llx\", "
         "\"last_state\": \"%016llx\", \"res_index\": \"%016llx\", \"point_index\": \"%016llx\", \"cam_to_world\": \"%016llx\", \"lean_equal\": %d}\n",
         nr, pattern.c_str(), *O.n_passes, *F.n_res_out, *F.n_pts_out, *F.lost, hx(fnv1a(S.x, 8 * N)), hx(fnv1a(F.world_to_cam_eval_out, 56 * nf)),
         hx(fnv1a(F.state_out, 64 * nf)), hx(fnv1a(F.ad_host_out, 512 * n2)), hx(fnv1a(F.ad_target_out, 512 * n2)), hx(fnv1a(F.ad_ht_delta_out, 32 * n2)),
         hx(fnv1a(F.delta_x_out, 8 * N)),
         hx(tables_hash(F.pre_RTll_0_out, F.pre_tTll_0_out, F.pre_KRKiTll_out, F.pre_KtTll_out, F.pre_aff_mode_out, F.pre_b0_mode_out, n2)),
         hx(fnv1a(F.new_state, nr)), hx(fnv1a(F.new_energy, 4 * nr)), hx(fnv1a(F.keep, nr)), hx(fnv1a(F.rel_bs, 4 * nr)), hx(fnv1a(F.energy, 8)),
         hx(fnv1a(F.n_good_residuals_out, 4 * n)), hx(fnv1a(F.max_rel_baseline_out, 4 * n)), hx(fnv1a(F.last_res_out, 8 * n)), hx(fnv1a(F.last_state_out, 2 * n)),
         hx(fnv1a(F.res_index_out, 4 * nr)), hx(fnv1a(F.point_index_out, 4 * n)), hx(fnv1a(F.cam_to_world_out, 56 * nf)), (int)same);
  return same ? 0 : 1;
}
