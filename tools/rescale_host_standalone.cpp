// rescale_host_standalone.cpp -- dsm_window_rescale_host as a stand-alone CPU program, for a sanitizer run of the host form (DESIGN.md
// section 25): reads a rescale job (the layout is tests/_rescale_ref.py's write_case), puts every array into a heap block of exactly
// its size, runs the job once with every output and once without the optional one, then both in one call, then a refused job, and
// prints one JSON line with the words and the FNV-1a hashes of every output, which tests/_rescale_ref.py's hashes reproduces from the
// checker (tools/host_standalone_check.py).  Build, from the repository root:
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       tools/rescale_host_standalone.cpp direct_stereo_slam_amd/csrc/points_host.cpp direct_stereo_slam_amd/csrc/solve_host.cpp \
//       direct_stereo_slam_amd/csrc/step_host.cpp direct_stereo_slam_amd/csrc/rescale_host.cpp -o rescale_host_standalone
// (points_host.cpp, solve_host.cpp and step_host.cpp for the parameter defaults and their rules.)
// The program frees none of its blocks: run it with ASAN_OPTIONS=detect_leaks=0.
#define WINDOW_CASE_STANDALONE
#include "../direct_stereo_slam_amd/host/window_case.hpp" // block, read_block, fnv1a and the dsm::set_error / dsm::invalid stubs

using window_case::block;
using window_case::fnv1a;
using window_case::read_block;
static const char *const PROGRAM = "rescale_host_standalone";

static dsm_rescale_job with_outputs(dsm_rescale_job j, bool optional) {
  const size_t n = j.n_frames, n2 = n * n, N = 4 + 8 * n, np = j.n_pts;
  j.idepth_out = block<float>(np), j.idepth_scaled_out = block<float>(np), j.idepth_zero_scaled_out = block<float>(np), j.delta_out = block<float>(np);
  j.world_to_cam_eval_out = block<double>(7 * n), j.state_out = block<double>(8 * n), j.state_zero_out = block<double>(8 * n);
  j.cam_to_tracking_ref_out = block<double>(7), j.cam_to_world_out = block<double>(7);
  j.pre_RTll_0_out = block<float>(9 * n2), j.pre_tTll_0_out = block<float>(3 * n2), j.pre_KRKiTll_out = block<float>(9 * n2);
  j.pre_KtTll_out = block<float>(3 * n2), j.pre_aff_mode_out = block<float>(2 * n2), j.pre_b0_mode_out = block<float>(n2);
  j.cam_out = block<float>(6), j.c_delta_out = block<float>(4), j.delta_x_out = block<double>(N), j.ad_ht_delta_out = block<float>(8 * n2);
  j.world_to_cam_out = block<double>(7 * n), j.cam_to_world_out_all = optional ? block<double>(7 * n) : nullptr;
  j.decision = block<int>(1), j.scale_error_out = block<float>(1), j.trapped_out = block<int>(1), j.fails_out = block<int>(1), j.applied_scale = block<float>(1);
  return j;
}
static bool same_core(const dsm_rescale_job &a, const dsm_rescale_job &b) {
  const size_t n = a.n_frames, n2 = n * n, np = a.n_pts;
  return *a.decision == *b.decision && !memcmp(a.idepth_out, b.idepth_out, 4 * np) && !memcmp(a.idepth_scaled_out, b.idepth_scaled_out, 4 * np) &&
         !memcmp(a.world_to_cam_eval_out, b.world_to_cam_eval_out, 56 * n) && !memcmp(a.state_out, b.state_out, 64 * n) &&
         !memcmp(a.pre_KRKiTll_out, b.pre_KRKiTll_out, 36 * n2) && !memcmp(a.pre_KtTll_out, b.pre_KtTll_out, 12 * n2) &&
         !memcmp(a.ad_ht_delta_out, b.ad_ht_delta_out, 32 * n2) && !memcmp(a.delta_x_out, b.delta_x_out, 8 * (4 + 8 * n)) &&
         !memcmp(a.world_to_cam_out, b.world_to_cam_out, 56 * n);
}

int main(int argc, char **argv) {
  FILE *f = argc > 1 ? fopen(argv[1], "rb") : nullptr;
  if (!f) {
    fprintf(stderr, "usage: rescale_host_standalone FILE\n");
    return 2;
  }
  const int *head = read_block<int>(f, 5, PROGRAM);
  const float *words = read_block<float>(f, 3, PROGRAM);
  const double *g2l = read_block<double>(f, 2, PROGRAM);
  if (head[0] < 1 || head[0] > DSM_WINDOW_MAX_FRAMES || head[1] < 0) {
    fprintf(stderr, "rescale_host_standalone: n_frames or n_pts\n");
    return 2;
  }
  const size_t n = head[0], n2 = n * n, N = 4 + 8 * n, np = head[1];
  dsm_rescale_job in;
  memset(&in, 0, sizeof in);
  in.n_frames = head[0], in.n_pts = head[1], in.enabled = head[2], in.trapped = head[3], in.fails = head[4];
  in.scale_error = words[0], in.new_scale = words[1], in.thres = words[2], in.aff_g2l[0] = g2l[0], in.aff_g2l[1] = g2l[1];
  in.idepth = read_block<float>(f, np, PROGRAM), in.idepth_scaled = read_block<float>(f, np, PROGRAM);
  in.idepth_zero_scaled = read_block<float>(f, np, PROGRAM), in.delta = read_block<float>(f, np, PROGRAM);
  in.world_to_cam_eval = read_block<double>(f, 7 * n, PROGRAM), in.state = read_block<double>(f, 8 * n, PROGRAM);
  in.state_zero = read_block<double>(f, 8 * n, PROGRAM), in.exposure = read_block<float>(f, n, PROGRAM);
  in.cam_to_tracking_ref = read_block<double>(f, 7, PROGRAM), in.ref_cam_to_world = read_block<double>(f, 7, PROGRAM);
  in.cam_to_world = read_block<double>(f, 7, PROGRAM), in.calib_value = read_block<double>(f, 4, PROGRAM), in.calib_zero = read_block<double>(f, 4, PROGRAM);
  in.ad_host = read_block<double>(f, 64 * n2, PROGRAM), in.ad_target = read_block<double>(f, 64 * n2, PROGRAM);
  in.pre_RTll_0 = read_block<float>(f, 9 * n2, PROGRAM), in.pre_tTll_0 = read_block<float>(f, 3 * n2, PROGRAM), in.pre_KRKiTll = read_block<float>(f, 9 * n2, PROGRAM);
  in.pre_KtTll = read_block<float>(f, 3 * n2, PROGRAM), in.pre_aff_mode = read_block<float>(f, 2 * n2, PROGRAM), in.pre_b0_mode = read_block<float>(f, n2, PROGRAM);
  in.cam = read_block<float>(f, 6, PROGRAM), in.c_delta = read_block<float>(f, 4, PROGRAM), in.delta_x = read_block<double>(f, N, PROGRAM);
  in.ad_ht_delta = read_block<float>(f, 8 * n2, PROGRAM), in.world_to_cam = read_block<double>(f, 7 * n, PROGRAM);
  in.cam_to_world_all = read_block<double>(f, 7 * n, PROGRAM);
  fclose(f);

  dsm_rescale_job full = with_outputs(in, true), bare = with_outputs(in, false);
  dsm_linearize_params lp;
  dsm_step_params sp;
  dsm_linearize_params_default(&lp), dsm_step_params_default(&sp);
  if (dsm_window_rescale_host(1, &full, &lp, &sp) != DSM_OK || dsm_window_rescale_host(1, &bare, nullptr, nullptr) != DSM_OK) {
    fprintf(stderr, "rescale_host_standalone: %s\n", dsm::last_error.c_str());
    return 1;
  }
  dsm_rescale_job *two = block<dsm_rescale_job>(2);
  two[0] = with_outputs(in, false), two[1] = with_outputs(in, true);
  if (dsm_window_rescale_host(2, two, nullptr, nullptr) != DSM_OK) return 1;
  const int forms_equal = same_core(full, bare) && same_core(full, two[0]) && same_core(full, two[1]) &&
                          !memcmp(full.cam_to_world_out_all, two[1].cam_to_world_out_all, 56 * n);
  dsm_rescale_job refused = with_outputs(in, false); // V: refused before an output is touched
  refused.new_scale = 0.0f;
  *refused.decision = 77;
  const int refusal = dsm_window_rescale_host(1, &refused, nullptr, nullptr) == DSM_ERR_INVALID && *refused.decision == 77;
  auto x = [](const void *p, size_t bytes) { return (unsigned long long)fnv1a(p, bytes); };
  const dsm_rescale_job &o = full;
  printf("{\"decision\": %d, \"trapped\": %d, \"fails\": %d, \"scale_error\": \"%016llx\", \"applied_scale\": \"%016llx\", \"idepth\": \"%016llx\", "
         "\"idepth_scaled\": \"%016llx\", \"idepth_zero_scaled\": \"%016llx\", \"delta\": \"%016llx\", \"eval\": \"%016llx\", \"state\": \"%016llx\", "
         "\"state_zero\": \"%016llx\", \"cam_to_tracking_ref\": \"%016llx\", \"cam_to_world\": \"%016llx\", \"tables\": \"%016llx\", \"cam\": \"%016llx\", "
         "\"c_delta\": \"%016llx\", \"delta_x\": \"%016llx\", \"ad_ht_delta\": \"%016llx\", \"world_to_cam\": \"%016llx\", \"cam_to_world_all\": \"%016llx\", "
         "\"forms_equal\": %d, \"refusal\": %d}\n",
         *o.decision, *o.trapped_out, *o.fails_out, x(o.scale_error_out, 4), x(o.applied_scale, 4), x(o.idepth_out, 4 * np), x(o.idepth_scaled_out, 4 * np),
         x(o.idepth_zero_scaled_out, 4 * np), x(o.delta_out, 4 * np), x(o.world_to_cam_eval_out, 56 * n), x(o.state_out, 64 * n), x(o.state_zero_out, 64 * n),
         x(o.cam_to_tracking_ref_out, 56), x(o.cam_to_world_out, 56),
         (unsigned long long)window_case::tables_hash(o.pre_RTll_0_out, o.pre_tTll_0_out, o.pre_KRKiTll_out, o.pre_KtTll_out, o.pre_aff_mode_out, o.pre_b0_mode_out, n2),
         x(o.cam_out, 24), x(o.c_delta_out, 16), x(o.delta_x_out, 8 * N), x(o.ad_ht_delta_out, 32 * n2), x(o.world_to_cam_out, 56 * n),
         x(o.cam_to_world_out_all, 56 * n), forms_equal, refusal);
  return forms_equal && refusal ? 0 : 1;
}
