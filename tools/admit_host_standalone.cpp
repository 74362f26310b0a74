// admit_host_standalone.cpp -- dsm_window_admit_host as a stand-alone CPU program, for a sanitizer run of the host form (DESIGN.md
// section 26): reads an admission job (the layout is tests/_admit_ref.py's write_case), puts every array into a heap block of exactly
// its size, runs the job as given, once more without the optional arrays, then both in one call, then a refused job, and prints one
// JSON line with the words and one FNV-1a hash per output ("-" for an optional array that is absent), which tests/_admit_ref.py's
// hashes reproduces from the checker (tools/host_standalone_check.py).  Build, from the repository root:
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       tools/admit_host_standalone.cpp direct_stereo_slam_amd/csrc/points_host.cpp direct_stereo_slam_amd/csrc/solve_host.cpp \
//       direct_stereo_slam_amd/csrc/step_host.cpp direct_stereo_slam_amd/csrc/rescale_host.cpp direct_stereo_slam_amd/csrc/admit_host.cpp \
//       -o admit_host_standalone
// (points_host.cpp, solve_host.cpp and step_host.cpp for the parameter defaults and their rules, rescale_host.cpp for the scales.)
// The program frees none of its blocks: run it with ASAN_OPTIONS=detect_leaks=0.
#define WINDOW_CASE_STANDALONE
#include "../direct_stereo_slam_amd/host/window_case.hpp" // block, read_block, fnv1a and the dsm::set_error / dsm::invalid stubs

#include <string>

using window_case::block;
using window_case::fnv1a;
using window_case::read_block;
static const char *const PROGRAM = "admit_host_standalone";

static dsm_admit_job with_outputs(dsm_admit_job j, bool optional) {
  const size_t n = j.n_frames, m = n + 1, m2 = m * m, M = 12 + 8 * n, np = j.n_pts, no = np + j.n_res;
  if (!optional) j.H_M = j.b_M = j.H_L = j.b_L = j.prior = j.prior_zero = nullptr;
  j.world_to_cam_eval_out = block<double>(7 * m), j.state_out = block<double>(8 * m), j.state_zero_out = block<double>(8 * m);
  j.exposure_out = block<float>(m), j.frame_energy_th_out = block<float>(m), j.keyframe_id_out = block<int>(m), j.world_to_cam_out = block<double>(7 * m);
  j.flagged_out = block<unsigned char>(m), j.cam_to_world_out = block<double>(7);
  j.pre_RTll_0_out = block<float>(9 * m2), j.pre_tTll_0_out = block<float>(3 * m2), j.pre_KRKiTll_out = block<float>(9 * m2);
  j.pre_KtTll_out = block<float>(3 * m2), j.pre_aff_mode_out = block<float>(2 * m2), j.pre_b0_mode_out = block<float>(m2);
  j.distance_ll_out = optional ? block<float>(m2) : nullptr;
  j.cam_out = block<float>(6), j.c_delta_out = block<float>(4), j.delta_x_out = block<double>(M);
  j.ad_host_out = block<double>(64 * m2), j.ad_target_out = block<double>(64 * m2), j.ad_ht_delta_out = block<float>(8 * m2);
  j.H_M_out = j.H_M ? block<double>(M * M) : nullptr, j.b_M_out = j.b_M ? block<double>(M) : nullptr;
  j.H_L_out = j.H_L ? block<double>(M * M) : nullptr, j.b_L_out = j.b_L ? block<double>(M) : nullptr;
  j.prior_out = j.prior ? block<double>(M) : nullptr, j.prior_zero_out = j.prior ? block<double>(M) : nullptr;
  j.frame_prior_out = block<double>(8), j.frame_delta_prior_out = block<double>(8);
  j.point_out = block<int>(no), j.target_out = block<int>(no), j.res_state_out = block<unsigned char>(no), j.energy_out = block<float>(no);
  j.is_new_out = block<unsigned char>(no), j.res_index_out = block<int>(j.n_res), j.new_res_index_out = block<int>(np), j.last_res_out = block<int>(2 * np);
  j.last_state_out = block<unsigned char>(2 * np), j.n_res_out = block<int>(1), j.n_flagged = block<int>(1), j.dist_score_out = block<double>(n);
  return j;
}
static bool same_core(const dsm_admit_job &a, const dsm_admit_job &b) {
  const size_t n = a.n_frames, m = n + 1, m2 = m * m, np = a.n_pts, no = np + a.n_res;
  return *a.n_flagged == *b.n_flagged && *a.n_res_out == *b.n_res_out && !memcmp(a.world_to_cam_eval_out, b.world_to_cam_eval_out, 56 * m) &&
         !memcmp(a.state_out, b.state_out, 64 * m) && !memcmp(a.flagged_out, b.flagged_out, m) && !memcmp(a.pre_KRKiTll_out, b.pre_KRKiTll_out, 36 * m2) &&
         !memcmp(a.ad_host_out, b.ad_host_out, 512 * m2) && !memcmp(a.ad_target_out, b.ad_target_out, 512 * m2) &&
         !memcmp(a.ad_ht_delta_out, b.ad_ht_delta_out, 32 * m2) && !memcmp(a.delta_x_out, b.delta_x_out, 8 * (12 + 8 * n)) &&
         !memcmp(a.point_out, b.point_out, 4 * no) && !memcmp(a.target_out, b.target_out, 4 * no) && !memcmp(a.last_res_out, b.last_res_out, 8 * np) &&
         !memcmp(a.dist_score_out, b.dist_score_out, 8 * n);
}

int main(int argc, char **argv) {
  FILE *f = argc > 1 ? fopen(argv[1], "rb") : nullptr;
  if (!f) {
    fprintf(stderr, "usage: admit_host_standalone FILE\n");
    return 2;
  }
  const int *head = read_block<int>(f, 5, PROGRAM);
  const float *words = read_block<float>(f, 2, PROGRAM);
  const double *g2l = read_block<double>(f, 2, PROGRAM);
  if (head[0] < 1 || head[0] >= DSM_WINDOW_MAX_FRAMES || head[1] < 0 || head[2] < 0) {
    fprintf(stderr, "admit_host_standalone: n_frames, n_pts or n_res\n");
    return 2;
  }
  const size_t n = head[0], m = n + 1, m2 = m * m, N = 4 + 8 * n, M = N + 8, np = head[1], nr = head[2], no = np + nr;
  const int bits = head[4];
  dsm_admit_job in;
  memset(&in, 0, sizeof in);
  in.n_frames = head[0], in.n_pts = head[1], in.n_res = head[2], in.new_keyframe_id = head[3];
  in.new_exposure = words[0], in.new_frame_energy_th = words[1], in.aff_g2l[0] = g2l[0], in.aff_g2l[1] = g2l[1];
  in.world_to_cam_eval = read_block<double>(f, 7 * n, PROGRAM), in.state = read_block<double>(f, 8 * n, PROGRAM), in.state_zero = read_block<double>(f, 8 * n, PROGRAM);
  in.exposure = read_block<float>(f, n, PROGRAM), in.frame_energy_th = read_block<float>(f, n, PROGRAM);
  in.keyframe_id = read_block<int>(f, n, PROGRAM), in.n_points_in = read_block<int>(f, n, PROGRAM), in.n_points_out = read_block<int>(f, n, PROGRAM);
  in.ref_cam_to_world = read_block<double>(f, 7, PROGRAM), in.cam_to_tracking_ref = read_block<double>(f, 7, PROGRAM);
  in.new_frame_prior = read_block<double>(f, 8, PROGRAM), in.new_frame_prior_zero = read_block<double>(f, 8, PROGRAM);
  in.calib_value = read_block<double>(f, 4, PROGRAM), in.calib_zero = read_block<double>(f, 4, PROGRAM);
  if (bits & 1) in.H_M = read_block<double>(f, N * N, PROGRAM);
  if (bits & 2) in.b_M = read_block<double>(f, N, PROGRAM);
  if (bits & 4) in.H_L = read_block<double>(f, N * N, PROGRAM);
  if (bits & 8) in.b_L = read_block<double>(f, N, PROGRAM);
  if (bits & 16) in.prior = read_block<double>(f, N, PROGRAM), in.prior_zero = read_block<double>(f, N, PROGRAM);
  in.host = read_block<int>(f, np, PROGRAM), in.last_res = read_block<int>(f, 2 * np, PROGRAM), in.last_state = read_block<unsigned char>(f, 2 * np, PROGRAM);
  in.point = read_block<int>(f, nr, PROGRAM), in.target = read_block<int>(f, nr, PROGRAM), in.state_in = read_block<unsigned char>(f, nr, PROGRAM);
  in.energy_in = read_block<float>(f, nr, PROGRAM), in.is_new = read_block<unsigned char>(f, nr, PROGRAM);
  fclose(f);

  dsm_admit_job full = with_outputs(in, true), bare = with_outputs(in, false);
  dsm_linearize_params lp;
  dsm_step_params sp;
  dsm_admit_params ap;
  dsm_linearize_params_default(&lp), dsm_step_params_default(&sp), dsm_admit_params_default(&ap);
  if (dsm_window_admit_host(1, &full, &lp, &sp, &ap) != DSM_OK || dsm_window_admit_host(1, &bare, nullptr, nullptr, nullptr) != DSM_OK) {
    fprintf(stderr, "admit_host_standalone: %s\n", dsm::last_error.c_str());
    return 1;
  }
  dsm_admit_job *two = block<dsm_admit_job>(2);
  two[0] = with_outputs(in, false), two[1] = with_outputs(in, true);
  if (dsm_window_admit_host(2, two, nullptr, nullptr, nullptr) != DSM_OK) return 1;
  const int forms_equal = same_core(full, bare) && same_core(full, two[0]) && same_core(full, two[1]) &&
                          !memcmp(full.distance_ll_out, two[1].distance_ll_out, 4 * m2) && (!full.H_M || !memcmp(full.H_M_out, two[1].H_M_out, 8 * M * M));
  dsm_admit_job refused = with_outputs(in, false); // V: refused before an output is touched
  refused.n_frames = DSM_WINDOW_MAX_FRAMES;
  *refused.n_flagged = 77;
  const int refusal = dsm_window_admit_host(1, &refused, nullptr, nullptr, nullptr) == DSM_ERR_INVALID && *refused.n_flagged == 77;
  const dsm_admit_job &o = full;
  std::string line = "{\"n_res\": " + std::to_string(*o.n_res_out) + ", \"n_flagged\": " + std::to_string(*o.n_flagged);
  auto add = [&line](const char *name, const void *p, size_t bytes) {
    char hex[24] = "-";
    if (p) snprintf(hex, sizeof hex, "%016llx", (unsigned long long)fnv1a(p, bytes));
    line += std::string(", \"") + name + "\": \"" + hex + "\"";
  };
  add("world_to_cam_eval", o.world_to_cam_eval_out, 56 * m), add("state", o.state_out, 64 * m), add("state_zero", o.state_zero_out, 64 * m);
  add("exposure", o.exposure_out, 4 * m), add("frame_energy_th", o.frame_energy_th_out, 4 * m), add("keyframe_id", o.keyframe_id_out, 4 * m);
  add("world_to_cam", o.world_to_cam_out, 56 * m), add("flagged", o.flagged_out, m), add("cam_to_world", o.cam_to_world_out, 56);
  add("pre_RTll_0", o.pre_RTll_0_out, 36 * m2), add("pre_tTll_0", o.pre_tTll_0_out, 12 * m2), add("pre_KRKiTll", o.pre_KRKiTll_out, 36 * m2);
  add("pre_KtTll", o.pre_KtTll_out, 12 * m2), add("pre_aff_mode", o.pre_aff_mode_out, 8 * m2), add("pre_b0_mode", o.pre_b0_mode_out, 4 * m2);
  add("distance_ll", o.distance_ll_out, 4 * m2), add("cam", o.cam_out, 24), add("c_delta", o.c_delta_out, 16), add("delta_x", o.delta_x_out, 8 * M);
  add("ad_host", o.ad_host_out, 512 * m2), add("ad_target", o.ad_target_out, 512 * m2), add("ad_ht_delta", o.ad_ht_delta_out, 32 * m2);
  add("H_M", o.H_M_out, 8 * M * M), add("b_M", o.b_M_out, 8 * M), add("H_L", o.H_L_out, 8 * M * M), add("b_L", o.b_L_out, 8 * M);
  add("prior", o.prior_out, 8 * M), add("prior_zero", o.prior_zero_out, 8 * M), add("frame_prior", o.frame_prior_out, 64);
  add("frame_delta_prior", o.frame_delta_prior_out, 64), add("point", o.point_out, 4 * no), add("target", o.target_out, 4 * no);
  add("res_state", o.res_state_out, no), add("energy", o.energy_out, 4 * no), add("is_new", o.is_new_out, no), add("res_index", o.res_index_out, 4 * nr);
  add("new_res_index", o.new_res_index_out, 4 * np), add("last_res", o.last_res_out, 8 * np), add("last_state", o.last_state_out, 2 * np);
  add("dist_score", o.dist_score_out, 8 * n);
  printf("%s, \"forms_equal\": %d, \"refusal\": %d}\n", line.c_str(), forms_equal, refusal);
  return forms_equal && refusal ? 0 : 1;
}
