// nullspace_host_standalone.cpp -- dsm_window_nullspace_host as a stand-alone CPU program, for a sanitizer run of the host form
// (DESIGN.md section 23): reads a case file (int32 n_frames, int32 given, n_frames * 7 doubles world_to_cam_eval, n_frames * 8 state_zero,
// n_frames floats exposure, and if given n_frames * 42 doubles frame_null_in), puts every array into a heap block of exactly its size,
// runs the job once with every optional output and once with none, then twice in one call, and prints one JSON line with the FNV-1a
// hashes of every output, which tests/_nullspace_ref.py's hashes reproduces from the checker (tools/host_standalone_check.py).  Build, from the repository root:
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       tools/nullspace_host_standalone.cpp direct_stereo_slam_amd/csrc/nullspace_host.cpp -o nullspace_host_standalone
// The program frees none of its blocks: run it with ASAN_OPTIONS=detect_leaks=0.
#define WINDOW_CASE_STANDALONE
#include "../direct_stereo_slam_amd/host/window_case.hpp" // block, read_block, fnv1a and the dsm::set_error / dsm::invalid stubs

using window_case::block;
using window_case::fnv1a;
static const char *const PROGRAM = "nullspace_host_standalone";

static dsm_nullspace_job make_job(int n, const double *ev, const double *zero, const float *expo, const double *fn, bool optional) {
  const size_t N = 4 + 8 * (size_t)n;
  dsm_nullspace_job j;
  memset(&j, 0, sizeof j);
  j.n_frames = n, j.world_to_cam_eval = ev, j.state_zero = zero, j.exposure = expo, j.frame_null_in = fn;
  j.null_basis = block<double>(7 * N), j.null_pinv = block<double>(7 * N), j.sing = block<double>(7), j.rank = block<int>(1), j.flags = block<int>(1);
  if (optional) j.frame_null_out = block<double>(42 * (size_t)n), j.null_x0_pre = block<double>(9 * N);
  return j;
}
static bool same_core(const dsm_nullspace_job &a, const dsm_nullspace_job &b) {
  const size_t N = 4 + 8 * (size_t)a.n_frames;
  return !memcmp(a.null_basis, b.null_basis, 56 * N) && !memcmp(a.null_pinv, b.null_pinv, 56 * N) && !memcmp(a.sing, b.sing, 56) && *a.rank == *b.rank &&
         *a.flags == *b.flags;
}

int main(int argc, char **argv) {
  FILE *f = argc > 1 ? fopen(argv[1], "rb") : nullptr;
  if (!f) {
    fprintf(stderr, "usage: nullspace_host_standalone FILE\n");
    return 2;
  }
  int *head = window_case::read_block<int>(f, 2, PROGRAM);
  const int n = head[0];
  if (n < 1 || n > DSM_WINDOW_MAX_FRAMES) {
    fprintf(stderr, "nullspace_host_standalone: n_frames\n");
    return 2;
  }
  const size_t N = 4 + 8 * (size_t)n;
  double *ev = window_case::read_block<double>(f, 7 * (size_t)n, PROGRAM), *zero = window_case::read_block<double>(f, 8 * (size_t)n, PROGRAM);
  float *expo = window_case::read_block<float>(f, n, PROGRAM);
  double *fn = head[1] ? window_case::read_block<double>(f, 42 * (size_t)n, PROGRAM) : nullptr;
  fclose(f);

  dsm_nullspace_job full = make_job(n, ev, zero, expo, fn, true), bare = make_job(n, ev, zero, expo, fn, false);
  dsm_nullspace_params P;
  dsm_nullspace_params_default(&P);
  if (dsm_window_nullspace_host(1, &full, &P) != DSM_OK || dsm_window_nullspace_host(1, &bare, nullptr) != DSM_OK) {
    fprintf(stderr, "nullspace_host_standalone: %s\n", dsm::last_error.c_str());
    return 1;
  }
  dsm_nullspace_job *two = block<dsm_nullspace_job>(2);
  two[0] = make_job(n, ev, zero, expo, fn, false), two[1] = make_job(n, ev, zero, expo, fn, true);
  if (dsm_window_nullspace_host(2, two, nullptr) != DSM_OK) return 1;
  const int forms_equal = same_core(full, bare) && same_core(full, two[0]) && same_core(full, two[1]) &&
                          !memcmp(full.null_x0_pre, two[1].null_x0_pre, 72 * N);
  dsm_nullspace_job refused = make_job(n, ev, zero, expo, fn, false); // V: refused before an output is touched
  refused.n_frames = DSM_WINDOW_MAX_FRAMES + 1;
  const int refusal = dsm_window_nullspace_host(1, &refused, nullptr) == DSM_ERR_INVALID;
  printf("{\"null_basis\": \"%016llx\", \"null_pinv\": \"%016llx\", \"sing\": \"%016llx\", \"frame_null\": \"%016llx\", \"null_x0_pre\": \"%016llx\", "
         "\"rank\": %d, \"flags\": %d, \"forms_equal\": %d, \"refusal\": %d}\n",
         (unsigned long long)fnv1a(full.null_basis, 56 * N), (unsigned long long)fnv1a(full.null_pinv, 56 * N), (unsigned long long)fnv1a(full.sing, 56),
         (unsigned long long)fnv1a(full.frame_null_out, 336 * (size_t)n), (unsigned long long)fnv1a(full.null_x0_pre, 72 * N), *full.rank, *full.flags,
         forms_equal, refusal);
  return forms_equal && refusal ? 0 : 1;
}
