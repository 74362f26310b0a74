// trace_host_standalone.cpp -- dsm_trace_points_host as a stand-alone CPU program, for a sanitizer run of the host form
// (DESIGN.md section 14): reads a sequence file in the format of host/trace_new_coarse_demo.cpp, puts the image and every array into
// heap blocks of exactly their size, traces the points against the first frame with the default settings (or with max_pix_search
// given as the second argument) and prints one JSON line: the statuses as a digit string, the steps summed and the FNV-1a hash of the
// traced floats (NaNs made canonical), which tests/_trace_ref.py can reproduce.  Build, from the repository root:
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       tools/trace_host_standalone.cpp direct_stereo_slam_amd/csrc/points_host.cpp -o trace_host_standalone
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#define WINDOW_CASE_STANDALONE
#include "../direct_stereo_slam_amd/host/window_case.hpp" // block, fnv1a and the dsm::set_error stub

using window_case::block;

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = fopen(argv[1], "rb");
  int hd[5];
  if (!f || fread(hd, sizeof(int), 5, f) != 5) return 2;
  const int w = hd[0], h = hd[1], n_frames = hd[2], nh = hd[3], n = hd[4];
  const size_t npx = (size_t)w * h;
  float *plane = block<float>(npx), *hosts = block<float>((size_t)nh * 14);
  int32_t *rec = block<int32_t>((size_t)n * 32);
  bool good = fread(plane, 4, npx, f) == npx && fseek(f, (long)((n_frames - 1) * npx * 4), SEEK_CUR) == 0 &&
              fread(hosts, 4, (size_t)nh * 14, f) == (size_t)nh * 14 && fread(rec, 4, (size_t)n * 32, f) == (size_t)n * 32;
  if (!good) return 2;
  fclose(f);
  float *krki = block<float>(9 * nh), *kt = block<float>(3 * nh), *aff = block<float>(2 * nh);
  for (int k = 0; k < nh; k++) memcpy(krki + 9 * k, hosts + 14 * k, 36), memcpy(kt + 3 * k, hosts + 14 * k + 9, 12), memcpy(aff + 2 * k, hosts + 14 * k + 12, 8);
  int *host = block<int>(n), *steps = block<int>(n), *counts = block<int>(6);
  unsigned char *status = block<unsigned char>(n);
  float *u = block<float>(n), *v = block<float>(n), *eth = block<float>(n), *G = block<float>(4 * (size_t)n), *color = block<float>(8 * (size_t)n),
        *wt = block<float>(8 * (size_t)n), *dmin = block<float>(n), *dmax = block<float>(n), *quality = block<float>(n), *uv = block<float>(2 * (size_t)n),
        *interval = block<float>(n);
  for (int i = 0; i < n; i++) {
    const int32_t *q = rec + (size_t)32 * i;
    float x[30];
    memcpy(x, q + 2, sizeof x);
    host[i] = q[0], status[i] = (unsigned char)q[1], u[i] = x[0], v[i] = x[1], eth[i] = x[2];
    memcpy(G + 4 * i, x + 3, 16), memcpy(color + 8 * i, x + 7, 32), memcpy(wt + 8 * i, x + 15, 32);
    dmin[i] = x[23], dmax[i] = x[24], quality[i] = x[25], uv[2 * i] = x[26], uv[2 * i + 1] = x[27], interval[i] = x[28];
  }
  dsm_trace_job J;
  memset(&J, 0, sizeof J);
  J.n_hosts = nh, J.krki = krki, J.kt = kt, J.aff = aff, J.n_pts = n, J.host = host, J.u = u, J.v = v, J.energy_th = eth, J.grad_h = G;
  J.color = color, J.weights = wt, J.status = status, J.idepth_min = dmin, J.idepth_max = dmax, J.quality = quality, J.trace_uv = uv;
  J.trace_interval = interval, J.steps_out = steps, J.counts_out = counts;
  dsm_trace_params P;
  dsm_trace_params_default(&P);
  if (argc > 2) P.max_pix_search = (float)atof(argv[2]);
  const int rc = dsm_trace_points_host(w, h, plane, &J, &P);
  if (rc) {
    fprintf(stderr, "dsm_trace_points_host: %d %s\n", rc, dsm::last_error.c_str());
    return 1;
  }
  uint64_t hsh = 1469598103934665603ull;
  long long total = 0;
  std::string st;
  for (int i = 0; i < n; i++) {
    const float x[6] = {dmin[i], dmax[i], quality[i], uv[2 * i], uv[2 * i + 1], interval[i]};
    for (float y : x) {
      uint32_t b;
      memcpy(&b, &y, 4);
      if (y != y) b = 0x7fc00000u;
      for (int k = 0; k < 4; k++) hsh = (hsh ^ ((b >> (8 * k)) & 0xffu)) * 1099511628211ull;
    }
    st += (char)('0' + status[i]), total += steps[i];
  }
  printf("{\"statuses\": \"%s\", \"steps\": %lld, \"hash\": \"%016llx\"}\n", st.c_str(), total, (unsigned long long)hsh);
  for (void *p : {(void *)plane, (void *)hosts, (void *)rec, (void *)krki, (void *)kt, (void *)aff, (void *)host, (void *)steps, (void *)counts,
                  (void *)status, (void *)u, (void *)v, (void *)eth, (void *)G, (void *)color, (void *)wt, (void *)dmin, (void *)dmax, (void *)quality,
                  (void *)uv, (void *)interval})
    free(p);
  return 0;
}
