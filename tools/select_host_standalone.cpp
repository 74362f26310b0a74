// select_host_standalone.cpp -- dsm_select_pixels_host as a stand-alone CPU program, for a sanitizer run of the host form (DESIGN.md
// section 15): reads a scene file written by tests/_select_ref.py dump_scene() -- int32 w, h, then the float planes of levels 0, 1, 2
// and the w * h bytes of the random pattern -- puts every plane and every array into a heap block of exactly its size, selects with
// the default settings at the potential and density given as the second and third argument (recursions as the fourth) and prints one
// JSON line: the counts, and the FNV-1a hashes of the map and of the point floats (NaNs made canonical), which tests/_select_ref.py
// fingerprint() reproduces.  Build, from the repository root:
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       tools/select_host_standalone.cpp direct_stereo_slam_amd/csrc/points_host.cpp -o select_host_standalone
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#define WINDOW_CASE_STANDALONE
#include "../direct_stereo_slam_amd/host/window_case.hpp" // block, fnv1a and the dsm::set_error stub

using window_case::block;
using window_case::fnv1a;

static uint64_t hash_floats(uint64_t h, const float *x, size_t n) {
  for (size_t i = 0; i < n; i++) {
    uint32_t b;
    memcpy(&b, x + i, 4);
    if (x[i] != x[i]) b = 0x7fc00000u;
    h = fnv1a(&b, 4, h);
  }
  return h;
}

int main(int argc, char **argv) {
  if (argc < 4) return 2;
  FILE *f = fopen(argv[1], "rb");
  int hd[2];
  if (!f || fread(hd, sizeof(int), 2, f) != 2) return 2;
  const int w = hd[0], h = hd[1];
  if (w < 1 || h < 1 || w > 4096 || h > 4096) return 2;
  const size_t npx = (size_t)w * h, n1 = (size_t)(w >> 1) * (h >> 1), n2 = (size_t)(w >> 2) * (h >> 2);
  float *I0 = block<float>(npx), *I1 = block<float>(n1), *I2 = block<float>(n2);
  unsigned char *rp = block<unsigned char>(npx), *map = block<unsigned char>(npx);
  if (fread(I0, 4, npx, f) != npx || fread(I1, 4, n1, f) != n1 || fread(I2, 4, n2, f) != n2 || fread(rp, 1, npx, f) != npx) return 2;
  fclose(f);
  const size_t cap = 1500;
  float *u = block<float>(cap), *v = block<float>(cap), *eth = block<float>(cap), *G = block<float>(4 * cap), *color = block<float>(8 * cap),
        *wt = block<float>(8 * cap), *dmin = block<float>(cap), *dmax = block<float>(cap), *quality = block<float>(cap), *type = block<float>(cap);
  unsigned char *status = block<unsigned char>(cap);
  int *potential = block<int>(1), *n_pts = block<int>(1), *num_total = block<int>(1), *counts = block<int>(3), *passes = block<int>(1);
  *potential = atoi(argv[2]);
  dsm_select_job J;
  memset(&J, 0, sizeof J);
  J.density = (float)atof(argv[3]), J.potential_io = potential, J.max_pts = (int)cap, J.u = u, J.v = v, J.energy_th = eth, J.grad_h = G;
  J.color = color, J.weights = wt, J.status = status, J.idepth_min = dmin, J.idepth_max = dmax, J.quality = quality, J.type = type;
  J.n_pts_out = n_pts, J.num_total_out = num_total, J.counts_out = counts, J.passes_out = passes, J.map_out = map;
  dsm_select_params P;
  dsm_select_params_default(&P);
  if (argc > 4) P.recursions = atoi(argv[4]);
  const int rc = dsm_select_pixels_host(w, h, I0, I1, I2, rp, &J, &P);
  if (rc) {
    fprintf(stderr, "dsm_select_pixels_host: %d %s\n", rc, dsm::last_error.c_str());
    return 1;
  }
  const size_t n = (size_t)(*n_pts < (int)cap ? *n_pts : (int)cap);
  uint64_t hp = 1469598103934665603ull;
  hp = hash_floats(hp, u, n), hp = hash_floats(hp, v, n), hp = hash_floats(hp, eth, n), hp = hash_floats(hp, G, 4 * n), hp = hash_floats(hp, color, 8 * n);
  hp = hash_floats(hp, wt, 8 * n), hp = hash_floats(hp, dmin, n), hp = hash_floats(hp, dmax, n), hp = hash_floats(hp, quality, n), hp = hash_floats(hp, type, n);
  hp = fnv1a(status, n, hp);
  printf("{\"counts\": [%d, %d, %d], \"n_pts\": %d, \"num_total\": %d, \"passes\": %d, \"potential\": %d, \"map_hash\": \"%016llx\", \"points_hash\": \"%016llx\"}\n",
         counts[0], counts[1], counts[2], *n_pts, *num_total, *passes, *potential, (unsigned long long)fnv1a(map, npx),
         (unsigned long long)hp);
  for (void *p : {(void *)I0, (void *)I1, (void *)I2, (void *)rp, (void *)map, (void *)u, (void *)v, (void *)eth, (void *)G, (void *)color, (void *)wt,
                  (void *)dmin, (void *)dmax, (void *)quality, (void *)type, (void *)status, (void *)potential, (void *)n_pts, (void *)num_total,
                  (void *)counts, (void *)passes})
    free(p);
  return 0;
}
