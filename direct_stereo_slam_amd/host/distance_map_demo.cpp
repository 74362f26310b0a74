// distance_map_demo.cpp -- the distance-map part of FrontEnd::activatePointsMT (FrontEnd.cpp:371-451) through the C++ adaptor
// host/CoarseDistanceMap.hpp, on a window read from a file: first the way the reference runs it (makeK, makeDistanceMap, then the
// walk of :431-449 on the host mirror with one addIntoDistFinal per activation), then the same window through activatePoints (one
// batched call), which must give the same decisions and the same map.
// Input file (native byte order): int32 w, h; float fx, fy, cx, cy, min_act_dist; int32 n_hosts, per host 9 floats R (row-major) and 3
// floats t; int32 n_points, then host[int32], u, v, idepth arrays; int32 n_cand, then host[int32], u, v, idepth_min, idepth_max, my_type.
// Usage: distance_map_demo FILE.  Prints one JSON line: the decisions as a digit string, their count of 1s, the FNV-1a hash of the
// final map's float bytes, and whether the batched call agreed; exit status 0 when it did.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "CoarseDistanceMap.hpp"
#include "window_case.hpp" // fnv1a, rd

using namespace dsm_host;
using window_case::fnv1a;
using window_case::rd;

int main(int argc, char **argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: distance_map_demo FILE\n");
    return 2;
  }
  FILE *f = fopen(argv[1], "rb");
  int wh[2], n_hosts = 0, n_points = 0, n_cand = 0;
  float cal[5];
  std::vector<float> hr, pu, pv, pd, cu, cv, cmin, cmax, ct;
  std::vector<int> ph, ch;
  bool good = f && fread(wh, sizeof(int), 2, f) == 2 && fread(cal, sizeof(float), 5, f) == 5 && fread(&n_hosts, sizeof(int), 1, f) == 1 &&
              n_hosts >= 0 && rd(f, hr, (size_t)12 * n_hosts);
  good = good && fread(&n_points, sizeof(int), 1, f) == 1 && n_points >= 0 && rd(f, ph, n_points) && rd(f, pu, n_points) && rd(f, pv, n_points) &&
         rd(f, pd, n_points);
  good = good && fread(&n_cand, sizeof(int), 1, f) == 1 && n_cand >= 0 && rd(f, ch, n_cand) && rd(f, cu, n_cand) && rd(f, cv, n_cand) &&
         rd(f, cmin, n_cand) && rd(f, cmax, n_cand) && rd(f, ct, n_cand);
  if (!good) {
    fprintf(stderr, "distance_map_demo: cannot read %s\n", argv[1]);
    return 2;
  }
  fclose(f);
  std::vector<DistMapHost> hosts(n_hosts);
  for (int i = 0; i < n_hosts; i++) {
    memcpy(hosts[i].R.m, &hr[12 * i], 9 * sizeof(float));
    memcpy(hosts[i].t, &hr[12 * i + 9], 3 * sizeof(float));
  }
  std::vector<DistMapPoint> points(n_points);
  for (int i = 0; i < n_points; i++) points[i] = DistMapPoint{ph[i], pu[i], pv[i], pd[i]};
  std::vector<ImmatureCandidate> cands(n_cand);
  for (int i = 0; i < n_cand; i++) cands[i] = ImmatureCandidate{ch[i], cu[i], cv[i], cmin[i], cmax[i], ct[i]};
  const float current_min_act_dist = cal[4];

  dsm_context *ctx = nullptr;
  distmap_check(dsm_context_create(0, &ctx), "dsm_context_create");
  std::string decisions;
  uint64_t hash_walk = 0, hash_batch = 0;
  int n_act = 0, batched_equal = 0;
  {
    // the reference's sequence: FrontEnd.cpp:374-375, then :382-451 with the deletions reduced to decision 2
    CoarseDistanceMap coarse_distance_map(ctx, wh[0], wh[1]);
    coarse_distance_map.addIntoDistFinal(1, 1); // before makeK: a no-op (:1327)
    coarse_distance_map.makeK(cal[0], cal[1], cal[2], cal[3]);
    coarse_distance_map.makeDistanceMap(hosts, points);
    const int wG1 = coarse_distance_map.w1(), hG1 = coarse_distance_map.h1();
    for (const ImmatureCandidate &ph_ : cands) {
      float KRKi[9], Kt[3];
      coarse_distance_map.krki_of(hosts[ph_.host], KRKi, Kt);
      const float id = 0.5f * (ph_.idepth_max + ph_.idepth_min);
      float ptp[3];
      for (int r = 0; r < 3; r++) ptp[r] = ((KRKi[3 * r] * ph_.u + KRKi[3 * r + 1] * ph_.v) + KRKi[3 * r + 2]) + Kt[r] * id;
      const float qu = ptp[0] / ptp[2] + 0.5f, qv = ptp[1] / ptp[2] + 0.5f;
      if (qu >= 1.0f && qv >= 1.0f && qu < (float)wG1 && qv < (float)hG1) {
        const int u = (int)qu, v = (int)qv;
        const float dist = coarse_distance_map.fwdWarpedIDDistFinal[u + wG1 * v] + (ptp[0] - floorf((float)(ptp[0])));
        if (dist >= current_min_act_dist * ph_.my_type) {
          coarse_distance_map.addIntoDistFinal(u, v);
          decisions += '1';
          n_act++;
        } else {
          decisions += '0';
        }
      } else {
        decisions += '2';
      }
    }
    hash_walk = fnv1a(coarse_distance_map.fwdWarpedIDDistFinal, sizeof(float) * wG1 * hG1);

    // the same window twice in one batched call
    CoarseDistanceMap m1(ctx, wh[0], wh[1]), m2(ctx, wh[0], wh[1]);
    m1.makeK(cal[0], cal[1], cal[2], cal[3]);
    m2.makeK(cal[0], cal[1], cal[2], cal[3]);
    std::vector<ActivationRequest> reqs(2);
    for (int i = 0; i < 2; i++) {
      reqs[i].map = i ? &m2 : &m1;
      reqs[i].hosts = &hosts, reqs[i].points = &points, reqs[i].candidates = &cands, reqs[i].min_act_dist = current_min_act_dist;
    }
    activatePoints(ctx, reqs);
    hash_batch = fnv1a(m1.fwdWarpedIDDistFinal, sizeof(float) * wG1 * hG1);
    batched_equal = hash_batch == hash_walk && fnv1a(m2.fwdWarpedIDDistFinal, sizeof(float) * wG1 * hG1) == hash_walk;
    for (int i = 0; i < 2; i++) {
      std::string d;
      for (unsigned char c : reqs[i].decisions) d += (char)('0' + c);
      batched_equal = batched_equal && d == decisions && reqs[i].n_activated == n_act;
    }
  }
  dsm_context_destroy(ctx);
  printf("{\"n_cand\": %d, \"n_activated\": %d, \"decisions\": \"%s\", \"map_hash\": \"%016llx\", \"batched_equal\": %d}\n", n_cand, n_act,
         decisions.c_str(), (unsigned long long)hash_walk, batched_equal);
  return batched_equal ? 0 : 1;
}
