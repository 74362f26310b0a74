// icp_demo.cpp -- the ICP fallback of loop closure through the C++ adaptor: every match of a file through dsm_host::icp() alone, then all
// of them in one dsm_host::icp_many call, which must give the same bits.  Input file (native byte order): int32 n, then per match int32
// n_src, int32 n_tgt, 16 doubles of the guess (row-major), n_src x 3 doubles of pts_source, n_tgt x 3 doubles of pts_target.
// Usage: icp_demo FILE.  Prints one line per match and a summary line; exit status 0 when icp_many matched icp() everywhere.
#include <cstdio>
#include <cstring>
#include <vector>

#include "LoopDetection.hpp"

int main(int argc, char **argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: icp_demo FILE\n");
    return 2;
  }
  FILE *f = fopen(argv[1], "rb");
  int n = 0;
  if (!f || fread(&n, sizeof n, 1, f) != 1 || n < 1) {
    fprintf(stderr, "icp_demo: cannot read %s\n", argv[1]);
    return 2;
  }
  std::vector<std::vector<double>> src(n), tgt(n);
  std::vector<dsm_host::IcpMatch> many(n);
  for (int j = 0; j < n; j++) {
    int ns = 0, nt = 0;
    bool good = fread(&ns, sizeof ns, 1, f) == 1 && fread(&nt, sizeof nt, 1, f) == 1 && ns >= 0 && nt >= 0;
    good = good && fread(many[j].tfm_target_source, sizeof(double), 16, f) == 16;
    src[j].resize((size_t)3 * ns), tgt[j].resize((size_t)3 * nt);
    good = good && fread(src[j].data(), sizeof(double), src[j].size(), f) == src[j].size();
    good = good && fread(tgt[j].data(), sizeof(double), tgt[j].size(), f) == tgt[j].size();
    if (!good) {
      fprintf(stderr, "icp_demo: short file\n");
      return 2;
    }
    many[j].pts_source = &src[j], many[j].pts_target = &tgt[j];
  }
  fclose(f);
  dsm_context *ctx = nullptr;
  dsm_host::loop_check(dsm_context_create(0, &ctx), "dsm_context_create");
  int mismatches = 0;
  {
    std::vector<dsm_host::IcpMatch> alone = many;
    for (int j = 0; j < n; j++) {
      dsm_host::IcpMatch &a = alone[j];
      a.ok = dsm_host::icp(ctx, *a.pts_source, *a.pts_target, a.tfm_target_source, a.icp_score);
    }
    dsm_host::icp_many(ctx, many);
    for (int j = 0; j < n; j++) {
      const dsm_host::IcpMatch &a = alone[j], &m = many[j];
      if (a.ok != m.ok || memcmp(&a.icp_score, &m.icp_score, sizeof(float)) || memcmp(a.tfm_target_source, m.tfm_target_source, sizeof(double) * 16))
        mismatches++;
      printf("match %d ok=%d state=%d iterations=%d score=%.9g tfm=", j, (int)m.ok, m.state, m.iterations, (double)m.icp_score);
      for (int e = 0; e < 16; e++) printf("%.17g%c", m.tfm_target_source[e], e < 15 ? ',' : '\n');
    }
  }
  dsm_context_destroy(ctx);
  printf("matches=%d mismatches=%d\n", n, mismatches);
  return mismatches == 0 ? 0 : 1;
}
