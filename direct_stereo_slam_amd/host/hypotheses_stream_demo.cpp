// hypotheses_stream_demo.cpp -- the hypothesis loop of FrontEnd::trackNewCoarse (FrontEnd.cpp:194-256) through dsm_host::Stream::submitHypotheses,
// against dsm_host::trackHypotheses on the same tracker and frame.  Inputs: the fixture of host_adaptor_demo.cpp (written by
// tests/test_host_adaptor.py's write_fixture) and a file with the hypothesis list: int32 n ; n x 7 doubles (qx qy qz qw tx ty tz).
// Prints one JSON line: trackHypotheses' result, and per (engine, window) whether the stream's group gave the same one field for field.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "TrackerAndScaler.hpp"

template <typename T>
static void rd(FILE *f, T *p, size_t n) {
  if (fread(p, sizeof(T), n, f) != n) {
    fprintf(stderr, "short read\n");
    exit(2);
  }
}

static bool same_double(double a, double b) { return (std::isnan(a) && std::isnan(b)) || memcmp(&a, &b, sizeof a) == 0; }

static bool same_result(const dsm_host::HypothesesResult &a, const dsm_host::HypothesesResult &b) {
  bool eq = a.haveOneGood == b.haveOneGood && a.triesUsed == b.triesUsed && same_double(a.aff_g2l.a, b.aff_g2l.a) && same_double(a.aff_g2l.b, b.aff_g2l.b);
  for (int k = 0; k < 4; k++) eq = eq && same_double(a.lastF_2_fh.q[k], b.lastF_2_fh.q[k]);
  for (int k = 0; k < 3; k++) eq = eq && same_double(a.lastF_2_fh.t[k], b.lastF_2_fh.t[k]) && same_double(a.flowVecs[k], b.flowVecs[k]);
  for (int l = 0; l < 5; l++) eq = eq && same_double(a.achievedRes[l], b.achievedRes[l]);
  return eq;
}

int main(int argc, char **argv) {
  if (argc < 4) {
    fprintf(stderr, "usage: %s fixture.bin tries.bin last_coarse_rmse0\n", argv[0]);
    return 2;
  }
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  int w, h, nl;
  rd(f, &w, 1);
  rd(f, &h, 1);
  rd(f, &nl, 1);
  float K[4];
  rd(f, K, 4);
  std::vector<double> T(16);
  rd(f, T.data(), 16);
  std::vector<std::vector<float>> u(nl), v(nl), id(nl), c(nl), newp(nl);
  dsm_host::TemplateLists tpl;
  for (int l = 0; l < nl; l++) {
    int n;
    rd(f, &n, 1);
    u[l].resize(n), v[l].resize(n), id[l].resize(n), c[l].resize(n);
    rd(f, u[l].data(), n), rd(f, v[l].data(), n), rd(f, id[l].data(), n), rd(f, c[l].data(), n);
    tpl.n[l] = n;
    tpl.pc_u[l] = u[l].data(), tpl.pc_v[l] = v[l].data(), tpl.pc_idepth[l] = id[l].data(), tpl.pc_color[l] = c[l].data();
  }
  std::vector<const float *> newptr(nl);
  for (int l = 0; l < nl; l++) {
    newp[l].resize(3 * (size_t)(w >> l) * (h >> l));
    rd(f, newp[l].data(), newp[l].size());
    newptr[l] = newp[l].data();
  }
  fclose(f);
  FILE *ft = fopen(argv[2], "rb");
  if (!ft) return 2;
  int n_tries = 0;
  rd(ft, &n_tries, 1);
  std::vector<dsm_host::SE3> tries((size_t)n_tries);
  for (dsm_host::SE3 &p : tries) rd(ft, p.q, 4), rd(ft, p.t, 3);
  fclose(ft);
  const double last_rmse0 = atof(argv[3]);

  dsm_context *ctx = nullptr;
  if (dsm_context_create(0, &ctx) != DSM_OK) {
    fprintf(stderr, "no device: %s\n", dsm_last_error());
    return 3;
  }
  {
    dsm_host::TrackerAndScaler tracker(ctx, w, h, nl, T, K);
    tracker.makeK(K[0], K[1], K[2], K[3]);
    dsm_host::FrameView ref, nf;
    ref.shell_id = 7;
    nf.dIp = newptr.data(), nf.unique_id = 1;
    tracker.setCoarseTrackingRef(ref, tpl);
    const dsm_host::AffLight aff0;
    // the synchronous form (try 0 alone, the rest as one batch); it leaves the frame resident in the tracker's NEW_LEFT slot
    const dsm_host::HypothesesResult R = dsm_host::trackHypotheses(ctx, tracker, nf, tries, aff0, nl - 1, last_rmse0);
    printf("{\"have\": %d, \"tries_used\": %d, \"n_tries\": %d, \"pose\": [%.17g, %.17g, %.17g, %.17g, %.17g, %.17g, %.17g], \"groups\": [", R.haveOneGood ? 1 : 0,
           R.triesUsed, n_tries, R.lastF_2_fh.q[0], R.lastF_2_fh.q[1], R.lastF_2_fh.q[2], R.lastF_2_fh.q[3], R.lastF_2_fh.t[0], R.lastF_2_fh.t[1], R.lastF_2_fh.t[2]);
    const int windows[3] = {0, 1, 8};
    bool first = true;
    for (int engine = 0; engine < 2; engine++)
      for (int wi = 0; wi < 3; wi++) {
        dsm_host::Stream stream(ctx, 4, 0);
        dsm_host::check(dsm_stream_set_engine(stream.handle(), engine, 0), "dsm_stream_set_engine");
        stream.setHypothesisWindow(windows[wi]);
        const uint64_t tk = stream.submitHypotheses(tracker, tries, aff0, nl - 1, last_rmse0);
        stream.drain();
        std::vector<std::pair<uint64_t, dsm_host::HypothesesResult>> got;
        stream.hypothesesResults(got);
        const bool equal = got.size() == 1 && got[0].first == tk && same_result(got[0].second, R);
        printf("%s{\"engine\": %d, \"window\": %d, \"equal\": %d, \"tries_run\": %d}", first ? "" : ", ", engine, windows[wi], equal ? 1 : 0,
               got.empty() ? -1 : got[0].second.triesRun);
        first = false;
      }
    printf("]}\n");
  }
  dsm_context_destroy(ctx);
  return 0;
}
