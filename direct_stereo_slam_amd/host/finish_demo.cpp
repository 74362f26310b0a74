// finish_demo.cpp -- the chain of two keyframes as FrontEnd::makeKeyFrame runs it, through the C++ adaptors host/WindowFinish.hpp and
// host/WindowMarginalize.hpp, once through the device forms and once through the host forms:
//   (1) WindowFinish::finishWindow: optimize's loop and, in the same call, setEvalPT, setAdjointsF, the final linearizeAll(true) with
//       its bookkeeping and removeOutliers; shrink() erases what did not survive;
//   (2) MarginalizeRequest::fromFinished on it; frame 1 flagged and marginalised (the frame's prior 100 (k + 1), its delta prior
//       0.001 (k + 1));
//   (3) the window shrunk as host/marginalize_demo.cpp does (window_case::shrink_window) -- the frame dropped, the points of verdict 0 kept with their residuals
//       against the frames that stay, H_L / b_L, the priors, the states and adHost / adTarget cut to those frames -- with the points'
//       counters, last residuals and last states carried over;
//   (4) finishWindow again, on the returned prior.
// Input: a finish file (window_case.hpp, kind FINISH; tests/_finish_ref.py writes the checker's scenes).
// Usage: finish_demo FINISH_FILE [MAX_ITERATIONS = 6].  Prints one JSON line: per form the two patterns, the counts, and the FNV-1a hashes
// of both finishes' decisions and of the marginalisation's verdicts and prior; the second finish's state, energies and rmse.
// Exit status 0 when both forms took the same decisions.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "window_case_requests.hpp"

using namespace dsm_host;
using window_case::fnv1a;
using window_case::vhash;

struct StepCase {
  window_case::Case file;
  std::vector<ActivePointData> points;
  WindowFinish proto; // with the finish's per-point inputs
};

static bool load_step(const char *path, StepCase &c) {
  if (!window_case::read_case(path, window_case::FINISH, c.file)) return false;
  c.points = window_case::points(c.file);
  window_case::fill(c.proto, c.file);
  return true;
}

// what a finish decided, on the lists as they were before shrink()
struct Decisions {
  uint64_t keep = 0, states = 0, n_good = 0, last_res = 0, last_state = 0, dropped = 0, res_index = 0, point_index = 0;
  int residuals = 0, points = 0, lost = 0;
  bool operator==(const Decisions &o) const {
    return keep == o.keep && states == o.states && n_good == o.n_good && last_res == o.last_res && last_state == o.last_state && dropped == o.dropped &&
           res_index == o.res_index && point_index == o.point_index && residuals == o.residuals && points == o.points && lost == o.lost;
  }
};
static Decisions decisions(const WindowFinish &f, const FinishResult &r) {
  Decisions d;
  std::vector<unsigned char> states;
  for (const ActiveResidualData &q : f.optimizer.window.residuals) states.push_back((unsigned char)q.state_state);
  d.keep = vhash(f.keep), d.states = vhash(states), d.n_good = vhash(f.numGoodResiduals), d.last_res = vhash(f.lastResiduals);
  d.last_state = vhash(f.lastResidualStates), d.dropped = vhash(f.pointDropped), d.res_index = vhash(f.resIndex), d.point_index = vhash(f.pointIndex);
  d.residuals = r.residuals, d.points = r.points, d.lost = r.lost;
  return d;
}

struct Chain {
  std::string first, second; // the accept / reject patterns of the two optimisations
  Decisions one, two;
  uint64_t verdict = 0, HM = 0, bM = 0, ad_ht_delta = 0, state = 0, state_zero = 0, eval = 0, calib = 0, idepth = 0;
  int resInM = 0, kept = 0, residuals = 0;
  double last = 0, energy = 0;
  float rmse = 0;
};

// device: through the device forms; otherwise through the host forms (the requests still name a window; the host forms do not read it)
static Chain chain(const StepCase &S, dsm_context *ctx, bool device, int max_its) {
  Chain out;
  const window_case::Case &F = S.file;
  const size_t nf = F.nf;
  const int leaves = nf > 1 ? 1 : 0;
  KeyframeWindow kw(ctx, F.w, F.h, (int)nf);
  window_case::put_planes(F, kw);
  const std::vector<const float *> planes = window_case::planes(F);
  WindowFinish f = S.proto; // (1) the first keyframe's optimize, whole
  f.points = S.points;
  f.optimizer.maxIterations = max_its;
  f.optimizer.window.req.hes.lin.window = &kw;
  const FinishResult r1 = device ? f.finishWindow(ctx) : f.finishWindowHost(F.w, F.h, planes.data());
  out.first = r1.loop.pattern, out.one = decisions(f, r1);
  f.shrink();

  MarginalizeRequest m; // (2) what makeKeyFrame does next, from the finish
  m.fromFinished(f);
  m.flaggedForMarginalization.assign(nf, 0), m.flaggedForMarginalization[leaves] = 1;
  m.margFrames.assign(1, leaves);
  for (int k = 0; k < 8; k++) m.framePrior.push_back(100.0 * (k + 1)), m.frameDeltaPrior.push_back(0.001 * (k + 1));
  if (device) marginalizeWindow(ctx, m);
  else marginalizeWindowHost(F.w, F.h, planes.data(), m);
  out.verdict = vhash(m.verdict), out.HM = vhash(m.HM_out), out.bM = vhash(m.bM_out), out.resInM = m.resInM, out.ad_ht_delta = vhash(m.adHTdeltaF);

  // (3) the next keyframe's window, with the final linearisation's states and at the finish's evaluation point
  kw.drop(F.frame_ids[leaves]);
  WindowFinish f2;
  WindowStep &w = f2.optimizer.window;
  const window_case::Shrunk shrunk = window_case::shrink_window(f.optimizer.window, f.points, m, leaves, &kw, w, f2.points);
  for (int p : shrunk.kept) { // the points' counters, last residuals and last states
    f2.numGoodResiduals.push_back(f.numGoodResiduals[p]), f2.maxRelBaseline.push_back(f.maxRelBaseline[p]);
    for (int s = 0; s < 2; s++) {
      const int last = f.lastResiduals[2 * p + s];
      f2.lastResiduals.push_back(last >= 0 ? shrunk.new_res[last] : -1), f2.lastResidualStates.push_back(f.lastResidualStates[2 * p + s]);
    }
  }
  f2.optimizer.maxIterations = max_its;
  std::vector<const float *> planes2 = window_case::per_frame(planes, shrunk.stay, 1);
  // (4)
  const FinishResult r2 = device ? f2.finishWindow(ctx) : f2.finishWindowHost(F.w, F.h, planes2.data());
  out.second = r2.loop.pattern, out.two = decisions(f2, r2), out.kept = (int)shrunk.kept.size(), out.residuals = (int)w.residuals.size();
  out.last = r2.loop.lastEnergy + r2.loop.lastEnergyM, out.energy = r2.energy, out.rmse = r2.rmse;
  out.state = vhash(w.state), out.state_zero = vhash(w.stateZero), out.eval = vhash(w.worldToCamEval), out.calib = fnv1a(w.calib, 32);
  out.idepth = vhash(w.idepth);
  return out;
}

static void show(const char *name, const Decisions &d) {
  auto x = [](uint64_t h) { return (unsigned long long)h; };
  printf("\"%s\": {\"keep\": \"%016llx\", \"states\": \"%016llx\", \"n_good\": \"%016llx\", \"last_res\": \"%016llx\", \"last_state\": \"%016llx\", "
         "\"dropped\": \"%016llx\", \"res_index\": \"%016llx\", \"point_index\": \"%016llx\", \"residuals\": %d, \"points\": %d, \"lost\": %d}, ",
         name, x(d.keep), x(d.states), x(d.n_good), x(d.last_res), x(d.last_state), x(d.dropped), x(d.res_index), x(d.point_index), d.residuals, d.points, d.lost);
}

int main(int argc, char **argv) {
  StepCase S;
  if (argc < 2 || !load_step(argv[1], S)) {
    fprintf(stderr, "usage: finish_demo FINISH_FILE [MAX_ITERATIONS]\n");
    return 2;
  }
  const int max_its = argc > 2 ? atoi(argv[2]) : 6;
  dsm_context *ctx = nullptr;
  immature_check(dsm_context_create(0, &ctx), "dsm_context_create");
  const Chain dev = chain(S, ctx, true, max_its), host = chain(S, ctx, false, max_its);
  dsm_context_destroy(ctx);
  auto x = [](uint64_t h) { return (unsigned long long)h; };
  printf("{");
  for (const Chain *c : {&dev, &host}) {
    printf("\"%s\": {\"first\": \"%s\", \"second\": \"%s\", ", c == &dev ? "chain_device" : "chain_host", c->first.c_str(), c->second.c_str());
    show("one", c->one), show("two", c->two);
    printf("\"verdict\": \"%016llx\", \"HM_out\": \"%016llx\", \"bM_out\": \"%016llx\", \"ad_ht_delta\": \"%016llx\", \"resInM\": %d, \"kept\": %d, "
           "\"residuals\": %d, \"state\": \"%016llx\", \"state_zero\": \"%016llx\", \"eval\": \"%016llx\", \"calib\": \"%016llx\", \"idepth\": \"%016llx\", "
           "\"last\": %.17g, \"energy\": %.17g, \"rmse\": %.9g}, ",
           x(c->verdict), x(c->HM), x(c->bM), x(c->ad_ht_delta), c->resInM, c->kept, c->residuals, x(c->state), x(c->state_zero), x(c->eval), x(c->calib),
           x(c->idepth), c->last, c->energy, (double)c->rmse);
  }
  const int same = dev.first == host.first && dev.second == host.second && dev.one == host.one && dev.two == host.two && dev.verdict == host.verdict &&
                   dev.resInM == host.resInM;
  printf("\"decisions_equal\": %d}\n", same);
  return same ? 0 : 1;
}
