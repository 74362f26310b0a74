// marginalize_demo.cpp -- flagPointsForRemoval, marginalizePointsF and marginalizeFrame (FrontEnd.cpp:816-839) as ONE call through the
// C++ adaptor host/WindowMarginalize.hpp.
// (1) Two windows read from marginalize files: window A alone on the device, A and B -- two DIFFERENT windows, with different numbers
// of frames leaving -- in one call, and both through the host form.
// (2) The chain of two keyframes on a window read from a step file, through the device forms and through
// the host forms: WindowOptimize::optimize, MarginalizeRequest::fromWindow on its committed members, frame 1 flagged and marginalised
// (every point with numGoodResiduals 9 and last states IN; the frame's prior 100 (k + 1), its delta prior 0.001 (k + 1)), then the
// window shrunk as makeKeyFrame leaves it -- the frame dropped, the points of verdict 0 kept with their residuals against the
// frames that stay, H_L / b_L, the priors and the states cut to those frames -- and optimize again on HM_out / bM_out.
// Input files: two marginalize files and a step file (window_case.hpp, kinds MARGINALIZE and STEP; tests/_marginalize_ref.py and
// tests/_step_ref.py write the checkers' scenes).
// Usage: marginalize_demo FILE_A FILE_B STEP_FILE [MAX_ITERATIONS = 6].  Prints one JSON line: the chain's outcome in both forms (the patterns of
// both optimisations, the hashes of the verdicts, of the returned prior, of the second optimisation's final state, calibration and
// depths, its last energy), and per run the FNV-1a hashes of the verdicts, of HM_out and bM_out, and
// resInM; for A alone also the hashes of the prior after the points and of res_toZeroF; and the hash of the adHTdeltaF that
// MarginalizeRequest::setDeltaF forms for A from a state that stands off its zero state by 0.001 (1 + (7 frame + 3 k) mod 11).
// Exit status 0 when A in the call of two equalled A alone, B in the call of two equalled B alone, and the device equalled the host form.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "window_case_requests.hpp"

using namespace dsm_host;
using window_case::fnv1a;

struct Outcome {
  uint64_t verdict = 0, HM = 0, bM = 0;
  int resInM = 0;
  bool operator==(const Outcome &o) const { return verdict == o.verdict && HM == o.HM && bM == o.bM && resInM == o.resInM; }
};
static Outcome outcome(const MarginalizeRequest &m) {
  Outcome o;
  o.verdict = fnv1a(m.verdict.data(), m.verdict.size()), o.HM = fnv1a(m.HM_out.data(), 8 * m.HM_out.size());
  o.bM = fnv1a(m.bM_out.data(), 8 * m.bM_out.size()), o.resInM = m.resInM;
  return o;
}

// a window of a marginalize file: the prototype of its request, its points and its residuals
struct Case {
  window_case::Case file;
  std::vector<ActivePointData> points;
  std::vector<ActiveResidualData> residuals;
  MarginalizeRequest proto;
};

static bool load(const char *path, Case &c) {
  if (!window_case::read_case(path, window_case::MARGINALIZE, c.file)) return false;
  c.points = window_case::points(c.file), c.residuals = window_case::residuals(c.file);
  window_case::fill(c.proto, c.file);
  return true;
}

// ---- (2) the chain ----------------------------------------------------------------------------------------------------------------

// a window of a step file: the prototype of its WindowOptimize and its points
struct StepCase {
  window_case::Case file;
  std::vector<ActivePointData> points;
  WindowOptimize proto;
};

static bool load_step(const char *path, StepCase &c) {
  if (!window_case::read_case(path, window_case::STEP, c.file)) return false;
  c.points = window_case::points(c.file);
  window_case::fill(c.proto.window, c.file);
  return true;
}

struct Chain {
  std::string first, second; // the accept / reject patterns of the two optimisations
  uint64_t verdict = 0, HM = 0, bM = 0, state = 0, calib = 0, idepth = 0;
  int resInM = 0, kept = 0, residuals = 0;
  double last = 0;
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
  WindowOptimize o = S.proto; // the first keyframe's optimisation
  o.maxIterations = max_its;
  o.window.req.hes.lin.window = &kw, o.window.req.hes.lin.points = &S.points;
  out.first = (device ? o.optimize(ctx) : o.optimizeHost(F.w, F.h, planes.data())).pattern;

  MarginalizeRequest m; // what makeKeyFrame does next, on the window's committed members
  m.fromWindow(o);
  const size_t n_pts = S.points.size();
  m.flaggedForMarginalization.assign(nf, 0), m.flaggedForMarginalization[leaves] = 1;
  m.numGoodResiduals.assign(n_pts, 9), m.lastResiduals.assign(2 * n_pts, DSM_RES_IN);
  m.margFrames.assign(1, leaves);
  for (int k = 0; k < 8; k++) m.framePrior.push_back(100.0 * (k + 1)), m.frameDeltaPrior.push_back(0.001 * (k + 1));
  if (device) marginalizeWindow(ctx, m);
  else marginalizeWindowHost(F.w, F.h, planes.data(), m);
  out.verdict = fnv1a(m.verdict.data(), m.verdict.size()), out.HM = fnv1a(m.HM_out.data(), 8 * m.HM_out.size());
  out.bM = fnv1a(m.bM_out.data(), 8 * m.bM_out.size()), out.resInM = m.resInM;

  // the next keyframe's window, on the committed states
  kw.drop(F.frame_ids[leaves]);
  std::vector<ActivePointData> points;
  WindowOptimize o2;
  WindowStep &w = o2.window;
  const window_case::Shrunk shrunk = window_case::shrink_window(o.window, S.points, m, leaves, &kw, w, points);
  w.req.hes.lin.points = &points;
  o2.maxIterations = max_its;
  std::vector<const float *> planes2 = window_case::per_frame(planes, shrunk.stay, 1);
  const OptimizeResult r2 = device ? o2.optimize(ctx) : o2.optimizeHost(F.w, F.h, planes2.data());
  out.second = r2.pattern, out.last = r2.lastEnergy + r2.lastEnergyM, out.kept = (int)shrunk.kept.size(), out.residuals = (int)w.residuals.size();
  out.state = fnv1a(w.state.data(), 8 * w.state.size()), out.calib = fnv1a(w.calib, 32), out.idepth = fnv1a(w.idepth.data(), 4 * w.idepth.size());
  return out;
}

int main(int argc, char **argv) {
  if (argc < 4) {
    fprintf(stderr, "usage: marginalize_demo FILE_A FILE_B STEP_FILE [MAX_ITERATIONS]\n");
    return 2;
  }
  Case A, B;
  if (!load(argv[1], A) || !load(argv[2], B) || A.file.w != B.file.w || A.file.h != B.file.h) {
    fprintf(stderr, "marginalize_demo: cannot read the files, or two image sizes\n");
    return 2;
  }
  StepCase S;
  if (!load_step(argv[3], S)) {
    fprintf(stderr, "marginalize_demo: cannot read the step file\n");
    return 2;
  }
  const int max_its = argc > 4 ? atoi(argv[4]) : 6;
  dsm_context *ctx = nullptr;
  immature_check(dsm_context_create(0, &ctx), "dsm_context_create");
  const Chain chain_device = chain(S, ctx, true, max_its), chain_host = chain(S, ctx, false, max_its);
  Outcome alone_a, alone_b, many_a, many_b, host_a, host_b;
  uint64_t points_prior = 0, rtz = 0, deltas = 0;
  {
    KeyframeWindow wa(ctx, A.file.w, A.file.h, (int)A.file.nf), wb(ctx, B.file.w, B.file.h, (int)B.file.nf);
    window_case::put_planes(A.file, wa), window_case::put_planes(B.file, wb);
    auto request = [](const Case &c, KeyframeWindow *w) {
      MarginalizeRequest m = c.proto;
      m.hes.lin.window = w, m.hes.lin.points = &c.points, m.hes.lin.residuals = &c.residuals;
      return m;
    };
    MarginalizeRequest a = request(A, &wa), b = request(B, &wb);
    a.wantDetails = true;
    marginalizeWindow(ctx, a);
    marginalizeWindow(ctx, b);
    alone_a = outcome(a), alone_b = outcome(b);
    points_prior = fnv1a(a.bM_points.data(), 8 * a.bM_points.size(), fnv1a(a.HM_points.data(), 8 * a.HM_points.size()));
    rtz = fnv1a(a.res_toZeroF.data(), 4 * a.res_toZeroF.size());

    MarginalizeRequest a2 = request(A, &wa), b2 = request(B, &wb); // the windows of two sequences in ONE call
    std::vector<MarginalizeRequest *> two = {&a2, &b2};
    marginalizeWindows(ctx, two);
    many_a = outcome(a2), many_b = outcome(b2);

    MarginalizeRequest ha = request(A, &wa), hb = request(B, &wb); // the host form (the request still names a window; the host form does not read it)
    marginalizeWindowHost(A.file.w, A.file.h, A.file.planes, ha);
    marginalizeWindowHost(B.file.w, B.file.h, B.file.planes, hb);
    host_a = outcome(ha), host_b = outcome(hb);

    MarginalizeRequest d = request(A, &wa); // setDeltaF on a state that stands off its zero state
    std::vector<double> zero(8 * A.file.nf, 0.25), state(8 * A.file.nf);
    for (size_t i = 0; i < A.file.nf; i++)
      for (size_t k = 0; k < 8; k++) state[8 * i + k] = zero[8 * i + k] + 0.001 * (double)(1 + (7 * i + 3 * k) % 11);
    const double calib[4] = {10.001, 10.002, 5.003, 5.004}, calib_zero[4] = {10.0, 10.0, 5.0, 5.0};
    d.setDeltaF(state, zero, calib, calib_zero);
    deltas = fnv1a(d.cDeltaF, 16, fnv1a(d.adHTdeltaF.data(), 4 * d.adHTdeltaF.size()));
  }
  dsm_context_destroy(ctx);
  auto show = [](const char *name, const Outcome &o) {
    printf("\"%s\": {\"verdict\": \"%016llx\", \"HM_out\": \"%016llx\", \"bM_out\": \"%016llx\", \"resInM\": %d}, ", name, (unsigned long long)o.verdict,
           (unsigned long long)o.HM, (unsigned long long)o.bM, o.resInM);
  };
  const int windows_equal = many_a == alone_a && many_b == alone_b, forms_equal = alone_a == host_a && alone_b == host_b;
  printf("{");
  for (const Chain *c : {&chain_device, &chain_host})
    printf("\"%s\": {\"first\": \"%s\", \"second\": \"%s\", \"verdict\": \"%016llx\", \"HM_out\": \"%016llx\", \"bM_out\": \"%016llx\", \"resInM\": %d, "
           "\"kept\": %d, \"residuals\": %d, \"state\": \"%016llx\", \"calib\": \"%016llx\", \"idepth\": \"%016llx\", \"last\": %.17g}, ",
           c == &chain_device ? "chain_device" : "chain_host", c->first.c_str(), c->second.c_str(), (unsigned long long)c->verdict,
           (unsigned long long)c->HM, (unsigned long long)c->bM, c->resInM, c->kept, c->residuals, (unsigned long long)c->state,
           (unsigned long long)c->calib, (unsigned long long)c->idepth, c->last);
  show("device_a", alone_a), show("device_b", alone_b), show("many_a", many_a), show("many_b", many_b), show("host_a", host_a), show("host_b", host_b);
  printf("\"points_prior_a\": \"%016llx\", \"res_to_zero_a\": \"%016llx\", \"set_delta_a\": \"%016llx\", \"windows_equal\": %d, \"device_equals_host\": %d}\n",
         (unsigned long long)points_prior, (unsigned long long)rtz, (unsigned long long)deltas, windows_equal, forms_equal);
  return windows_equal && forms_equal ? 0 : 1;
}
