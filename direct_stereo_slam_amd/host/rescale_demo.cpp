// rescale_demo.cpp -- a stereo keyframe as FrontEnd::makeKeyFrame runs it (FrontEnd.cpp:721-840), through the C++ adaptors
// host/WindowFinish.hpp, host/WindowRescale.hpp, host/WindowMarginalize.hpp and host/WindowNullspace.hpp:
//   (1) WindowFinish::finishWindow and shrink(): optimize, whole (device form);
//   (2) WindowRescale::fromFinished and the rescale call: optimizeScale behind its scale search (:806, :1010-1061).  The newest frame
//       was tracked against frame n - 2 (a pose outside the window for one frame): refCamToWorld is that frame's evaluation pose
//       inverted, camToTrackingRef the relative pose;
//   (3) MarginalizeRequest::fromFinished, applyTo, frame 1 flagged and marginalised (the frame's prior 100 (k + 1), its delta prior
//       0.001 (k + 1));
//   (4) applyTo(WindowNullspace) and the nullspaces at the returned evaluation poses.
// The chain runs without (2), and with (2) accepted (error 0.5 under the threshold 1), rejected (error 2) and disabled, through the
// device form and through the host form of the rescale call; the other calls are the device's in every run.  Then the accepted and the
// rejected window go through ONE call, and a ScaleState runs through accept, jump, and six rejections.
// Input: a finish file (window_case.hpp, kind FINISH; tests/_finish_ref.py writes the checker's scenes).
// Usage: rescale_demo FINISH_FILE [NEW_SCALE = 1.4] [MAX_ITERATIONS = 6].  Prints one JSON line with every chain's FNV-1a hashes; exit
// status 0 when the device and host chains agreed and the call of two repeated the single calls.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "WindowRescale.hpp"
#include "window_case_requests.hpp"

using namespace dsm_host;
using window_case::fnv1a;
using window_case::vhash;

// poses {qx, qy, qz, qw, tx, ty, tz}: just enough of SE3 to state a tracking reference
static void rotate(const double *q, const double *v, double *o) {
  const double u[3] = {2 * (q[1] * v[2] - q[2] * v[1]), 2 * (q[2] * v[0] - q[0] * v[2]), 2 * (q[0] * v[1] - q[1] * v[0])};
  o[0] = v[0] + q[3] * u[0] + (q[1] * u[2] - q[2] * u[1]), o[1] = v[1] + q[3] * u[1] + (q[2] * u[0] - q[0] * u[2]);
  o[2] = v[2] + q[3] * u[2] + (q[0] * u[1] - q[1] * u[0]);
}
static void inverse(const double *a, double *o) {
  const double qc[4] = {-a[0], -a[1], -a[2], a[3]};
  double r[3];
  rotate(qc, a + 4, r);
  memcpy(o, qc, 32), o[4] = -r[0], o[5] = -r[1], o[6] = -r[2];
}
static void multiply(const double *a, const double *b, double *o) {
  double r[3];
  rotate(a, b + 4, r);
  const double q[4] = {a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1], a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
                       a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0], a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]};
  const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  for (int k = 0; k < 4; k++) o[k] = q[k] / n;
  for (int k = 0; k < 3; k++) o[4 + k] = a[4 + k] + r[k];
}

struct StepCase {
  window_case::Case file;
  std::vector<ActivePointData> points;
  WindowFinish proto;
};

enum Mode { NONE, ACCEPTED, REJECTED, DISABLED };

struct Chain {
  int decision = -1, trapped = 0, fails = 0, resInM = 0, rank = 0;
  float scaleErrorOut = 0, appliedScale = 0;
  uint64_t idepth = 0, eval = 0, state = 0, tables = 0, ad_ht_delta = 0, verdict = 0, HM = 0, bM = 0, null_basis = 0, null_pinv = 0;
  bool operator==(const Chain &o) const {
    return decision == o.decision && trapped == o.trapped && fails == o.fails && same_window(o) && memcmp(&scaleErrorOut, &o.scaleErrorOut, 4) == 0 &&
           memcmp(&appliedScale, &o.appliedScale, 4) == 0;
  }
  bool same_window(const Chain &o) const {
    return resInM == o.resInM && rank == o.rank && idepth == o.idepth && eval == o.eval && state == o.state && tables == o.tables &&
           ad_ht_delta == o.ad_ht_delta && verdict == o.verdict && HM == o.HM && bM == o.bM && null_basis == o.null_basis && null_pinv == o.null_pinv;
  }
};

static void prepare(WindowRescale &r, const WindowFinish &f, Mode mode, float new_scale) {
  r.fromFinished(f);
  const size_t n = r.frames();
  const double *ev = r.in.worldToCamEval.data();
  double ref[7], ctr[7], c2w[7], ref_inv[7];
  inverse(ev + 7 * (n - 1), c2w);
  if (n > 1) {
    inverse(ev + 7 * (n - 2), ref);
  } else {
    const double outside[7] = {0.0, 0.0, 0.0, 1.0, 0.1, -0.05, 0.02};
    memcpy(ref, outside, sizeof ref);
  }
  inverse(ref, ref_inv);
  multiply(ref_inv, c2w, ctr);
  r.setTrackingRef(ref, ctr, c2w);
  r.enabled = mode != DISABLED, r.thres = 1.0f, r.newScale = new_scale, r.scaleError = mode == REJECTED ? 2.0f : 0.5f;
}

// the finished and shrunk window `f` through (2)-(4); device: the rescale call's device form, otherwise its host form
static Chain chain(const WindowFinish &f, const window_case::Case &F, dsm_context *ctx, Mode mode, bool device, float new_scale) {
  Chain out;
  const size_t nf = F.nf;
  const int leaves = nf > 1 ? 1 : 0;
  MarginalizeRequest m;
  m.fromFinished(f);
  WindowNullspace ns;
  ns.worldToCamEval = f.optimizer.window.worldToCamEval, ns.stateZero = f.optimizer.window.stateZero, ns.exposure = f.optimizer.window.exposure;
  if (mode != NONE) {
    WindowRescale r;
    ScaleState scale;
    prepare(r, f, mode, new_scale);
    if (device) r.rescaleWindow(ctx, scale);
    else r.rescaleWindowHost(scale);
    r.applyTo(m), r.applyTo(ns);
    out.decision = r.decision, out.trapped = scale.trapped, out.fails = scale.fails, out.scaleErrorOut = r.scaleErrorOut, out.appliedScale = r.appliedScale;
    out.idepth = vhash(r.out.idepth), out.eval = vhash(r.out.worldToCamEval), out.state = vhash(r.out.state);
  } else {
    out.idepth = vhash(f.optimizer.window.idepth), out.eval = vhash(ns.worldToCamEval), out.state = vhash(f.optimizer.window.state);
  }
  for (float &e : ns.exposure) // the demo's scenes hold an exposure of 0, which the nullspace call refuses
    if (!(e > 0.f)) e = 1.f;
  out.ad_ht_delta = vhash(m.adHTdeltaF);
  out.tables = fnv1a(m.hes.lin.precalc.data(), sizeof(LinearizePrecalc) * m.hes.lin.precalc.size());
  m.flaggedForMarginalization.assign(nf, 0), m.flaggedForMarginalization[leaves] = 1;
  m.margFrames.assign(1, leaves);
  for (int k = 0; k < 8; k++) m.framePrior.push_back(100.0 * (k + 1)), m.frameDeltaPrior.push_back(0.001 * (k + 1));
  marginalizeWindow(ctx, m);
  out.verdict = vhash(m.verdict), out.HM = vhash(m.HM_out), out.bM = vhash(m.bM_out), out.resInM = m.resInM;
  ns.compute(ctx);
  out.null_basis = vhash(ns.nullBasis), out.null_pinv = vhash(ns.nullPinv), out.rank = ns.rank;
  return out;
}

static void show(const char *name, const Chain &c, const char *end) {
  auto x = [](uint64_t h) { return (unsigned long long)h; };
  printf("\"%s\": {\"decision\": %d, \"trapped\": %d, \"fails\": %d, \"scale_error\": %.9g, \"applied_scale\": %.9g, \"idepth\": \"%016llx\", "
         "\"eval\": \"%016llx\", \"state\": \"%016llx\", \"tables\": \"%016llx\", \"ad_ht_delta\": \"%016llx\", \"verdict\": \"%016llx\", "
         "\"H_M_out\": \"%016llx\", \"b_M_out\": \"%016llx\", \"resInM\": %d, \"null_basis\": \"%016llx\", \"null_pinv\": \"%016llx\", \"rank\": %d}%s",
         name, c.decision, c.trapped, c.fails, (double)c.scaleErrorOut, (double)c.appliedScale, x(c.idepth), x(c.eval), x(c.state), x(c.tables),
         x(c.ad_ht_delta), x(c.verdict), x(c.HM), x(c.bM), c.resInM, x(c.null_basis), x(c.null_pinv), c.rank, end);
}

int main(int argc, char **argv) {
  StepCase S;
  if (argc < 2 || !window_case::read_case(argv[1], window_case::FINISH, S.file)) {
    fprintf(stderr, "usage: rescale_demo FINISH_FILE [NEW_SCALE] [MAX_ITERATIONS]\n");
    return 2;
  }
  S.points = window_case::points(S.file);
  window_case::fill(S.proto, S.file);
  const float new_scale = argc > 2 ? (float)atof(argv[2]) : 1.4f;
  const int max_its = argc > 3 ? atoi(argv[3]) : 6;
  const window_case::Case &F = S.file;
  dsm_context *ctx = nullptr;
  immature_check(dsm_context_create(0, &ctx), "dsm_context_create");
  Chain none, dev[4], host[4];
  int windows_equal = 0;
  std::string sequence;
  {
    KeyframeWindow kw(ctx, F.w, F.h, (int)F.nf);
    window_case::put_planes(F, kw);
    WindowFinish f = S.proto; // (1)
    f.points = S.points;
    f.optimizer.maxIterations = max_its;
    f.optimizer.window.req.hes.lin.window = &kw;
    f.finishWindow(ctx);
    f.shrink();
    none = chain(f, F, ctx, NONE, true, new_scale);
    for (int mode = ACCEPTED; mode <= DISABLED; mode++)
      dev[mode] = chain(f, F, ctx, (Mode)mode, true, new_scale), host[mode] = chain(f, F, ctx, (Mode)mode, false, new_scale);

    // two windows in ONE call, each with its own decision and state
    WindowRescale a, b, a1, b1;
    ScaleState sa, sb, sa1, sb1;
    prepare(a, f, ACCEPTED, new_scale), prepare(b, f, REJECTED, new_scale), a1 = a, b1 = b;
    sb.trapped = sb1.trapped = true, sb.fails = sb1.fails = 2;
    std::vector<WindowRescale *> two = {&a, &b};
    std::vector<ScaleState *> states = {&sa, &sb};
    WindowRescale::rescaleWindows(ctx, two, states);
    a1.rescaleWindow(ctx, sa1), b1.rescaleWindow(ctx, sb1);
    auto same = [](const WindowRescale &p, const WindowRescale &q) {
      return p.decision == q.decision && vhash(p.out.idepth) == vhash(q.out.idepth) && vhash(p.out.worldToCamEval) == vhash(q.out.worldToCamEval) &&
             vhash(p.out.pre[2]) == vhash(q.out.pre[2]) && vhash(p.out.adHTdeltaF) == vhash(q.out.adHTdeltaF) && vhash(p.out.deltaX) == vhash(q.out.deltaX);
    };
    windows_equal = same(a, a1) && same(b, b1) && a.accepted() && !b.accepted() && sa.trapped && sa.fails == 0 && sb.trapped && sb.fails == 3 &&
                    sb1.fails == 3 && vhash(b.out.idepth) == vhash(b.in.idepth);

    // S1 through a ScaleState: an accept traps, a trapped jump rejects, six rejections in a row untrap
    ScaleState s;
    WindowRescale r;
    prepare(r, f, ACCEPTED, 5.0f);
    const float errors[8] = {0.5f, 0.5f, 2.f, 2.f, 2.f, 2.f, 2.f, 0.5f}, scales[8] = {5.0f, 1.6f, 1.1f, 1.1f, 1.1f, 1.1f, 1.1f, 1.6f};
    for (int k = 0; k < 8; k++) {
      r.scaleError = errors[k], r.newScale = scales[k];
      const float returned = r.rescaleWindowHost(s);
      sequence += r.accepted() ? 'A' : returned == -1.f ? 'U' : 'R';
      sequence += s.wantGuesses() ? 'g' : 't';
    }
  }
  dsm_context_destroy(ctx);
  int forms_equal = 1;
  for (int mode = ACCEPTED; mode <= DISABLED; mode++) forms_equal = forms_equal && dev[mode] == host[mode];
  printf("{");
  show("none", none, ", ");
  const char *names[4] = {"", "accepted", "rejected", "disabled"};
  for (int form = 0; form < 2; form++) {
    printf("\"%s\": {", form ? "host" : "device");
    for (int mode = ACCEPTED; mode <= DISABLED; mode++) show(names[mode], form ? host[mode] : dev[mode], mode < DISABLED ? ", " : "}, ");
  }
  printf("\"sequence\": \"%s\", \"windows_equal\": %d, \"forms_equal\": %d}\n", sequence.c_str(), windows_equal, forms_equal);
  return windows_equal && forms_equal ? 0 : 1;
}
