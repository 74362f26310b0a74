// finish_demo.cpp -- the chain of two keyframes as FrontEnd::makeKeyFrame runs it, through the C++ adaptors host/WindowFinish.hpp and
// host/WindowMarginalize.hpp, once through the device forms and once through the host forms:
//   (1) WindowFinish::finishWindow: optimize's loop and, in the same call, setEvalPT, setAdjointsF, the final linearizeAll(true) with
//       its bookkeeping and removeOutliers; shrink() erases what did not survive;
//   (2) MarginalizeRequest::fromFinished on it; frame 1 flagged and marginalised (the frame's prior 100 (k + 1), its delta prior
//       0.001 (k + 1));
//   (3) the window shrunk as host/marginalize_demo.cpp does -- the frame dropped, the points of verdict 0 kept with their residuals
//       against the frames that stay, H_L / b_L, the priors, the states and adHost / adTarget cut to those frames -- with the points'
//       counters, last residuals and last states carried over;
//   (4) finishWindow again, on the returned prior.
// Input (native byte order): a finish file (tests/_finish_ref.py, write_case): host/step_demo.cpp's step file, then per point
// numGoodResiduals, maxRelBaseline, the two last residual indices and the two last states.
// Usage: finish_demo FINISH_FILE [MAX_ITERATIONS = 6].  Prints one JSON line: per form the two patterns, the counts, and the FNV-1a hashes
// of both finishes' decisions and of the marginalisation's verdicts and prior; the second finish's state, energies and rmse.
// Exit status 0 when both forms took the same decisions.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "WindowMarginalize.hpp" // includes WindowFinish.hpp

using namespace dsm_host;

static uint64_t fnv1a(const void *p, size_t n, uint64_t hsh = 1469598103934665603ull) {
  for (size_t i = 0; i < n; i++) hsh = (hsh ^ ((const unsigned char *)p)[i]) * 1099511628211ull;
  return hsh;
}
template <typename T>
static uint64_t hash_of(const std::vector<T> &v) { return fnv1a(v.data(), sizeof(T) * v.size()); }
template <typename T>
static bool rd(FILE *f, std::vector<T> &v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

struct StepCase {
  int wh[2] = {0, 0};
  std::vector<int> ids;
  std::vector<float> planes;
  std::vector<ActivePointData> points;
  WindowFinish proto; // with the finish's per-point inputs
  size_t nf = 0, npx = 0;
};

static bool load_step(const char *path, StepCase &c) {
  FILE *f = fopen(path, "rb");
  int nff[2] = {0, 0}, n_pts = 0, n_res = 0, shift = 1, n_null = 0, has_hm = 0, has_prior = 0;
  float cal[6];
  double lambda = 0;
  std::vector<float> pre, eth, prec, rrec, pin, idb, ids_step, expo, fac;
  std::vector<double> adh, adt, HL, bL, HM, bM, basis, pinv, ev, zero, backup, fstep, cz, cb, cs, prior, pzero;
  bool good = f && fread(c.wh, sizeof(int), 2, f) == 2 && fread(cal, sizeof(float), 6, f) == 6 && fread(nff, sizeof(int), 2, f) == 2 && nff[0] >= 1 &&
              nff[0] <= DSM_WINDOW_MAX_FRAMES && c.wh[0] > 0 && c.wh[1] > 0;
  const size_t nf = good ? nff[0] : 0, npx = good ? (size_t)c.wh[0] * c.wh[1] : 0, N = 4 + 8 * nf;
  good = good && rd(f, c.ids, nf) && rd(f, c.planes, nf * npx) && rd(f, pre, nf * nf * 27) && rd(f, eth, nf) && fread(&n_pts, sizeof(int), 1, f) == 1 &&
         n_pts >= 0 && rd(f, prec, (size_t)n_pts * 21) && fread(&n_res, sizeof(int), 1, f) == 1 && n_res >= 0 && rd(f, rrec, (size_t)n_res * 5) &&
         rd(f, adh, nf * nf * 64) && rd(f, adt, nf * nf * 64) && rd(f, pin, (size_t)n_pts * 8) && fread(&shift, sizeof(int), 1, f) == 1;
  good = good && rd(f, HL, N * N) && rd(f, bL, N) && fread(&has_hm, sizeof(int), 1, f) == 1 && (!has_hm || (rd(f, HM, N * N) && rd(f, bM, N))) &&
         fread(&lambda, sizeof(double), 1, f) == 1 && fread(&n_null, sizeof(int), 1, f) == 1 && n_null >= 0 && n_null <= DSM_SOLVE_MAX_NULL &&
         rd(f, basis, N * n_null) && rd(f, pinv, N * n_null);
  good = good && rd(f, ev, 7 * nf) && rd(f, zero, 8 * nf) && rd(f, backup, 8 * nf) && rd(f, fstep, 8 * nf) && rd(f, cz, 4) && rd(f, cb, 4) && rd(f, cs, 4) &&
         rd(f, idb, n_pts) && rd(f, ids_step, n_pts) && rd(f, expo, nf) && rd(f, fac, 5) && fread(&has_prior, sizeof(int), 1, f) == 1 &&
         (!has_prior || (rd(f, prior, N) && rd(f, pzero, N)));
  // the finish's inputs behind the step file
  good = good && rd(f, c.proto.numGoodResiduals, n_pts) && rd(f, c.proto.maxRelBaseline, n_pts) && rd(f, c.proto.lastResiduals, 2 * (size_t)n_pts) &&
         rd(f, c.proto.lastResidualStates, 2 * (size_t)n_pts);
  if (f) fclose(f);
  if (!good) return false;
  c.nf = nf, c.npx = npx;
  c.points.resize(n_pts);
  for (int i = 0; i < n_pts; i++) {
    const float *q = &prec[(size_t)21 * i];
    memcpy(&c.points[i].host, q, 4);
    c.points[i].u = q[1], c.points[i].v = q[2], c.points[i].idepth_scaled = 0, c.points[i].idepth_zero_scaled = 0;
    memcpy(c.points[i].color, q + 5, 32), memcpy(c.points[i].weights, q + 13, 32);
  }
  WindowStep &w = c.proto.optimizer.window;
  w.residuals.resize(n_res);
  for (int i = 0; i < n_res; i++) {
    const float *q = &rrec[(size_t)5 * i];
    int isnew;
    ActiveResidualData &r = w.residuals[i];
    memcpy(&r.point, q, 4), memcpy(&r.target, q + 1, 4), memcpy(&r.state_state, q + 2, 4);
    r.state_energy = q[3];
    memcpy(&isnew, q + 4, 4);
    r.isNew = isnew != 0;
  }
  LinearizeRequest &lin = w.req.hes.lin;
  lin.frame_ids = c.ids, lin.fixLinearization = false, lin.wantJacobians = false;
  w.frameEnergyTH = eth;
  w.req.hes.adHost = adh, w.req.hes.adTarget = adt, w.req.hes.shiftPriorToZero = shift != 0;
  for (int i = 0; i < n_pts; i++) {
    const float *q = &pin[(size_t)8 * i];
    w.req.hes.priorF.push_back(q[0]), w.req.hes.Hdd_accLF.push_back(q[2]), w.req.hes.bd_accLF.push_back(q[3]);
    w.req.hes.Hcd_accLF.insert(w.req.hes.Hcd_accLF.end(), q + 4, q + 8);
  }
  w.req.H_L = HL, w.req.b_L = bL, w.req.HM = HM, w.req.bM = bM, w.req.nullBasis = basis, w.req.nullPinv = pinv;
  w.worldToCamEval = ev, w.stateZero = zero, w.exposure = expo, w.prior = prior, w.priorZero = pzero;
  w.state = backup, w.idepth = idb;
  memcpy(w.calibZero, cz.data(), 32), memcpy(w.calib, cb.data(), 32);
  return true;
}

// rows / columns 0..3 and those of the frames in `stay`, of an N-vector or an N x N matrix (empty stays empty)
static std::vector<double> cut(const std::vector<double> &v, const std::vector<int> &stay, size_t N, bool matrix) {
  std::vector<int> idx = {0, 1, 2, 3};
  for (int f : stay)
    for (int k = 0; k < 8; k++) idx.push_back(4 + 8 * f + k);
  std::vector<double> out;
  if (v.empty()) return out;
  for (int i : idx) {
    if (!matrix) out.push_back(v[i]);
    else
      for (int j : idx) out.push_back(v[(size_t)i * N + j]);
  }
  return out;
}
template <typename T>
static std::vector<T> per_frame(const std::vector<T> &v, const std::vector<int> &stay, size_t width) {
  std::vector<T> out;
  for (int f : stay) out.insert(out.end(), v.begin() + f * width, v.begin() + (f + 1) * width);
  return out;
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
  d.keep = hash_of(f.keep), d.states = hash_of(states), d.n_good = hash_of(f.numGoodResiduals), d.last_res = hash_of(f.lastResiduals);
  d.last_state = hash_of(f.lastResidualStates), d.dropped = hash_of(f.pointDropped), d.res_index = hash_of(f.resIndex), d.point_index = hash_of(f.pointIndex);
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
  const size_t nf = S.nf, N = 4 + 8 * nf;
  const int leaves = nf > 1 ? 1 : 0;
  KeyframeWindow kw(ctx, S.wh[0], S.wh[1], (int)nf);
  std::vector<const float *> planes(nf);
  for (size_t k = 0; k < nf; k++) kw.put(S.ids[k], &S.planes[k * S.npx]), planes[k] = &S.planes[k * S.npx];
  WindowFinish f = S.proto; // (1) the first keyframe's optimize, whole
  f.points = S.points;
  f.optimizer.maxIterations = max_its;
  f.optimizer.window.req.hes.lin.window = &kw;
  const FinishResult r1 = device ? f.finishWindow(ctx) : f.finishWindowHost(S.wh[0], S.wh[1], planes.data());
  out.first = r1.loop.pattern, out.one = decisions(f, r1);
  f.shrink();

  MarginalizeRequest m; // (2) what makeKeyFrame does next, from the finish
  m.fromFinished(f);
  m.flaggedForMarginalization.assign(nf, 0), m.flaggedForMarginalization[leaves] = 1;
  m.margFrames.assign(1, leaves);
  for (int k = 0; k < 8; k++) m.framePrior.push_back(100.0 * (k + 1)), m.frameDeltaPrior.push_back(0.001 * (k + 1));
  if (device) marginalizeWindow(ctx, m);
  else marginalizeWindowHost(S.wh[0], S.wh[1], planes.data(), m);
  out.verdict = hash_of(m.verdict), out.HM = hash_of(m.HM_out), out.bM = hash_of(m.bM_out), out.resInM = m.resInM, out.ad_ht_delta = hash_of(m.adHTdeltaF);

  // (3) the next keyframe's window: the frame dropped, the points of verdict 0 and their residuals against the frames that stay
  const size_t n_pts = f.points.size();
  WindowStep &was = f.optimizer.window;
  std::vector<int> stay, new_frame(nf, -1), new_point(n_pts, -1), kept, new_res(was.residuals.size(), -1);
  for (size_t k = 0; k < nf; k++)
    if ((int)k != leaves) new_frame[k] = (int)stay.size(), stay.push_back((int)k);
  for (size_t p = 0; p < n_pts; p++)
    if (m.verdict[p] == 0) new_point[p] = (int)kept.size(), kept.push_back((int)p);
  kw.drop(S.ids[leaves]);
  WindowFinish f2;
  WindowStep &w = f2.optimizer.window;
  HessianRequest &H = w.req.hes;
  for (size_t r = 0; r < was.residuals.size(); r++) { // with the final linearisation's states
    const ActiveResidualData &q = was.residuals[r];
    if (new_point[q.point] < 0 || new_frame[q.target] < 0) continue;
    new_res[r] = (int)w.residuals.size();
    w.residuals.push_back(q);
    w.residuals.back().point = new_point[q.point], w.residuals.back().target = new_frame[q.target];
  }
  for (int p : kept) {
    f2.points.push_back(f.points[p]);
    f2.points.back().host = new_frame[f.points[p].host];
    w.idepth.push_back(was.idepth[p]);
    H.priorF.push_back(was.req.hes.priorF[p]), H.Hdd_accLF.push_back(was.req.hes.Hdd_accLF[p]), H.bd_accLF.push_back(was.req.hes.bd_accLF[p]);
    H.Hcd_accLF.insert(H.Hcd_accLF.end(), was.req.hes.Hcd_accLF.begin() + 4 * p, was.req.hes.Hcd_accLF.begin() + 4 * p + 4);
    f2.numGoodResiduals.push_back(f.numGoodResiduals[p]), f2.maxRelBaseline.push_back(f.maxRelBaseline[p]);
    for (int s = 0; s < 2; s++) {
      const int last = f.lastResiduals[2 * p + s];
      f2.lastResiduals.push_back(last >= 0 ? new_res[last] : -1), f2.lastResidualStates.push_back(f.lastResidualStates[2 * p + s]);
    }
  }
  H.lin.window = &kw, H.lin.fixLinearization = false, H.lin.wantJacobians = false;
  H.lin.frame_ids = per_frame(S.ids, stay, 1);
  w.frameEnergyTH = per_frame(was.frameEnergyTH, stay, 1);
  H.shiftPriorToZero = was.req.hes.shiftPriorToZero;
  for (int h : stay)
    for (int t : stay) { // the finish's adHost / adTarget
      const size_t at = ((size_t)h * nf + t) * 64;
      H.adHost.insert(H.adHost.end(), was.req.hes.adHost.begin() + at, was.req.hes.adHost.begin() + at + 64);
      H.adTarget.insert(H.adTarget.end(), was.req.hes.adTarget.begin() + at, was.req.hes.adTarget.begin() + at + 64);
    }
  w.req.H_L = cut(was.req.H_L, stay, N, true), w.req.b_L = cut(was.req.b_L, stay, N, false);
  w.req.HM = m.HM_out, w.req.bM = m.bM_out; // the returned prior
  w.prior = cut(was.prior, stay, N, false), w.priorZero = cut(was.priorZero, stay, N, false);
  w.worldToCamEval = per_frame(was.worldToCamEval, stay, 7), w.stateZero = per_frame(was.stateZero, stay, 8), w.exposure = per_frame(was.exposure, stay, 1);
  w.state = per_frame(was.state, stay, 8); // at the finish's evaluation point
  memcpy(w.calib, was.calib, 32), memcpy(w.calibZero, was.calibZero, 32);
  f2.optimizer.maxIterations = max_its;
  std::vector<const float *> planes2 = per_frame(planes, stay, 1);
  // (4)
  const FinishResult r2 = device ? f2.finishWindow(ctx) : f2.finishWindowHost(S.wh[0], S.wh[1], planes2.data());
  out.second = r2.loop.pattern, out.two = decisions(f2, r2), out.kept = (int)kept.size(), out.residuals = (int)w.residuals.size();
  out.last = r2.loop.lastEnergy + r2.loop.lastEnergyM, out.energy = r2.energy, out.rmse = r2.rmse;
  out.state = hash_of(w.state), out.state_zero = hash_of(w.stateZero), out.eval = hash_of(w.worldToCamEval), out.calib = fnv1a(w.calib, 32);
  out.idepth = hash_of(w.idepth);
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
