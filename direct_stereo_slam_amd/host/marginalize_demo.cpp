// marginalize_demo.cpp -- flagPointsForRemoval, marginalizePointsF and marginalizeFrame (FrontEnd.cpp:816-839) as ONE call through the
// C++ adaptor host/WindowMarginalize.hpp.
// (1) Two windows read from marginalize files: window A alone on the device, A and B -- two DIFFERENT windows, with different numbers
// of frames leaving -- in one call, and both through the host form.
// (2) The chain of two keyframes on a window read from a step file (host/step_demo.cpp's format), through the device forms and through
// the host forms: WindowOptimize::optimize, MarginalizeRequest::fromWindow on its committed members, frame 1 flagged and marginalised
// (every point with numGoodResiduals 9 and last states IN; the frame's prior 100 (k + 1), its delta prior 0.001 (k + 1)), then the
// window shrunk as makeKeyFrame leaves it -- the frame dropped, the points of verdict 0 kept with their residuals against the
// frames that stay, H_L / b_L, the priors and the states cut to those frames -- and optimize again on HM_out / bM_out.
// Input files (native byte order): tests/_marginalize_ref.py, write_case: the window file host/linearize_demo.cpp reads, then adHost,
// adTarget, per point (priorF, deltaF), the frames' flags, per point numGoodResiduals, the two last states and idepth_hessian,
// adHTdeltaF, cDeltaF, a flag and HM, bM, the marginalised frames with their priors and delta priors.
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

#include "WindowMarginalize.hpp" // includes WindowOptimize.hpp

using namespace dsm_host;

static uint64_t fnv1a(const void *p, size_t n, uint64_t hsh = 1469598103934665603ull) {
  for (size_t i = 0; i < n; i++) hsh = (hsh ^ ((const unsigned char *)p)[i]) * 1099511628211ull;
  return hsh;
}
template <typename T>
static bool rd(FILE *f, std::vector<T> &v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

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

// a window of a marginalize file: the prototype of its request, its planes, its points and its residuals
struct Case {
  int wh[2] = {0, 0};
  std::vector<float> planes;
  std::vector<ActivePointData> points;
  std::vector<ActiveResidualData> residuals;
  MarginalizeRequest proto;
  size_t nf = 0, npx = 0;
};

static bool load(const char *path, Case &c) {
  FILE *f = fopen(path, "rb");
  int nff[2] = {0, 0}, n_pts = 0, n_res = 0, has_hm = 0, nm = 0;
  float cal[6];
  std::vector<float> pre, prec, rrec, pin, cd;
  MarginalizeRequest &m = c.proto;
  LinearizeRequest &lin = m.hes.lin;
  bool good = f && fread(c.wh, sizeof(int), 2, f) == 2 && fread(cal, sizeof(float), 6, f) == 6 && fread(nff, sizeof(int), 2, f) == 2 && nff[0] >= 1 &&
              nff[0] <= DSM_WINDOW_MAX_FRAMES && c.wh[0] > 0 && c.wh[1] > 0;
  const size_t nf = good ? nff[0] : 0, npx = good ? (size_t)c.wh[0] * c.wh[1] : 0, N = 4 + 8 * nf;
  good = good && rd(f, lin.frame_ids, nf) && rd(f, c.planes, nf * npx) && rd(f, pre, nf * nf * 27) && rd(f, lin.frameEnergyTH, nf) &&
         fread(&n_pts, sizeof(int), 1, f) == 1 && n_pts >= 0 && rd(f, prec, (size_t)n_pts * 21) && fread(&n_res, sizeof(int), 1, f) == 1 && n_res >= 0 &&
         rd(f, rrec, (size_t)n_res * 5) && rd(f, m.hes.adHost, nf * nf * 64) && rd(f, m.hes.adTarget, nf * nf * 64) && rd(f, pin, (size_t)n_pts * 2);
  good = good && rd(f, m.flaggedForMarginalization, nf) && rd(f, m.numGoodResiduals, n_pts) && rd(f, m.lastResiduals, (size_t)n_pts * 2) &&
         rd(f, m.idepthHessian, n_pts) && rd(f, m.adHTdeltaF, nf * nf * 8) && rd(f, cd, 4) && fread(&has_hm, sizeof(int), 1, f) == 1 &&
         (!has_hm || (rd(f, m.HM, N * N) && rd(f, m.bM, N))) && fread(&nm, sizeof(int), 1, f) == 1 && nm >= 0 && nm <= (int)nf && rd(f, m.margFrames, nm) &&
         rd(f, m.framePrior, 8 * (size_t)nm) && rd(f, m.frameDeltaPrior, 8 * (size_t)nm);
  if (f) fclose(f);
  if (!good) return false;
  c.nf = nf, c.npx = npx;
  lin.fxl = cal[0], lin.fyl = cal[1], lin.cxl = cal[2], lin.cyl = cal[3], lin.fxli = cal[4], lin.fyli = cal[5];
  lin.fixLinearization = false, lin.wantJacobians = false;
  lin.precalc.resize(nf * nf);
  for (size_t p = 0; p < nf * nf; p++) {
    const float *q = &pre[27 * p];
    LinearizePrecalc &P = lin.precalc[p];
    memcpy(P.PRE_RTll_0, q, 36), memcpy(P.PRE_tTll_0, q + 9, 12), memcpy(P.PRE_KRKiTll, q + 12, 36), memcpy(P.PRE_KtTll, q + 21, 12);
    memcpy(P.PRE_aff_mode, q + 24, 8), P.PRE_b0_mode = q[26];
  }
  c.points.resize(n_pts);
  for (int i = 0; i < n_pts; i++) {
    const float *q = &prec[(size_t)21 * i];
    memcpy(&c.points[i].host, q, 4);
    c.points[i].u = q[1], c.points[i].v = q[2], c.points[i].idepth_scaled = q[3], c.points[i].idepth_zero_scaled = q[4];
    memcpy(c.points[i].color, q + 5, 32), memcpy(c.points[i].weights, q + 13, 32);
    m.hes.priorF.push_back(pin[2 * i]), m.hes.deltaF.push_back(pin[2 * i + 1]);
  }
  c.residuals.resize(n_res);
  for (int i = 0; i < n_res; i++) {
    const float *q = &rrec[(size_t)5 * i];
    int isnew;
    ActiveResidualData &r = c.residuals[i];
    memcpy(&r.point, q, 4), memcpy(&r.target, q + 1, 4), memcpy(&r.state_state, q + 2, 4);
    r.state_energy = q[3];
    memcpy(&isnew, q + 4, 4);
    r.isNew = isnew != 0;
  }
  memcpy(m.cDeltaF, cd.data(), 16);
  return true;
}

// ---- (2) the chain ----------------------------------------------------------------------------------------------------------------

// a window of a step file (as host/optimize_demo.cpp reads it): the prototype of its WindowOptimize, its planes and its points
struct StepCase {
  int wh[2] = {0, 0};
  std::vector<int> ids;
  std::vector<float> planes;
  std::vector<ActivePointData> points;
  WindowOptimize proto;
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
  WindowStep &w = c.proto.window;
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

struct Chain {
  std::string first, second; // the accept / reject patterns of the two optimisations
  uint64_t verdict = 0, HM = 0, bM = 0, state = 0, calib = 0, idepth = 0;
  int resInM = 0, kept = 0, residuals = 0;
  double last = 0;
};

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

// device: through the device forms; otherwise through the host forms (the requests still name a window; the host forms do not read it)
static Chain chain(const StepCase &S, dsm_context *ctx, bool device, int max_its) {
  Chain out;
  const size_t nf = S.nf, N = 4 + 8 * nf;
  const int leaves = nf > 1 ? 1 : 0;
  KeyframeWindow kw(ctx, S.wh[0], S.wh[1], (int)nf);
  std::vector<const float *> planes(nf);
  for (size_t k = 0; k < nf; k++) kw.put(S.ids[k], &S.planes[k * S.npx]), planes[k] = &S.planes[k * S.npx];
  WindowOptimize o = S.proto; // the first keyframe's optimisation
  o.maxIterations = max_its;
  o.window.req.hes.lin.window = &kw, o.window.req.hes.lin.points = &S.points;
  out.first = (device ? o.optimize(ctx) : o.optimizeHost(S.wh[0], S.wh[1], planes.data())).pattern;

  MarginalizeRequest m; // what makeKeyFrame does next, on the window's committed members
  m.fromWindow(o);
  const size_t n_pts = S.points.size();
  m.flaggedForMarginalization.assign(nf, 0), m.flaggedForMarginalization[leaves] = 1;
  m.numGoodResiduals.assign(n_pts, 9), m.lastResiduals.assign(2 * n_pts, DSM_RES_IN);
  m.margFrames.assign(1, leaves);
  for (int k = 0; k < 8; k++) m.framePrior.push_back(100.0 * (k + 1)), m.frameDeltaPrior.push_back(0.001 * (k + 1));
  if (device) marginalizeWindow(ctx, m);
  else marginalizeWindowHost(S.wh[0], S.wh[1], planes.data(), m);
  out.verdict = fnv1a(m.verdict.data(), m.verdict.size()), out.HM = fnv1a(m.HM_out.data(), 8 * m.HM_out.size());
  out.bM = fnv1a(m.bM_out.data(), 8 * m.bM_out.size()), out.resInM = m.resInM;

  // the next keyframe's window: the frame dropped, the points of verdict 0 and their residuals against the frames that stay
  std::vector<int> stay, new_frame(nf, -1), new_point(n_pts, -1), kept;
  for (size_t f = 0; f < nf; f++)
    if ((int)f != leaves) new_frame[f] = (int)stay.size(), stay.push_back((int)f);
  for (size_t p = 0; p < n_pts; p++)
    if (m.verdict[p] == 0) new_point[p] = (int)kept.size(), kept.push_back((int)p);
  kw.drop(S.ids[leaves]);
  std::vector<ActivePointData> points;
  WindowOptimize o2;
  WindowStep &w = o2.window, &was = o.window;
  HessianRequest &H = w.req.hes;
  for (int p : kept) {
    points.push_back(S.points[p]);
    points.back().host = new_frame[S.points[p].host];
    w.idepth.push_back(was.idepth[p]);
    H.priorF.push_back(was.req.hes.priorF[p]), H.Hdd_accLF.push_back(was.req.hes.Hdd_accLF[p]), H.bd_accLF.push_back(was.req.hes.bd_accLF[p]);
    H.Hcd_accLF.insert(H.Hcd_accLF.end(), was.req.hes.Hcd_accLF.begin() + 4 * p, was.req.hes.Hcd_accLF.begin() + 4 * p + 4);
  }
  for (const ActiveResidualData &r : was.residuals) // with the committed states
    if (new_point[r.point] >= 0 && new_frame[r.target] >= 0) {
      w.residuals.push_back(r);
      w.residuals.back().point = new_point[r.point], w.residuals.back().target = new_frame[r.target];
    }
  H.lin.window = &kw, H.lin.points = &points, H.lin.fixLinearization = false, H.lin.wantJacobians = false;
  H.lin.frame_ids = per_frame(S.ids, stay, 1);
  w.frameEnergyTH = per_frame(was.frameEnergyTH, stay, 1);
  H.shiftPriorToZero = was.req.hes.shiftPriorToZero;
  for (int h : stay)
    for (int t : stay) {
      const size_t at = ((size_t)h * nf + t) * 64;
      H.adHost.insert(H.adHost.end(), was.req.hes.adHost.begin() + at, was.req.hes.adHost.begin() + at + 64);
      H.adTarget.insert(H.adTarget.end(), was.req.hes.adTarget.begin() + at, was.req.hes.adTarget.begin() + at + 64);
    }
  w.req.H_L = cut(was.req.H_L, stay, N, true), w.req.b_L = cut(was.req.b_L, stay, N, false);
  w.req.HM = m.HM_out, w.req.bM = m.bM_out; // the returned prior
  w.prior = cut(was.prior, stay, N, false), w.priorZero = cut(was.priorZero, stay, N, false);
  w.worldToCamEval = per_frame(was.worldToCamEval, stay, 7), w.stateZero = per_frame(was.stateZero, stay, 8), w.exposure = per_frame(was.exposure, stay, 1);
  w.state = per_frame(was.state, stay, 8);
  memcpy(w.calib, was.calib, 32), memcpy(w.calibZero, was.calibZero, 32);
  o2.maxIterations = max_its;
  std::vector<const float *> planes2 = per_frame(planes, stay, 1);
  const OptimizeResult r2 = device ? o2.optimize(ctx) : o2.optimizeHost(S.wh[0], S.wh[1], planes2.data());
  out.second = r2.pattern, out.last = r2.lastEnergy + r2.lastEnergyM, out.kept = (int)kept.size(), out.residuals = (int)w.residuals.size();
  out.state = fnv1a(w.state.data(), 8 * w.state.size()), out.calib = fnv1a(w.calib, 32), out.idepth = fnv1a(w.idepth.data(), 4 * w.idepth.size());
  return out;
}

int main(int argc, char **argv) {
  if (argc < 4) {
    fprintf(stderr, "usage: marginalize_demo FILE_A FILE_B STEP_FILE [MAX_ITERATIONS]\n");
    return 2;
  }
  Case A, B;
  if (!load(argv[1], A) || !load(argv[2], B) || A.wh[0] != B.wh[0] || A.wh[1] != B.wh[1]) {
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
    KeyframeWindow wa(ctx, A.wh[0], A.wh[1], (int)A.nf), wb(ctx, B.wh[0], B.wh[1], (int)B.nf);
    for (size_t k = 0; k < A.nf; k++) wa.put(A.proto.hes.lin.frame_ids[k], &A.planes[k * A.npx]);
    for (size_t k = 0; k < B.nf; k++) wb.put(B.proto.hes.lin.frame_ids[k], &B.planes[k * B.npx]);
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
    std::vector<const float *> pa(A.nf), pb(B.nf);
    for (size_t k = 0; k < A.nf; k++) pa[k] = &A.planes[k * A.npx];
    for (size_t k = 0; k < B.nf; k++) pb[k] = &B.planes[k * B.npx];
    marginalizeWindowHost(A.wh[0], A.wh[1], pa.data(), ha);
    marginalizeWindowHost(B.wh[0], B.wh[1], pb.data(), hb);
    host_a = outcome(ha), host_b = outcome(hb);

    MarginalizeRequest d = request(A, &wa); // setDeltaF on a state that stands off its zero state
    std::vector<double> zero(8 * A.nf, 0.25), state(8 * A.nf);
    for (size_t i = 0; i < A.nf; i++)
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
