// marginalize_host.cpp -- the host form of the marginalisation of points and frames (dsm_window_marginalize_host, DESIGN.md section
// 21) and what both forms share on the host: the job rules (V) with the verdicts (C), the sub-window (M1) and the way its results go
// back (Z).  The host form is dsm_window_hessian_host on the sub-window with X1 between its linearisation and its accumulation, then
// plain loops over M2 and G1-G7; the expressions are marginalize_math.hpp, shared with the device kernels (marginalize_kernels.hip),
// which must equal it bit for bit.  Plain C++; no device code.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "marginalize_internal.hpp"
#include "marginalize_math.hpp"

extern "C" int dsm_marginalize_params_default(dsm_marginalize_params *p) {
  if (!p) return DSM_ERR_INVALID;
  p->min_good_active_res_for_marg = 3, p->min_good_res_for_marg = 4;
  p->min_idepth_h_marg = 50.0f, p->marg_weight_fac = 0.25f, p->idepth_fix_prior_marg_fac = 600.0f * 600.0f;
  return DSM_OK;
}

namespace dsm {

const char *marginalize_params_error(const dsm_marginalize_params *p) {
  if (!p) return "no marginalisation parameters";
  if (!std::isfinite(p->min_idepth_h_marg) || !std::isfinite(p->marg_weight_fac) || !std::isfinite(p->idepth_fix_prior_marg_fac))
    return "a non-finite marginalisation parameter";
  if (p->min_good_active_res_for_marg < 0 || p->min_good_res_for_marg < 0) return "a negative count among the marginalisation parameters";
  return nullptr;
}

const char *marginalize_job_error(const dsm_marginalize_job &J, const dsm_marginalize_params &P, std::vector<unsigned char> &verdict) {
  const dsm_linearize_job &L = J.hes.lin;
  const int nf = L.n_frames, np = L.n_pts, nr = L.n_res;
  const size_t N = 4 + 8 * (size_t)nf;
  if (L.J_out || L.keep || L.rel_bs) return "lin.J_out, keep or rel_bs given";
  if (L.fix_linearization) return "lin.fix_linearization is not 0";
  if (!J.flagged || !J.ad_ht_delta || !J.c_delta || !J.H_M_out || !J.b_M_out || !J.n_res_marg) return "a NULL required array";
  if (np && (!J.n_good_residuals || !J.last_state || !J.idepth_hessian || !J.verdict)) return "a NULL per-point array";
  auto finite_f = [](const float *a, size_t n) {
    for (size_t i = 0; a && i < n; i++)
      if (!std::isfinite(a[i])) return false;
    return true;
  };
  auto finite_d = [](const double *a, size_t n) {
    for (size_t i = 0; a && i < n; i++)
      if (!std::isfinite(a[i])) return false;
    return true;
  };
  for (int i = 0; i < 2 * np; i++)
    if (J.last_state[i] != DSM_RES_IN && J.last_state[i] != DSM_RES_OOB && J.last_state[i] != DSM_RES_OUTLIER) return "a last_state that is no residual state";
  if (!finite_f(J.idepth_hessian, np) || !finite_f(J.ad_ht_delta, (size_t)nf * nf * 8) || !finite_f(J.c_delta, 4))
    return "a non-finite idepth_hessian, ad_ht_delta or c_delta";
  if (!finite_d(J.H_M, N * N) || !finite_d(J.b_M, N)) return "a non-finite H_M or b_M";
  if (J.n_marg_frames < 0 || J.n_marg_frames > nf) return "n_marg_frames outside [0, n_frames]";
  if (J.n_marg_frames && (!J.marg_frames || !J.frame_prior || !J.frame_delta_prior)) return "NULL marg_frames, frame_prior or frame_delta_prior";
  for (int m = 0; m < J.n_marg_frames; m++) {
    const int f = J.marg_frames[m];
    if (f < 0 || f >= nf || (m && f <= J.marg_frames[m - 1])) return "marg_frames out of range or not strictly ascending";
    if (!J.flagged[f]) return "a marginalised frame that is not flagged";
  }
  if (!finite_d(J.frame_prior, 8 * (size_t)J.n_marg_frames) || !finite_d(J.frame_delta_prior, 8 * (size_t)J.n_marg_frames))
    return "a non-finite frame_prior or frame_delta_prior";
  // C
  std::vector<int> k((size_t)np, 0), vis((size_t)np, 0);
  for (int r = 0; r < nr; r++) {
    k[L.point[r]]++;
    if (L.state_in[r] == DSM_RES_IN && J.flagged[L.target[r]]) vis[L.point[r]]++;
  }
  verdict.resize((size_t)np);
  for (int p = 0; p < np; p++)
    verdict[p] = (unsigned char)mrg::verdict(L.idepth_scaled[p], k[p], vis[p], J.n_good_residuals[p], J.last_state[2 * p], J.last_state[2 * p + 1],
                                             J.flagged[L.host[p]] != 0, J.idepth_hessian[p], P.min_good_active_res_for_marg,
                                             P.min_good_res_for_marg, P.min_idepth_h_marg);
  std::vector<unsigned char> leaves((size_t)nf, 0);
  for (int m = 0; m < J.n_marg_frames; m++) leaves[J.marg_frames[m]] = 1;
  for (int p = 0; p < np; p++)
    if (verdict[p] == mrg::KEEP && leaves[L.host[p]]) return "a marginalised frame that still hosts a point of verdict 0";
  return nullptr;
}

void marginalize_sub(const dsm_marginalize_job &J, const dsm_marginalize_params &P, const unsigned char *verdict, MrgSub &S) {
  const dsm_hessian_job &H = J.hes;
  const dsm_linearize_job &L = H.lin;
  std::vector<int> sub_of((size_t)L.n_pts, -1);
  for (int p = 0; p < L.n_pts; p++)
    if (verdict[p] == mrg::MARGINALIZE) sub_of[p] = (int)S.pts.size(), S.pts.push_back(p);
  for (int r = 0; r < L.n_res; r++)
    if (sub_of[L.point[r]] >= 0) S.res.push_back(r);
  const size_t n = S.pts.size(), nr = S.res.size();
  S.host.resize(n), S.u.resize(n), S.v.resize(n), S.id.resize(n), S.idz.resize(n), S.color.resize(8 * n), S.wts.resize(8 * n);
  S.prior.resize(n), S.delta.resize(n);
  for (size_t i = 0; i < n; i++) {
    const int p = S.pts[i];
    S.host[i] = L.host[p], S.u[i] = L.u[p], S.v[i] = L.v[p], S.id[i] = L.idepth_scaled[p], S.idz[i] = L.idepth_zero_scaled[p];
    memcpy(&S.color[8 * i], L.color + 8 * (size_t)p, 32), memcpy(&S.wts[8 * i], L.weights + 8 * (size_t)p, 32);
    S.prior[i] = (H.prior ? H.prior[p] : 0.0f) * P.idepth_fix_prior_marg_fac; // A1'
    S.delta[i] = H.delta ? H.delta[p] : 0.0f;
  }
  S.point.resize(nr), S.target.resize(nr), S.state_in.assign(nr, DSM_RES_IN), S.energy_in.assign(nr, 0.0f); // resetOOB
  for (size_t i = 0; i < nr; i++) S.point[i] = sub_of[L.point[S.res[i]]], S.target[i] = L.target[S.res[i]];
  S.new_state.resize(nr + 1), S.new_energy.resize(nr + 1), S.new_ewo.resize(nr + 1);
  memset(&S.job, 0, sizeof S.job);
  dsm_hessian_job &G = S.job.hes;
  G = H;
  dsm_linearize_job &D = G.lin;
  D.n_pts = (int)n, D.host = S.host.data(), D.u = S.u.data(), D.v = S.v.data(), D.idepth_scaled = S.id.data(), D.idepth_zero_scaled = S.idz.data();
  D.color = S.color.data(), D.weights = S.wts.data();
  D.n_res = (int)nr, D.point = S.point.data(), D.target = S.target.data(), D.state_in = S.state_in.data(), D.energy_in = S.energy_in.data();
  D.is_new = nullptr, D.fix_linearization = 0;
  D.new_state = S.new_state.data(), D.new_energy = S.new_energy.data(), D.new_energy_with_outlier = S.new_ewo.data();
  auto room = [](std::vector<float> &v, const float *asked, size_t count) { return asked ? (v.resize(count + 1), v.data()) : nullptr; };
  D.center_projected_to = room(S.cpt, L.center_projected_to, 3 * nr), D.projected_to = room(S.proj, L.projected_to, 16 * nr);
  G.prior = S.prior.data(), G.delta = S.delta.data(), G.hdd_lin = G.bd_lin = G.hcd_lin = nullptr, G.shift_prior_to_zero = 0;
  S.active.resize(nr + 1), G.active = S.active.data();
  G.JpJdF = room(S.jp, H.JpJdF, 8 * nr);
  G.hdd_acc = room(S.hdd_acc, H.hdd_acc, n), G.bd_acc = room(S.bd_acc, H.bd_acc, n), G.hcd_acc = room(S.hcd_acc, H.hcd_acc, 4 * n);
  G.hdi = room(S.hdi, H.hdi, n), G.bd_sum = room(S.bd_sum, H.bd_sum, n), G.idepth_hessian = room(S.idh, H.idepth_hessian, n);
}

void marginalize_scatter(const dsm_marginalize_job &J, const unsigned char *verdict, const MrgSub &S) {
  const dsm_hessian_job &H = J.hes, &G = S.job.hes;
  const dsm_linearize_job &L = H.lin;
  if (L.n_pts) memcpy(J.verdict, verdict, (size_t)L.n_pts);
  int n_marg = 0;
  for (size_t i = 0; i < S.res.size(); i++) {
    const size_t r = (size_t)S.res[i];
    const int state = S.new_state[i];
    L.new_state[r] = S.new_state[i], L.new_energy[r] = S.new_energy[i], L.new_energy_with_outlier[r] = S.new_ewo[i];
    if (state != DSM_RES_OOB) { // L8
      if (L.center_projected_to) memcpy(L.center_projected_to + 3 * r, &S.cpt[3 * i], 12);
      if (L.projected_to) memcpy(L.projected_to + 16 * r, &S.proj[16 * i], 64);
    }
    if (H.active) H.active[r] = S.active[i];
    if (S.active[i] && H.JpJdF) memcpy(H.JpJdF + 8 * r, &S.jp[8 * i], 32);
    n_marg += S.active[i] != 0;
  }
  for (size_t i = 0; i < S.pts.size(); i++) {
    const size_t p = (size_t)S.pts[i];
    if (H.hdd_acc) H.hdd_acc[p] = G.hdd_acc[i];
    if (H.bd_acc) H.bd_acc[p] = G.bd_acc[i];
    if (H.hcd_acc) memcpy(H.hcd_acc + 4 * p, G.hcd_acc + 4 * i, 16);
    if (H.hdi) H.hdi[p] = G.hdi[i];
    if (H.bd_sum) H.bd_sum[p] = G.bd_sum[i];
    if (H.idepth_hessian) H.idepth_hessian[p] = G.idepth_hessian[i];
  }
  *J.n_res_marg = n_marg;
}

} // namespace dsm

namespace {

struct FixHook { // X1 on the rows of the sub-window's active residuals
  const dsm_marginalize_job *J;
  const dsm::MrgSub *S;
};
void fix_rows(void *user, const dsm_linearize_job &L, float *rows) {
  const FixHook &F = *(const FixHook *)user;
  const int nf = L.n_frames;
  for (int i = 0; i < L.n_res; i++) {
    if (L.new_state[i] != DSM_RES_IN) continue; // A0: every residual of the sub-window enters IN
    const int p = L.point[i];
    float *row = rows + (size_t)dsm::lin::J_FLOATS * i;
    dsm::mrg::res_to_zero(row, F.J->ad_ht_delta + 8 * ((size_t)L.host[p] * nf + L.target[i]), F.J->c_delta, F.S->delta[p], row + dsm::lin::J_RESF);
    if (F.J->res_to_zero) memcpy(F.J->res_to_zero + 8 * (size_t)F.S->res[i], row + dsm::lin::J_RESF, 32);
  }
}

// G1-G7 for one frame (current index f) of the N x N system H, b; the (N - 8) system into Ho, bo
void marginalize_frame(int N, const double *H, const double *b, int f, const double *prior, const double *delta_prior, double *Ho, double *bo) {
  using namespace dsm::mrg;
  const int nd = N - 8;
  std::vector<double> Hs((size_t)N * N), bs(N), S(N), SI(N), bli((size_t)nd * 8);
  for (int i = 0; i < N; i++) { // G1
    const int si = source_index(i, f, N);
    bs[i] = b[si];
    for (int j = 0; j < N; j++) Hs[(size_t)i * N + j] = H[(size_t)si * N + source_index(j, f, N)];
  }
  for (int k = 0; k < 8; k++) { // G2
    Hs[(size_t)(nd + k) * N + nd + k] += prior[k];
    bs[nd + k] += prior[k] * delta_prior[k];
  }
  for (int i = 0; i < N; i++) S[i] = scale_of(Hs[(size_t)i * N + i]), SI[i] = scale_inverse(S[i]); // G3
  for (int i = 0; i < N; i++) {                                                                    // G4
    for (int j = 0; j < N; j++) Hs[(size_t)i * N + j] = scaled(SI[i], Hs[(size_t)i * N + j], SI[j]);
    bs[i] = SI[i] * bs[i];
  }
  double a[64], P[64], y[8];
  int piv[8];
  for (int i = 0; i < 8; i++)
    for (int j = 0; j < 8; j++) a[8 * i + j] = Hs[(size_t)(nd + i) * N + nd + j];
  lu_inverse8(a, P, piv, y); // G5
  const double *bottom = Hs.data() + (size_t)nd * N;
  for (int i = 0; i < nd; i++) // G6
    for (int k = 0; k < 8; k++) bli[8 * (size_t)i + k] = bli_entry(bottom + i, N, P + k);
  for (int i = 0; i < nd; i++) {
    for (int j = 0; j < nd; j++) Hs[(size_t)i * N + j] = schur_entry(Hs[(size_t)i * N + j], &bli[8 * (size_t)i], bottom + j, N);
    bs[i] = schur_entry(bs[i], &bli[8 * (size_t)i], bs.data() + nd, 1);
  }
  for (int i = 0; i < nd; i++) { // G7
    for (int j = 0; j < nd; j++)
      Ho[(size_t)i * nd + j] = symmetrised(scaled(S[i], Hs[(size_t)i * N + j], S[j]), scaled(S[j], Hs[(size_t)j * N + i], S[i]));
    bo[i] = S[i] * bs[i];
  }
}

} // namespace

extern "C" int dsm_window_marginalize_host(int w, int h, const dsm_marginalize_job *job, const float *const *frame_I,
                                           const dsm_linearize_params *lin_params, const dsm_marginalize_params *marg_params) {
  using namespace dsm;
  auto fail = [](const char *msg) {
    set_error(std::string("dsm_window_marginalize_host: ") + msg);
    return DSM_ERR_INVALID;
  };
  if (w < 8 || h < 8 || !job || !frame_I) return fail("bad argument");
  if (const char *e = linearize_params_error(lin_params)) return fail(e);
  if (const char *e = marginalize_params_error(marg_params)) return fail(e);
  if (const char *e = linearize_job_error(job->hes.lin)) return fail(e);
  if (const char *e = hessian_job_error(job->hes, false)) return fail(e);
  std::vector<unsigned char> verdict;
  if (const char *e = marginalize_job_error(*job, *marg_params, verdict)) return fail(e);
  const dsm_marginalize_job &J = *job;
  const int nf = J.hes.lin.n_frames, N = 4 + 8 * nf;
  for (int f = 0; f < nf; f++)
    if (!frame_I[f]) return fail("NULL frame");
  MrgSub S;
  marginalize_sub(J, *marg_params, verdict.data(), S);
  dsm_hessian_job &G = S.job.hes;
  std::vector<double> HA, bA, HS, bS; // room of our own for what the job does not ask for
  if (!G.H_A) HA.resize((size_t)N * N), G.H_A = HA.data();
  if (!G.b_A) bA.resize(N), G.b_A = bA.data();
  if (!G.H_sc) HS.resize((size_t)N * N), G.H_sc = HS.data();
  if (!G.b_sc) bS.resize(N), G.b_sc = bS.data();
  FixHook hook{&J, &S};
  if (int rc = hessian_host_run(w, h, &G, frame_I, lin_params, fix_rows, &hook)) return rc;
  marginalize_scatter(J, verdict.data(), S);
  std::vector<double> H((size_t)N * N), b(N), Hn, bn;
  const double wt = (double)marg_params->marg_weight_fac;
  for (size_t e = 0; e < (size_t)N * N; e++) H[e] = mrg::fold(J.H_M ? J.H_M[e] : 0.0, wt, G.H_A[e], G.H_sc[e]); // M2
  for (int i = 0; i < N; i++) b[i] = mrg::fold(J.b_M ? J.b_M[i] : 0.0, wt, G.b_A[i], G.b_sc[i]);
  if (J.H_M_points) memcpy(J.H_M_points, H.data(), 8 * (size_t)N * N);
  if (J.b_M_points) memcpy(J.b_M_points, b.data(), 8 * (size_t)N);
  int n = N;
  for (int m = 0; m < J.n_marg_frames; m++, n -= 8) { // G, frame after frame on the previous result, the indices renumbered
    Hn.assign((size_t)(n - 8) * (n - 8), 0.0), bn.assign(n - 8, 0.0);
    marginalize_frame(n, H.data(), b.data(), J.marg_frames[m] - m, J.frame_prior + 8 * m, J.frame_delta_prior + 8 * m, Hn.data(), bn.data());
    H.swap(Hn), b.swap(bn);
  }
  memcpy(J.H_M_out, H.data(), 8 * (size_t)n * n), memcpy(J.b_M_out, b.data(), 8 * (size_t)n);
  return DSM_OK;
}
