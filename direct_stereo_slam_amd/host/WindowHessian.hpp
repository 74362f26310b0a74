// WindowHessian.hpp -- C++ host adaptor for what FrontEnd::optimize (dso_helpers/FrontEndOptimize.cpp:332-486) does between
// linearizeAll and the solve: accumulateAF_MT and accumulateSCF_MT over the active residuals of a window (AccumulatedTopHessianSSE /
// AccumulatedSCHessianSSE::addPoint per point and stitchDouble), as ONE call together with the linearisation of the same pass, for one
// window or for the windows of many sequences, on top of the C ABI (include/dsm_hotpath.h).  Header-only, plain C++11.
// Semantics: DESIGN.md section 17 (A0-A3, P1, S1-S3, T1).  The call is stateless: a rejected trial step discards what came back.
#pragma once
#include "ResidualLinearizer.hpp"

namespace dsm_host {

// One window: the linearisation's request (lin.wantJacobians is normally false: the rows stay on the device) and what the
// accumulation reads on top.  The per-point vectors may be empty (zeros).
struct HessianRequest {
  LinearizeRequest lin;
  std::vector<double> adHost, adTarget; // EF->adHost / adTarget: n_frames * n_frames blocks of 8 x 8, [host][target], row-major
  std::vector<float> priorF, deltaF;    // per point
  std::vector<float> Hdd_accLF, bd_accLF, Hcd_accLF; // per point (Hcd_accLF: 4 each): the sums over the linearised residuals
  bool shiftPriorToZero = true;

  // results: N = 4 + 8 n_frames
  std::vector<double> H_A, b_A;   // accumulateAF
  std::vector<double> H_sc, b_sc; // accumulateSCF
  std::vector<unsigned char> isActive; // per residual
  std::vector<float> JpJdF;            // per residual 8 floats, of the active ones: what resubstituteFPt reads
  std::vector<float> HdiF, bdSumF, idepth_hessian; // per point

  void accumulateAF(std::vector<double> &H, std::vector<double> &b) const { H = H_A, b = b_A; }
  void accumulateSCF(std::vector<double> &H, std::vector<double> &b) const { H = H_sc, b = b_sc; }
};

namespace hessian_detail {
inline dsm_hessian_job flatten(linearize_detail::Flat &f, HessianRequest &r) {
  dsm_hessian_job j;
  memset(&j, 0, sizeof j);
  j.lin = linearize_detail::flatten(f, r.lin);
  const size_t nf = r.lin.frame_ids.size(), n = r.lin.points->size(), nr = r.lin.residuals->size(), N = 4 + 8 * nf;
  auto sized = [](const std::vector<float> &v, size_t want) {
    if (!v.empty() && v.size() != want) throw std::invalid_argument("accumulateWindow: a per-point array of the wrong length");
    return v.empty() ? nullptr : v.data();
  };
  if (r.adHost.size() != nf * nf * 64 || r.adTarget.size() != nf * nf * 64) throw std::invalid_argument("accumulateWindow: adHost / adTarget");
  j.ad_host = r.adHost.data(), j.ad_target = r.adTarget.data();
  j.prior = sized(r.priorF, n), j.delta = sized(r.deltaF, n);
  j.hdd_lin = sized(r.Hdd_accLF, n), j.bd_lin = sized(r.bd_accLF, n), j.hcd_lin = sized(r.Hcd_accLF, 4 * n);
  j.shift_prior_to_zero = r.shiftPriorToZero ? 1 : 0;
  r.H_A.assign(N * N, 0.0), r.b_A.assign(N, 0.0), r.H_sc.assign(N * N, 0.0), r.b_sc.assign(N, 0.0);
  r.isActive.assign(nr + 1, 0), r.JpJdF.assign(8 * nr + 1, 0.f), r.HdiF.assign(n + 1, 0.f), r.bdSumF.assign(n + 1, 0.f), r.idepth_hessian.assign(n + 1, 0.f);
  j.H_A = r.H_A.data(), j.b_A = r.b_A.data(), j.H_sc = r.H_sc.data(), j.b_sc = r.b_sc.data();
  j.active = r.isActive.data(), j.JpJdF = r.JpJdF.data(), j.hdi = r.HdiF.data(), j.bd_sum = r.bdSumF.data(), j.idepth_hessian = r.idepth_hessian.data();
  return j;
}
inline void unpack(const linearize_detail::Flat &f, HessianRequest &r) {
  linearize_detail::unpack(f, r.lin);
  r.isActive.pop_back(), r.JpJdF.pop_back(), r.HdiF.pop_back(), r.bdSumF.pop_back(), r.idepth_hessian.pop_back();
}
} // namespace hessian_detail

// linearizeAll + accumulateAF_MT + accumulateSCF_MT for the windows of many sequences in ONE call; every window must have the same
// image size.  Fills the results of every request.  params: null = the upstream defaults.
inline void accumulateWindows(dsm_context *ctx, std::vector<HessianRequest> &reqs, const dsm_linearize_params *params = nullptr) {
  if (reqs.empty()) return;
  dsm_linearize_params defaults;
  dsm_linearize_params_default(&defaults);
  std::vector<linearize_detail::Flat> flat(reqs.size());
  std::vector<dsm_hessian_job> jobs(reqs.size());
  for (size_t i = 0; i < reqs.size(); i++) jobs[i] = hessian_detail::flatten(flat[i], reqs[i]);
  immature_check(dsm_window_hessian_batch(ctx, (int)jobs.size(), jobs.data(), params ? params : &defaults), "accumulateWindows");
  for (size_t i = 0; i < reqs.size(); i++) hessian_detail::unpack(flat[i], reqs[i]);
}

// ... and for one window
inline void accumulateWindow(dsm_context *ctx, HessianRequest &req, const dsm_linearize_params *params = nullptr) {
  dsm_linearize_params defaults;
  dsm_linearize_params_default(&defaults);
  linearize_detail::Flat flat;
  dsm_hessian_job job = hessian_detail::flatten(flat, req);
  immature_check(dsm_window_hessian_batch(ctx, 1, &job, params ? params : &defaults), "accumulateWindow");
  hessian_detail::unpack(flat, req);
}

} // namespace dsm_host
