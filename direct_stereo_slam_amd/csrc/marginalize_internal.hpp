// marginalize_internal.hpp -- what both forms of the marginalisation call (marginalize_kernels.hip, marginalize_host.cpp) share on
// the host: the job rules (V) with the verdicts (C), the sub-window of M1 as a job of its own, and Z, the way its results go back
// to the window's arrays.  DESIGN.md section 21.
#pragma once
#include <vector>

#include "dsm_internal.hpp"

namespace dsm {

const char *marginalize_params_error(const dsm_marginalize_params *p);
// V of section 21, after linearize_job_error and hessian_job_error(J.hes, false) have passed; C for every point into `verdict`
// (the rules need the verdicts; the job's own array is not touched)
const char *marginalize_job_error(const dsm_marginalize_job &J, const dsm_marginalize_params &P, std::vector<unsigned char> &verdict);

// M1: the points of verdict 1 in ascending index with all their residuals in ascending index, every residual IN with energy 0, the
// prior scaled (A1'), shift_prior_to_zero 0, no linearised sums.  `job.hes` is a Hessian job like any other; its per-residual and
// per-point outputs point into the room below (only what the window's job asks for), H_A ... acc_bc, energy_out and
// new_frame_energy_th_out at the window job's own arrays.  The struct points into itself: build it where it stays.
struct MrgSub {
  std::vector<int> pts, res; // the window's index of every point and residual of the sub-window
  std::vector<int> host, point, target;
  std::vector<float> u, v, id, idz, color, wts, energy_in, prior, delta;
  std::vector<unsigned char> state_in;
  std::vector<unsigned char> new_state, active;
  std::vector<float> new_energy, new_ewo, cpt, proj, jp, hdd_acc, bd_acc, hcd_acc, hdi, bd_sum, idh;
  dsm_solve_job job; // only job.hes is filled: the solve pieces run the stitch alone
};
void marginalize_sub(const dsm_marginalize_job &J, const dsm_marginalize_params &P, const unsigned char *verdict, MrgSub &S);
// Z: the verdicts, the sub-window's per-residual and per-point results at the window's indices, n_res_marg
void marginalize_scatter(const dsm_marginalize_job &J, const unsigned char *verdict, const MrgSub &S);

} // namespace dsm
