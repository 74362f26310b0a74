// rescale_launch.hpp -- what the two forms of the rescale call (rescale_kernels.hip, rescale_host.cpp) share on the host: the rules V
// of DESIGN.md section 25, the decisions (S0, S1), the byte copies of a job that is not accepted (S6) and the launch geometry.
#pragma once
#include "dsm_internal.hpp"
#include "rescale_math.hpp"

namespace dsm {

constexpr int kRscBlock = 256;     // rsc_kernel's workgroup
constexpr int kRscPointBlocks = 8; // at most this many workgroups stride over a job's points

const char *rescale_job_error(const dsm_rescale_job &J);
// V for the whole call (ctx apart); LP, SP: the caller's parameters, or the defaults for NULL
int rescale_check(const char *call, int n_jobs, const dsm_rescale_job *jobs, const dsm_linearize_params *lp, const dsm_step_params *sp,
                  dsm_linearize_params &LP, dsm_step_params &SP);
stp::Scales rescale_scales(const dsm_linearize_params &LP, const dsm_step_params &SP);
// S0, S1 of one job, written to its five words; returns the decision
int rescale_decide(const dsm_rescale_job &J);
// S6: every array output is a byte copy of its input
void rescale_copy_through(const dsm_rescale_job &J);

} // namespace dsm
