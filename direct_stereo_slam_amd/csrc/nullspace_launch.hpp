// nullspace_launch.hpp -- what the two forms of the nullspace call (nullspace_kernels.hip, nullspace_host.cpp) share on the host: the
// rules V of DESIGN.md section 23 and the parameters as the expressions of nullspace_math.hpp take them.
#pragma once
#include "dsm_internal.hpp"
#include "nullspace_math.hpp"

namespace dsm {

const char *nullspace_params_error(const dsm_nullspace_params *p);
const char *nullspace_job_error(const dsm_nullspace_job &J);
// V for the whole call (ctx apart); P: the caller's parameters, or the defaults for NULL
int nullspace_check(const char *call, int n_jobs, const dsm_nullspace_job *jobs, const dsm_nullspace_params *params, dsm_nullspace_params &P);
nsp::Scales nullspace_scales(const dsm_nullspace_params &P);

} // namespace dsm
