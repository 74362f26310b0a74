// optimize_launch.hpp -- the checks, the layout, the staging, the passes and the unpacking of dsm_window_optimize_batch
// (optimize_kernels.hip) as pieces, for the two calls that run them: dsm_window_optimize_batch itself and dsm_window_finish_batch
// (finish_kernels.hip), whose own kernels read what the loop's last pass left and write a region of their own.
#pragma once
#include <vector>

#include "step_launch.hpp"

#include "optimize_math.hpp"

namespace dsm {

struct OptPlan {
  int n_jobs = 0, max_it = 0;
  std::vector<const dsm_optimize_job *> jobs;
  std::vector<double> zero;        // pass 0's steps
  std::vector<dsm_step_job> first; // the jobs as the step call's rules and pieces see pass 0
  StpPlan stp;
  std::vector<size_t> log, keys; // per job: bytes into out (its state, mirrored after every pass) and into work (the select's list)
  size_t o_opt = 0, o_states = 0, o_keep = 0, doubles = 0, max_lanes = 0;
};

// all-or-nothing validation of a batch (`call` names the entry point in the message); fills the plan's jobs
int optimize_check(const char *call, dsm_context *ctx, int n_jobs, const dsm_optimize_job *const *jobs, const dsm_linearize_params *lp,
                   const dsm_step_params *sp, const dsm_optimize_params *op, OptPlan &P);
// takes the call's parts of A.in, A.work and A.out (the step pieces' among them); before A.bind()
void optimize_layout(OptPlan &P, CallArena &A);
// fills the job tables, the states and the staged inputs; after A.bind(), before A.upload()
void optimize_stage(OptPlan &P, CallArena &A, const dsm_optimize_params &op);
// `count` passes back to back on the context's stream
int optimize_passes(dsm_context *ctx, OptPlan &P, CallArena &A, const dsm_linearize_params &lp, const dsm_step_params &sp, int count);
// the jobs that the read-back shows unfinished; after A.fetch()
int optimize_unfinished(const OptPlan &P, const CallArena &A);
// every output of the jobs from the read-back; after A.fetch()
void optimize_unpack(const OptPlan &P, const CallArena &A, const dsm_linearize_params &lp);
// the device's array of the jobs' states (opt::State), in job order
inline const opt::State *optimize_dev_states(const OptPlan &P, const CallArena &A) { return A.dev_in<const opt::State>(P.o_states); }

} // namespace dsm
