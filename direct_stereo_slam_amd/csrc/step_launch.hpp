// step_launch.hpp -- the checks, the layout, the staging, the ten launches and the unpacking of dsm_window_step_batch (step_kernels.hip)
// as pieces, for the two calls that run them: dsm_window_step_batch itself and dsm_window_optimize_batch (optimize_kernels.hip), whose
// own kernels write the next pass's inputs where these pieces staged the job's.
#pragma once
#include <vector>

#include "solve_launch.hpp"

namespace dsm {

struct StpWhere {
  size_t state = 0, calib = 0, idepth = 0, W = 0, can = 0, sums = 0, em = 0; // bytes into out
  long long C = -1, cam = -1, pre = -1, dx = -1, HL = -1, bL = -1;        // bytes into out; -1: not asked for
};

// what the kernels of another call need of a job's device table: doubles into the step's staged doubles (q_*; q_prior -1: no prior),
// 4-byte words into its staged floats (f_*), 4-byte words from the start of the arena's device-only part (o_*)
struct StpView {
  int q_backup, q_step, q_cbackup, q_cstep, q_prior;
  int f_idb, f_ids;
  long long o_state, o_calib, o_idepth, o_em, o_can, o_W;
};

struct StpPlan {
  int n_jobs = 0;
  const dsm_step_job *jobs = nullptr;
  std::vector<double> zero;     // the placeholders of what the device forms
  std::vector<dsm_solve_job> T; // the jobs completed with them, as the solve call's rules and pieces see them
  SolPlan sol;
  std::vector<StpWhere> at;
  std::vector<StpView> view;
  size_t o_stp = 0, o_sq = 0, o_sf = 0; // bytes into in: the job table, the staged doubles, the staged floats
  size_t stp_stride = 0, stp_stepfac = 0; // bytes: one entry of the job table, and its stepfac[5] within it
  size_t doubles = 0, floats = 0;
  int max_pts = 0;
};

// all-or-nothing validation of a batch (`call` names the entry point in the message); fills P.jobs, P.zero and P.T
int step_check(const char *call, dsm_context *ctx, int n_jobs, const dsm_step_job *jobs, const dsm_linearize_params *lp, const dsm_step_params *sp,
               StpPlan &P);
// takes the call's parts of A.in, A.work and A.out (the solve pieces' among them); before A.bind()
void step_layout(StpPlan &P, CallArena &A);
// fills the job tables and the staged inputs; after A.bind(), before A.upload()
void step_stage(StpPlan &P, CallArena &A);
// stp_frame_kernel, stp_point_kernel and the eight launches of solve_launch on the context's stream: one pass
int step_launch(dsm_context *ctx, StpPlan &P, CallArena &A, const dsm_linearize_params &lp, const dsm_step_params &sp);
// every output of the jobs from the read-back; after A.fetch()
void step_unpack(const StpPlan &P, const CallArena &A, const dsm_linearize_params &lp);

} // namespace dsm
