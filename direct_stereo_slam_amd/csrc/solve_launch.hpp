// solve_launch.hpp -- the layout, the staging, the eight launches and the unpacking of dsm_window_solve_batch (solve_kernels.hip) as
// pieces, for the two calls that run them: dsm_window_solve_batch itself and dsm_window_step_batch (step_kernels.hip), whose own
// kernels write the trial state's tables where these pieces staged the job's.
#pragma once
#include <vector>

#include "hessian_launch.hpp"

namespace dsm {

struct SolWhere {
  HesSpot HA, bA, HS, bS;
  size_t x = 0, step = 0, flags = 0;    // bytes into out
  long long lastH = -1, lastb = -1; // bytes into out; -1: not asked for
};

// what the kernels of another call need of a job's device table: doubles into the staged doubles, -1: the job gave none
struct SolView {
  int N;
  long long d_HL, d_bL, d_HM, d_bM, d_dx;
};

struct SolPlan {
  std::vector<const dsm_solve_job *> jobs;
  HesPlan hes;
  size_t o_sol = 0, o_sd = 0;
  size_t sol_stride = 0, sol_lambda = 0; // bytes: one entry of the device job table at o_sol, and its double `lambda` within it
  std::vector<SolWhere> at;
  std::vector<SolView> view;
  int max_N = 12;
  // the jobs hold hes alone and the call runs the stitch alone (dsm_window_marginalize_batch): no room for the solve's inputs and
  // outputs is taken, and solve_unpack leaves them alone
  bool stitch_only = false;
};

// takes the call's parts of A.in, A.work and A.out (the Hessian pieces' among them); before A.bind()
void solve_layout(SolPlan &P, CallArena &A);
// fills the job tables and the staged inputs; after A.bind(), before A.upload()
void solve_stage(SolPlan &P, CallArena &A);
// the five launches of hessian_launch and the three of the solve on the context's stream
int solve_launch(dsm_context *ctx, SolPlan &P, CallArena &A, const dsm_linearize_params &params);
// its pieces: hessian_launch is the first; the stitch (T1d) of the raw accumulators into H_A, b_A, H_sc, b_sc where the plan put them
int solve_launch_stitch(dsm_context *ctx, SolPlan &P, CallArena &A);
// every output of the jobs from the read-back; after A.fetch()
void solve_unpack(const SolPlan &P, const CallArena &A, const dsm_linearize_params &params);

} // namespace dsm
