// linearize_launch.hpp -- the staging, the launch and the unpacking of linearize_kernel (linearize_kernels.hip) as pieces, for the two
// calls that run it: dsm_linearize_residuals_batch and dsm_window_hessian_batch (hessian_kernels.hip), whose own kernels read the same
// staged job table, the heads and the rows.
#pragma once
#include <vector>

#include "call_arena.hpp"
#include "linearize_math.hpp"

namespace dsm {

constexpr int kLinHeadWords = 4; // per residual: new_state | keep << 8, new_energy, new_energy_with_outlier, rel_bs

struct LinJob {
  const float *plane[DSM_WINDOW_MAX_FRAMES]; // level-0 planes in frame_ids order
  float fx, fy, cx, cy, fxi, fyi;
  int n_frames, n_res, fix;
  // 4-byte words into the staged inputs
  int off_R0, off_t0, off_M, off_Kt, off_aff, off_b0, off_eth, off_host, off_u, off_v, off_id, off_idz, off_color, off_wt, off_point, off_target,
      off_ein, off_flags;
  long long o_head, o_J, o_cpt, o_proj; // 4-byte words into the output; -1: the job does not ask for it
};

// all-or-nothing validation of a batch (`call` names the entry point in the message); the residuals of the call into *res_out
int linearize_check_jobs(const char *call, dsm_context *ctx, int n_jobs, const dsm_linearize_job *const *jobs, const dsm_linearize_params *params,
                         size_t *res_out);
// 4-byte words that linearize_stage packs for the job
size_t linearize_stage_words(const dsm_linearize_job &J);
// fills the job table entry D (its o_* from the caller) and packs the job's inputs at W; returns nothing the caller has to keep
void linearize_stage(const dsm_linearize_job &J, LinJob &D, WordPacker &W);
// one launch over the jobs; `out` is what the o_* count their words from
int linearize_launch(dsm_context *ctx, int n_jobs, int max_res, const LinJob *dev_jobs, const float *dev_stage, float *out, int w, int h,
                     const dsm_linearize_params &params);
// the heads of job J from the read-back (B3 included), and the optional arrays from where the o_* (words from ho) put them
void linearize_unpack(const dsm_linearize_job &J, const float *ho, long long o_head, long long o_cpt, long long o_proj, long long o_J);

} // namespace dsm
