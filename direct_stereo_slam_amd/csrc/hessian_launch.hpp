// hessian_launch.hpp -- the layout, the staging, the five launches and the unpacking of dsm_window_hessian_batch (hessian_kernels.hip) as
// pieces, for the two calls that run them: dsm_window_hessian_batch itself and dsm_window_solve_batch (solve_kernels.hip), whose own
// kernels read the records, the per-point results, the index lists and the raw accumulators where these pieces put them.
#pragma once
#include <vector>

#include "linearize_launch.hpp"

namespace dsm {

// a piece of the call arena: in the read-back part, or (the solve call, for what nobody asked for) in the device-only part
struct HesSpot {
  size_t at = 0;
  bool out = true;
  // 4-byte words from the start of the device-only part; the read-back part follows it at word out0
  long long word(long long out0) const { return (long long)(at / 4) + (out ? out0 : 0); }
};

struct HesWhere {
  size_t rows = 0, rec = 0, slot = 0; // bytes into work
  bool rows_out = false;
  size_t head = 0;                    // bytes into out
  HesSpot prec, top, D, E, EB, Hcc, bc;
  long long jp = -1, cpt = -1, proj = -1, J = -1; // bytes into out; -1: not asked for
};

// what the kernels of another call need of a job's device table: 4-byte words, the off_* into the staged inputs, the o_* from the
// start of the device-only part
struct HesView {
  int n_frames, n_pts, n_res;
  int off_pt_start, off_pt_list, off_target, off_host;
  long long o_rec, o_prec, o_top, o_D, o_E, o_EB, o_Hcc, o_bc;
};

struct HesPlan {
  std::vector<const dsm_hessian_job *> jobs;
  // lean: the call stitches on the device (dsm_window_solve_batch): the raw accumulators and the per-point results are read back only
  // for a job that asks for one of them, and hessian_unpack leaves H_A, b_A, H_sc, b_sc alone
  bool lean = false;
  size_t o_lin = 0, o_hes = 0, o_stage = 0;
  std::vector<HesWhere> at;
  std::vector<HesView> view;
  int max_res = 0, max_pts = 0, max_nf = 1;
  long long out0 = 0;
  const float *dev_stage = nullptr;
  float *dev_base = nullptr;
};

// takes the call's parts of A.in, A.work and A.out; before A.bind()
void hessian_layout(HesPlan &P, CallArena &A);
// fills the job tables and the staged inputs; after A.bind(), before A.upload()
void hessian_stage(HesPlan &P, CallArena &A);
// linearize_kernel and the four accumulation kernels on the context's stream
int hessian_launch(dsm_context *ctx, HesPlan &P, CallArena &A, const dsm_linearize_params &params);
// its two halves, for a call that rewrites the rows between them (dsm_window_marginalize_batch): linearize_kernel; the four others
int hessian_launch_linearize(dsm_context *ctx, HesPlan &P, CallArena &A, const dsm_linearize_params &params);
int hessian_launch_accumulate(dsm_context *ctx, HesPlan &P, CallArena &A);
// every output of the jobs from the read-back; after A.fetch()
void hessian_unpack(const HesPlan &P, const CallArena &A, const dsm_linearize_params &params);

} // namespace dsm
