// form_launch.hpp -- the launch-per-step form of the tracker kernels (a part of tracker_kernels.hip, see the map at the top of that
// file): eval_kernel (grid = chunks x problems, optionally with the fused LM step) and lm_kernel (start, step, the single evaluations
// of dsm_tracker_calc_res_*), each with its launcher.  lm_start_problem is here because lm_kernel's LM_OP_START is its first user;
// the tick engine's admission calls it too.
#pragma once

namespace dsm {

// ------------------------------------------------------------------------------------------
// eval kernel: grid (chunk slots, problems).
// LVL0 = true is the level-0 instantiation (adds the flow indicators); it is also the dominant kernel
// of the path and shows up under its own symbol in rocprofv3 kernel traces.
// FUSED = true: the workgroup of a problem that finishes last (ticket counter over ALL gridDim.x
// workgroups of the problem's row, so that every one of them has read the state before it is
// rewritten) also runs the LM step -- no separate lm_kernel launch for this evaluation.  The step
// reads the same partials in the same order: results are bit-identical to the two-kernel form.
// ------------------------------------------------------------------------------------------
// The plain form (levels >= 1 of the launch-per-step schedule) is held to 96 VGPRs = five waves per SIMD, which is worth
// more there than the two or three registers the allocator would otherwise take (no spills); the level-0 and fused forms
// need 104-109 and run four.
// ROSEL: 0 = full and residual-only evaluations alike (chosen per problem at run time); 1 = this launch takes the full
// evaluations only, 2 = the residual-only ones only -- an instantiation of its own, without the 45 accumulators: 8 waves
// per SIMD instead of 4.
template <int MODE, bool LVL0, bool FUSED, int ROSEL = 0>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(ROSEL == 2 ? 7 : (LVL0 || FUSED || MODE == 1) ? 4 : 5))) void eval_kernel(const TrackerDev *const *__restrict__ trackers,
                                                        const LMState *__restrict__ states,
                                                        float *__restrict__ partials,
                                                        int partial_stride, int lvl, int *__restrict__ tickets,
                                                        int *__restrict__ status_out, int spec_nprob, const int *__restrict__ rowmap) {
  // spec_nprob > 0: grid rows [spec_nprob, 2 spec_nprob) evaluate the problems' speculative candidates (where staged)
  // rowmap != nullptr: a COMPACT launch -- grid row r works on problem rowmap[r] (the host lists the problems still at this
  // level after a read-back: a launch over all problems of a batch costs ~1.6 ns per workgroup just to start and end the
  // idle ones, 100 us for a level-0 grid of 512 problems; a level's last rounds are needed by a few stragglers only)
  const bool cand = spec_nprob > 0 && (int)blockIdx.y >= spec_nprob;
  const int row = cand ? blockIdx.y - spec_nprob : blockIdx.y;
  const int prob = rowmap ? ((const DSM_GLOBAL int *)rowmap)[row] : row;
  // Uniform, read-only state: global address space so that it becomes scalar (s_load) reads -- and ALL of them are issued
  // before the first one is looked at: the head of the state and the evaluation inputs of this row's candidate arrive in
  // ONE memory round trip instead of a chain of three (state -> candidate -> inputs), which was a seventh of a mid-level
  // workgroup's life.  (The asm statements pin the loads above the early exits; they emit no instruction.)
  const DSM_GLOBAL LMState &S = ((const DSM_GLOBAL LMState *)states)[prob];
  const DSM_GLOBAL EvalIn &in = cand ? S.spec_in : S.in;
  const int s_status = S.status, s_lvl = S.lvl, s_kind = S.is_scale, s_spec_valid = S.spec_valid;
  const TrackerDev *trk_ptr = FUSED ? ((const TrackerDev *const DSM_GLOBAL *)trackers)[prob] : nullptr; // (the fused step's descriptor: asked for with the state)
  // the MAIN candidate's point count: what the fused step reduces over (a speculative row's own inputs, S.spec_in, are stale where no
  // candidate was staged -- another level's count)
  const int main_n = FUSED ? S.in.n : 0, main_ppt = FUSED ? S.in.ppt : 0;
  EvalConsts c;
  DSM_EVAL_CONSTS_FROM_GLOBAL(c, in);
  asm volatile("" ::"s"(s_status), "s"(s_lvl), "s"(s_kind), "s"(s_spec_valid), "s"(c.pts), "s"(c.img), "s"(c.n), "s"(c.w), "s"(c.h),
               "s"(c.residual_only));
  if (FUSED) asm volatile("" ::"s"(trk_ptr), "s"(main_n), "s"(main_ppt));
  asm volatile("" ::"s"(c.fx), "s"(c.fy), "s"(c.cx), "s"(c.cy), "s"(c.huber), "s"(c.t[0]), "s"(c.t[1]), "s"(c.t[2]), "s"(c.aff0),
               "s"(c.aff1), "s"(c.b0), "s"(c.scale), "s"(c.cutoff), "s"(c.max_energy));
  asm volatile("" ::"s"(c.M[0]), "s"(c.M[1]), "s"(c.M[2]), "s"(c.M[3]), "s"(c.M[4]), "s"(c.M[5]), "s"(c.M[6]), "s"(c.M[7]), "s"(c.M[8]));
  if (LVL0) asm volatile("" ::"s"(c.Ki[0]), "s"(c.Ki[1]), "s"(c.Ki[2]), "s"(c.Ki[3]), "s"(c.Ki[4]), "s"(c.Ki[5]), "s"(c.Ki[6]), "s"(c.Ki[7]), "s"(c.Ki[8]));
  __shared__ int arrive; // tickets of the waves' row sums (eval_chunk_impl)
  if (!FUSED) {
    if (threadIdx.x == 0) arrive = 0;
    __syncthreads(); // (the waves of a workgroup start together and the loads above are in flight: costs nothing)
  }
  if (s_status != ST_RUNNING || s_lvl != lvl || s_kind != MODE) return;
  const bool have_eval = !cand || s_spec_valid != 0;
  if (!FUSED && !have_eval) return;
  if (ROSEL == 1 && c.residual_only) return;
  if (ROSEL == 2 && !c.residual_only) return;
  const int n = c.n;
  const int P = c.ppt;
  const int nchunks = (n + kThreads * P - 1) / (kThreads * P);
  // XCD-aware chunk mapping: workgroup b is dispatched to XCD b % 8, so give each XCD a
  // contiguous band of the template (and therefore of the target rows it gathers from).  Levels of fewer than 8 chunks get
  // exactly as many workgroups as chunks (a launch over hundreds of problems is bound by the workgroup dispatch rate there:
  // rounding 2 chunks up to 8 made the coarsest level's launches 2.5x longer).
  const int per_xcd = gridDim.x >> 3;
  const int chunk = (gridDim.x & 7) ? (int)blockIdx.x : (int)((blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3));
  float *partials_prob = partials + (size_t)prob * partial_stride;
  const int spec_off = partial_stride >> 1; // the speculative candidate's partials: second half of the problem's block
  if (chunk < nchunks && have_eval) {
    __shared__ float red[16][kNumSlots];
    int *const arr = FUSED ? nullptr : &arrive;
    float *const out = partials_prob + (cand ? spec_off : 0) + (size_t)chunk * kPartialStride;
    if (ROSEL == 2)
      eval_chunk_impl<MODE, LVL0, true>(c, chunk, threadIdx.x, true, red, out, arr);
    else
      eval_chunk<MODE, LVL0>(c, chunk, threadIdx.x, true, red, out, arr, MODE == 0 && LVL0 ? eval_fast(c) : 0);
    if (FUSED && threadIdx.x < 64) xwg_release(); // wave 0 stored the partial: performed at device scope before the ticket
  } else if (!FUSED) {
    return;
  }
  if (FUSED) {
    __shared__ int last;
    __syncthreads();
    if (threadIdx.x == 0) {
      const int t = atomicAdd(&tickets[prob], 1);
      last = t == (int)gridDim.x * (spec_nprob > 0 ? 2 : 1) - 1; // both candidates' rows arrive at the same counter
      if (last) tickets[prob] = 0; // for the next launch
    }
    __syncthreads();
    if (!last) return;
    xwg_acquire(); // the other workgroups' partials were announced by their tickets
    __shared__ LmShared sh;
    __shared__ LmSpecShared sps;
    // (the pending evaluation's point count came with this workgroup's own inputs, the tracker pointer with them: the step asks for
    // state, descriptor and partials in ONE round trip -- one frame in flight is a chain of these launches)
    LmPre pre;
    pre.n_lvl = main_n, pre.ppt_lvl = main_ppt, pre.have_sv = false;
    lm_step_block(MODE, lvl, prob, trk_ptr, const_cast<LMState &>(states[prob]), partials_prob, sh, threadIdx.x,
                  status_out, spec_nprob > 0 ? &sps : nullptr, spec_off, &pre);
  }
}

template <int MODE>
static void launch_eval_ml(hipStream_t s, int lvl, dim3 grid, const TrackerDev *const *trackers, const LMState *states,
                           float *partials, int partial_stride, int *tickets, int *status_out, int spec_nprob, bool split_ro, const int *rowmap) {
  auto launch = [&](auto lvl0, auto fused, auto rosel) {
    hipLaunchKernelGGL((eval_kernel<MODE, decltype(lvl0)::value != 0, decltype(fused)::value != 0, decltype(rosel)::value>), grid, dim3(kThreads), 0, s,
                       trackers, states, partials, partial_stride, lvl, tickets, status_out, spec_nprob, rowmap);
  };
  if (tickets) { // fused LM step (never level 0: its kernel stays a pure evaluation)
    launch(Const<0>{}, Const<1>{}, Const<0>{});
    return;
  }
  with_constant<2>(lvl == 0, [&](auto lvl0) {
    if (split_ro) { // the full evaluations, then the residual-only ones (ROSEL)
      launch(lvl0, Const<0>{}, Const<1>{});
      launch(lvl0, Const<0>{}, Const<2>{});
    } else {
      launch(lvl0, Const<0>{}, Const<0>{});
    }
  });
}

// tickets != nullptr (levels >= 1 only): the kernel also performs the LM step (no lm_kernel launch needed)
void launch_eval(hipStream_t s, int mode, int lvl, int grid_x, int nprob,
                 const TrackerDev *const *trackers, const LMState *states, float *partials,
                 int partial_stride, int *tickets, int *status_out, bool spec, bool split_ro, const int *rowmap) {
  dim3 grid(grid_x, spec ? 2 * nprob : nprob);
  const int spec_nprob = spec ? nprob : 0;
  if (lvl == 0) tickets = nullptr;
  with_constant<3>(mode, [&](auto m) {
    launch_eval_ml<decltype(m)::value>(s, lvl, grid, trackers, states, partials, partial_stride, tickets, status_out, spec_nprob, split_ro, rowmap);
  });
}

// one thread: the state machine of a new problem at its coarsest level (:451-474 / :854-872), first evaluation staged
__device__ __forceinline__ void lm_start_problem(const TrackerDev &T, LMState &S, int mode, const StartInfo &I) {
  S.is_scale = mode;
  S.coarsest = I.coarsest;
  S.have_repeated = 0;
  S.lambda = 0.01f;
  S.inc_norm = 0;
  S.inc_f = 0;
  for (int i = 0; i < 7; i++) S.cur[i] = I.pose[i];
  S.aff_cur[0] = I.aff[0];
  S.aff_cur[1] = I.aff[1];
  S.scale_cur = I.scale;
  for (int i = 0; i < DSM_MAX_LEVELS; i++) {
    S.last_residuals[i] = __builtin_nan(""); // :459 / :860
    S.last_inners[i] = 0;
    S.min_res[i] = I.min_res[i];
    S.evals[i] = 0;
    S.evals_ro[i] = 0;
    S.rounds[i] = 0;
  }
  S.spec_valid = 0;
  S.ticks = 0;
  S.n0 = T.lv[0].n;
  S.flow[0] = S.flow[1] = S.flow[2] = 1000; // :460
  S.status = ST_RUNNING;
  begin_level(T, S, I.coarsest);
}

__global__ __launch_bounds__(kLmThreads) void lm_kernel(int mode, int op, int lvl,
                                                        const TrackerDev *const *__restrict__ trackers,
                                                        LMState *__restrict__ states,
                                                        const float *__restrict__ partials, int partial_stride,
                                                        const StartInfo *__restrict__ start,
                                                        SingleOut *__restrict__ single_out,
                                                        int *__restrict__ status_out, int spec, const int *__restrict__ rowmap) {
  const int prob = rowmap ? rowmap[blockIdx.x] : blockIdx.x; // (compact launch: see eval_kernel)
  const bool pose_like = mode != 1; // 0: frame tracking, 2: loop-closure pose -- same 8-DoF LM; 1: stereo scale
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const TrackerDev &T = *trackers[prob];
  LMState &S = states[prob];
  __shared__ LmShared sh;
  __shared__ LmSpecShared sps;

  if (op == LM_OP_START) {
    if (tid == 0) {
      lm_start_problem(T, S, mode, start[prob]);
      if (status_out) {
        status_out[2 * prob] = S.status;
        status_out[2 * prob + 1] = S.lvl;
      }
    }
    return;
  }
  if (op == LM_OP_SINGLE_PREP) {
    if (tid == 0) {
      const StartInfo &I = start[prob];
      S.is_scale = mode;
      S.status = ST_RUNNING;
      S.lvl = I.lvl;
      S.spec_valid = 0;
      make_eval_any(T, S, mode, I.lvl, I.pose, I.aff, I.scale, I.cutoff, I.residual_only != 0);
    }
    return;
  }

  // ---- LM_OP_STEP / LM_OP_SINGLE_FINISH ----
  // (one round trip: status, level, kind, the pending evaluation's point count, the tracker pointer and this thread's block of the state)
  const LmHead hd = lm_read_head(S, trackers, prob, tid);
  const bool active = (hd.status == ST_RUNNING && hd.lvl == lvl && hd.kind == mode);
  if (!active) { // block-uniform
    if (tid == 0 && status_out) {
      status_out[2 * prob] = hd.status;
      status_out[2 * prob + 1] = hd.lvl;
    }
    return;
  }
  if (op == LM_OP_STEP) {
    lm_step_block(mode, lvl, prob, hd.Tg, S, partials + (size_t)prob * partial_stride, sh, tid, status_out, spec ? &sps : nullptr, partial_stride >> 1, &hd.pre);
    return;
  }

  // LM_OP_SINGLE_FINISH: reduced sums -> rs, H, b of one evaluation (dsm_tracker_calc_res_*)
  reduce_partials_groups(partials + (size_t)prob * partial_stride, chunks_of(S.in.n, S.in.ppt), tid, sh.red);
  __syncthreads();
  if (tid >= 64) return;
  reduce_partials_final(lane, sh.red);
  const double *sums = sh.red.sums;
  const long long *isums = sh.red.isums;
  double rs[6];
  build_rs(sums, isums, S.in.max_energy, rs);
  const int n_warped = (int)isums[2];
  const int n4 = (n_warped + 3) & ~3;
  const int r = lane >> 3, c = lane & 7;
  SingleOut &O = single_out[prob];
  if (pose_like) {
    O.H[lane] = build_H_elem(T.p, sums, n4, r, c);
    if (lane < 8) O.b[lane] = build_b_elem(T.p, sums, n4, lane);
  }
  if (lane == 0) {
    for (int i = 0; i < 6; i++) O.rs[i] = rs[i];
    O.n_warped = n4;
    if (pose_like) {
      O.Hs = O.bs = 0;
    } else {
      O.Hs = (float)sums[0] * (1.0f / n4); // :1003-1004
      O.bs = (float)sums[1] * (1.0f / n4);
    }
    S.status = ST_IDLE;
  }
}
void launch_lm(hipStream_t s, int mode, int op, int lvl, int nprob, const TrackerDev *const *trackers,
               LMState *states, const float *partials, int partial_stride, const StartInfo *start,
               SingleOut *single_out, int *status_out, bool spec, const int *rowmap) {
  hipLaunchKernelGGL(lm_kernel, dim3(nprob), dim3(kLmThreads), 0, s, mode, op, lvl, trackers, states, partials,
                     partial_stride, start, single_out, status_out, spec ? 1 : 0, rowmap);
}

} // namespace dsm
