// form_chain.hpp -- the chain form of the tracker kernels (a part of tracker_kernels.hip, see the map at the top of that file): one
// workgroup carries a problem through every round whose evaluation is a single chunk.  tick_chain_round is the round both users share:
// chain_kernel here and the chain branch of tick_eval_kernel (form_tick.hpp, included after this file).
#pragma once

namespace dsm {

// One LM round of a chain (below): the single chunk's partial (LDS) reduced in the fixed order of every other form, wave 0 steps the
// state machine on the LDS copy of the state.  Not inlined: the evaluation loops of tick_eval_kernel keep their registers.
// (LDS objects are handed over as local-address-space pointers: the inlined state machine keeps its ds_ instructions.)
template <int MODE>
__device__ __attribute__((noinline)) void tick_chain_round(DSM_LDS LmShared *shp, const DSM_LDS float *partp, int nch, int lvl, int tid, bool help) {
  LmShared &sh = *(LmShared *)shp;
  const float *part = (const float *)partp;
  reduce_partials_groups(part, nch, tid, sh.red);
  if (tid == 0) sh.help.cmd = 0, sh.help.done = 0;
  __syncthreads();
  if (tid < 64) {
    reduce_partials_final(tid, sh.red);
    lm_step_wave0(MODE, lvl, sh.trk, sh.st, sh, tid, nullptr, MODE != 1 && help);
  } else if (MODE != 1 && help && tid >= 128 && tid < 192) {
    lm_help_wave(sh.trk, sh.st, sh.help, tid - 128);
  }
  __syncthreads(); // the state (status, level, next evaluation inputs) is read by all waves
}

// chain_kernel: the chain of the tick engine as a launch of its own (dsm_params.persistent_coarse < 0: single calls -- one frame in
// flight).  One workgroup per problem carries it through every level whose evaluation is ONE chunk -- evaluate, reduce, step, on the
// LDS copy of the state -- and hands it back (still RUNNING) at the first level of several chunks: the coarse levels' rounds, each
// a launch of 12-14 us in the launch-per-step form, cost an evaluation and a step.  Same chunk, same partial, same reduction order.
template <int MODE>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(4))) void chain_kernel(const TrackerDev *const *__restrict__ trackers,
                                                                                              LMState *__restrict__ states, int *__restrict__ status_out) {
  __shared__ float red[16][kNumSlots];
  __shared__ LmShared sh;
  __shared__ __attribute__((aligned(16))) float part[kPartialStride];
  const int prob = blockIdx.x, tid = threadIdx.x;
  LMState &S = states[prob];
  if (!(S.status == ST_RUNNING && S.is_scale == MODE)) return; // workgroup-uniform
  stage_in(sh.st, &S, tid, kThreads);
  stage_in(sh.trk, trackers[prob], tid, kThreads);
  __syncthreads();
  int rounds = 0;
  for (;;) {
    const int status = __builtin_amdgcn_readfirstlane(sh.st.status), lvl = __builtin_amdgcn_readfirstlane(sh.st.lvl);
    const int spec_valid = __builtin_amdgcn_readfirstlane(sh.st.spec_valid);
    EvalConsts c;
    eval_consts_from_lds(sh.st.in, c);
    const int nch = chunks_of(c.n, c.ppt);
    if (status != ST_RUNNING || nch > 1 || spec_valid) break; // workgroup-uniform
    if (nch == 1) {
      DSM_EVAL_CHUNK_DEEP(MODE, c, lvl, 0, tid, red, part);
    }
    __syncthreads();
    tick_chain_round<MODE>((DSM_LDS LmShared *)&sh, (const DSM_LDS float *)part, nch, lvl, tid, true);
    rounds++;
  }
  if (rounds > 0 && tid < 64) stage_out(&S, sh.st, tid, 64);
  if (tid == 0 && status_out) {
    status_out[2 * prob] = sh.st.status;
    status_out[2 * prob + 1] = sh.st.lvl;
  }
}
void launch_chain(hipStream_t s, int mode, int nprob, const TrackerDev *const *trackers, LMState *states, int *status_out) {
  with_constant<3>(mode, [&](auto m) {
    hipLaunchKernelGGL((chain_kernel<decltype(m)::value>), dim3(nprob), dim3(kThreads), 0, s, trackers, states, status_out);
  });
}

} // namespace dsm
