// form_diag.hpp -- the two diagnostic kernels of the tracker kernels (a part of tracker_kernels.hip, see the map at the top of that
// file): one evaluation in the form the chains run it, and the proposing half of an LM step on caller-supplied systems.
#pragma once

namespace dsm {

// dsm_diag_single_eval / dsm_diag_pose_estimator_eval, form 3: ONE evaluation in the form the chains run it (chain_kernel of form_chain.hpp, tick_eval_kernel's chain path) -- the
// inputs from the LDS copy of the state, the level's single chunk into an LDS partial with the workgroup barrier between the row sums
// and the final sum -- and the partial copied out to where LM_OP_SINGLE_FINISH reads it.  The same eval_chunk instantiations under the
// same register budget as the chains'; no state machine.  A level of no chunk writes nothing (as the chains evaluate nothing there).
template <int MODE>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(4))) void diag_chain_eval_kernel(const LMState *__restrict__ states,
                                                                                                        float *__restrict__ partials) {
  __shared__ float red[16][kNumSlots];
  __shared__ __attribute__((aligned(16))) LMState st;
  __shared__ __attribute__((aligned(16))) float part[kPartialStride];
  const int tid = threadIdx.x;
  stage_in(st, states, tid, kThreads);
  if (tid < kPartialStride) part[tid] = 0.f; // (the scale problem writes 7 of the 52 slots)
  __syncthreads();
  const int status = __builtin_amdgcn_readfirstlane(st.status), lvl = __builtin_amdgcn_readfirstlane(st.lvl);
  EvalConsts c;
  eval_consts_from_lds(st.in, c);
  if (status != ST_RUNNING || st.is_scale != MODE || chunks_of(c.n, c.ppt) != 1) return; // workgroup-uniform
  DSM_EVAL_CHUNK_DEEP(MODE, c, lvl, 0, tid, red, part);
  __syncthreads();
  if (tid < kNumSlots) partials[tid] = part[tid];
}
void launch_diag_chain_eval(hipStream_t s, int mode, const LMState *states, float *partials) {
  with_constant<3>(mode, [&](auto m) {
    hipLaunchKernelGGL((diag_chain_eval_kernel<decltype(m)::value>), dim3(1), dim3(kThreads), 0, s, states, partials);
  });
}

// dsm_diag_lm_propose: the proposing half of an LM step on caller-supplied systems, one workgroup per problem.  A zeroed LMState in
// LDS takes the level part of both candidates' blocks (as begin_level leaves them) and the caller's fields; wave 0 then runs the
// production propose_pose / propose_scale unchanged -- with wave 2 as its helper where asked for, as in lm_step_block -- after one
// extra call of the solve that exposes the raw increment.  No state machine, no partials.
__global__ __launch_bounds__(kLmThreads) void diag_lm_propose_kernel(int mode, int lvl, const TrackerDev *__restrict__ Tg, int n,
                                                                     const ::dsm_lm_propose_in *__restrict__ in,
                                                                     ::dsm_lm_propose_out *__restrict__ out, int spec, int helper) {
  __shared__ LmShared sh;
  const int prob = blockIdx.x, tid = threadIdx.x;
  if (prob >= n) return; // workgroup-uniform
  if (tid < kLmT16) ((uint4 *)&sh.trk)[tid] = ((const uint4 *)Tg)[tid];
  for (int i = tid; i < kLmS16; i += kLmThreads) ((uint4 *)&sh.st)[i] = uint4{0, 0, 0, 0};
  if (tid == 0) sh.help.cmd = 0, sh.help.done = 0;
  __syncthreads();
  const TrackerDev &T = sh.trk;
  LMState &S = sh.st;
  const ::dsm_lm_propose_in &I = in[prob];
  const float lambda = I.lambda;
  if (tid < 64) S.H[tid] = I.H[tid];
  if (tid < 8) S.b[tid] = I.b[tid];
  if (tid == 0) {
    S.status = ST_RUNNING;
    S.lvl = lvl;
    S.phase = PH_INIT;
    S.is_scale = mode;
    S.iteration = I.iteration;
    S.lambda = lambda;
    S.level_cutoff_repeat = I.level_cutoff_repeat;
    for (int i = 0; i < 7; i++) S.cur[i] = I.cur[i];
    S.aff_cur[0] = I.aff_cur[0], S.aff_cur[1] = I.aff_cur[1];
    S.Hs = I.Hs, S.bs = I.bs, S.scale_cur = I.scale_cur;
    make_eval_level(T, S.in, mode, lvl);
    make_eval_level(T, S.spec_in, mode, lvl);
  }
  __syncthreads();
  const bool helped = mode != 1 && helper != 0;
  if (helped && tid >= 128 && tid < 192) lm_help_wave(T, S, sh.help, tid - 128);
  if (tid >= 64) return; // wave 0 carries on
  const int lane = tid;
  double inc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (mode != 1) {
    unsigned active;
    bool stitch;
    lm_solve_unknowns(T, active, stitch);
    wave_ldlt_solve8(S.H, S.b, lambda, active, stitch, lane, sh.ldlt, inc);
    propose_pose(T, S, lambda, lane, sh.ldlt, spec != 0, helped ? &sh.help : nullptr);
  } else if (lane == 0) {
    propose_scale(T, S, lambda, spec != 0);
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  if (lane != 0) return;
  const EvalIn &e = spec ? S.spec_in : S.in;
  ::dsm_lm_propose_out &O = out[prob];
  for (int i = 0; i < 8; i++) O.inc[i] = inc[i];
  O.inc_norm = spec ? S.spec_inc_norm : S.inc_norm;
  for (int i = 0; i < 7; i++) O.cand[i] = spec ? S.spec_cand[i] : S.cand[i];
  for (int i = 0; i < 2; i++) O.aff_cand[i] = spec ? S.spec_aff_cand[i] : S.aff_cand[i];
  for (int i = 0; i < 9; i++) O.M[i] = e.M[i], O.Ki[i] = e.Ki[i];
  for (int i = 0; i < 3; i++) O.t[i] = e.t[i];
  O.aff0 = e.aff0, O.aff1 = e.aff1, O.cutoff = e.cutoff, O.max_energy = e.max_energy;
  O.residual_only = e.residual_only;
  O.inc_f = spec ? S.spec_inc_f : S.inc_f;
  O.scale_cand = spec ? S.spec_scale_cand : S.scale_cand;
  O.pad[0] = O.pad[1] = 0;
}
void launch_diag_lm_propose(hipStream_t s, int mode, int lvl, const TrackerDev *tracker, int n, const ::dsm_lm_propose_in *in,
                            ::dsm_lm_propose_out *out, bool spec, bool helper) {
  hipLaunchKernelGGL(diag_lm_propose_kernel, dim3(n), dim3(kLmThreads), 0, s, mode, lvl, tracker, n, in, out, spec ? 1 : 0, helper ? 1 : 0);
}

} // namespace dsm
