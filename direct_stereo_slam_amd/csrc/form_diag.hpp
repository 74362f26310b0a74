// form_diag.hpp -- the diagnostic kernels of the tracker kernels (a part of tracker_kernels.hip, see the map at the top of that
// file): one evaluation in the form the chains run it, the proposing half of an LM step on caller-supplied systems, one whole LM
// step on caller-supplied states and partials, and the tick engine's reservation and staging (tick_after_step) on caller-supplied
// slot states, with the kernels that build and unpack the slots of dsm_diag_tick_step.
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

// dsm_diag_lm_step: ONE production LM step -- lm_step_block unchanged: the fixed-order reduction of the caller's partials, build_rs /
// build_H_elem / build_b_elem, lm_step_wave0 with end_level, begin_level and finish_track, the speculative block and the helper waves
// where asked for -- on a caller-supplied state, one workgroup per problem.  The problem is built in device memory, where the
// production kernels keep it: a zeroed LMState takes the level part of both candidates' blocks (as begin_level leaves them) and the
// caller's fields; the pending evaluation's n / ppt are set so that chunks_of gives the caller's chunk count.  After the step the
// state is read back from device memory (what lm_step_block stored, not its LDS copy).
__device__ __forceinline__ void diag_eval_in(EvalIn &e, const ::dsm_lm_step_eval &v, int mode, int nch) {
  if (mode == 1) { // (M, t and the affine pair are the level's: make_eval_level)
    e.scale = v.scale;
  } else {
    for (int i = 0; i < 9; i++) e.M[i] = v.M[i];
    for (int i = 0; i < 3; i++) e.t[i] = v.t[i];
    e.aff0 = v.aff0, e.aff1 = v.aff1;
  }
  e.cutoff = v.cutoff, e.max_energy = v.max_energy;
  e.residual_only = v.residual_only;
  e.n = nch * kThreads, e.ppt = 1; // chunks_of(n, ppt) == nch
}
__device__ __forceinline__ void diag_eval_out(::dsm_lm_step_eval &v, const EvalIn &e) {
  for (int i = 0; i < 9; i++) v.M[i] = e.M[i], v.Ki[i] = e.Ki[i];
  for (int i = 0; i < 3; i++) v.t[i] = e.t[i];
  v.aff0 = e.aff0, v.aff1 = e.aff1, v.cutoff = e.cutoff, v.max_energy = e.max_energy;
  v.residual_only = e.residual_only;
  v.scale = e.scale;
  v.n = e.n;
}
// all threads of the workgroup: the problem dsm_diag_lm_step describes, built in S (device memory); ends with a workgroup barrier
__device__ __forceinline__ void diag_fill_state(LMState &S, const ::dsm_lm_step_state &I, const TrackerDev *Tg, int mode, int lvl, int tid) {
  for (int i = tid; i < kLmS16; i += kLmThreads) ((uint4 *)&S)[i] = uint4{0, 0, 0, 0};
  __syncthreads();
  if (tid < 64) S.H[tid] = I.H[tid];
  if (tid < 8) S.b[tid] = I.b[tid];
  if (tid == 0) {
    S.status = ST_RUNNING;
    S.lvl = lvl;
    S.phase = I.phase;
    S.is_scale = mode;
    S.iteration = I.iteration;
    S.have_repeated = I.have_repeated;
    S.coarsest = I.coarsest;
    S.lambda = I.lambda;
    S.level_cutoff_repeat = I.level_cutoff_repeat;
    S.inc_f = I.inc_f, S.scale_cur = I.scale_cur, S.scale_cand = I.scale_cand, S.Hs = I.Hs, S.bs = I.bs;
    S.inc_norm = I.inc_norm;
    for (int i = 0; i < 7; i++) S.cur[i] = I.cur[i], S.cand[i] = I.cand[i], S.spec_cand[i] = I.spec_cand[i];
    for (int i = 0; i < 2; i++) S.aff_cur[i] = I.aff_cur[i], S.aff_cand[i] = I.aff_cand[i], S.spec_aff_cand[i] = I.spec_aff_cand[i];
    for (int i = 0; i < 6; i++) S.res_old[i] = I.res_old[i];
    for (int i = 0; i < DSM_MAX_LEVELS; i++) {
      S.min_res[i] = I.min_res[i], S.last_residuals[i] = I.last_residuals[i], S.last_inners[i] = I.last_inners[i];
      S.evals[i] = I.evals[i], S.evals_ro[i] = I.evals_ro[i], S.rounds[i] = I.rounds[i];
    }
    for (int i = 0; i < 3; i++) S.flow[i] = I.flow[i];
    S.spec_valid = I.spec_valid;
    S.ticks = I.ticks;
    S.spec_scale_cand = I.spec_scale_cand, S.spec_inc_f = I.spec_inc_f;
    S.spec_inc_norm = I.spec_inc_norm;
    make_eval_level(*Tg, S.in, mode, lvl);
    make_eval_level(*Tg, S.spec_in, mode, lvl);
    diag_eval_in(S.in, I.ev, mode, I.nch);
    diag_eval_in(S.spec_in, I.spec_ev, mode, I.nch);
  }
  __threadfence(); // the state is read back below by other threads, in the coherent form with device-scope loads
  __syncthreads();
}
// one thread: the state R as dsm_diag_lm_step hands it back
__device__ __forceinline__ void diag_state_out(::dsm_lm_step_state &O, const LMState &R, int nch) {
  for (int i = 0; i < 64; i++) O.H[i] = R.H[i];
  for (int i = 0; i < 8; i++) O.b[i] = R.b[i];
  for (int i = 0; i < 7; i++) O.cur[i] = R.cur[i], O.cand[i] = R.cand[i], O.spec_cand[i] = R.spec_cand[i];
  for (int i = 0; i < 2; i++) O.aff_cur[i] = R.aff_cur[i], O.aff_cand[i] = R.aff_cand[i], O.spec_aff_cand[i] = R.spec_aff_cand[i];
  O.inc_norm = R.inc_norm, O.spec_inc_norm = R.spec_inc_norm;
  for (int i = 0; i < 6; i++) O.res_old[i] = R.res_old[i];
  for (int i = 0; i < DSM_MAX_LEVELS; i++) {
    O.min_res[i] = R.min_res[i], O.last_residuals[i] = R.last_residuals[i], O.last_inners[i] = R.last_inners[i];
    O.evals[i] = R.evals[i], O.evals_ro[i] = R.evals_ro[i], O.rounds[i] = R.rounds[i];
  }
  for (int i = 0; i < 3; i++) O.flow[i] = R.flow[i];
  O.status = R.status, O.lvl = R.lvl, O.phase = R.phase, O.iteration = R.iteration, O.have_repeated = R.have_repeated;
  O.coarsest = R.coarsest, O.spec_valid = R.spec_valid, O.ticks = R.ticks;
  O.lambda = R.lambda, O.level_cutoff_repeat = R.level_cutoff_repeat;
  O.inc_f = R.inc_f, O.spec_inc_f = R.spec_inc_f, O.scale_cur = R.scale_cur, O.scale_cand = R.scale_cand;
  O.spec_scale_cand = R.spec_scale_cand, O.Hs = R.Hs, O.bs = R.bs;
  O.nch = nch;
  diag_eval_out(O.ev, R.in);
  diag_eval_out(O.spec_ev, R.spec_in);
}
template <bool COH>
__global__ __launch_bounds__(kLmThreads) void diag_lm_step_kernel(int mode, int lvl, const TrackerDev *__restrict__ Tg, int n,
                                                                  const ::dsm_lm_step_state *__restrict__ in, ::dsm_lm_step_state *__restrict__ out,
                                                                  LMState *states, const float *partials, long long partial_stride, int spec,
                                                                  int spec_off, int helper) {
  __shared__ LmShared sh;
  __shared__ LmSpecShared sps;
  const int prob = blockIdx.x, tid = threadIdx.x;
  if (prob >= n) return; // workgroup-uniform
  LMState &S = states[prob];
  diag_fill_state(S, in[prob], Tg, mode, lvl, tid);
  lm_step_block<COH>(mode, lvl, prob, Tg, S, partials + (size_t)prob * (size_t)partial_stride, sh, tid, nullptr, spec ? &sps : nullptr, spec_off,
                     nullptr, (LmNoEarly *)nullptr, helper != 0);
  __threadfence(); // wave 0's stores of the state
  __syncthreads();
  if (tid != 0) return;
  uint4 *back = (uint4 *)&sh.st; // (the step is over: its LDS copy is free) the stored state, through the path that stored it
  for (int i = 0; i < kLmS16; i++) back[i] = COH ? load16_coherent((const uint4 *)&S + i) : ((const uint4 *)&S)[i];
  diag_state_out(out[prob], sh.st, in[prob].nch);
}
void launch_diag_lm_step(hipStream_t s, int mode, int lvl, const TrackerDev *tracker, int n, const ::dsm_lm_step_state *in,
                         ::dsm_lm_step_state *out, LMState *states, const float *partials, long long partial_stride, bool spec, int spec_off,
                         bool helper, bool coherent) {
  if (coherent)
    hipLaunchKernelGGL(diag_lm_step_kernel<true>, dim3(n), dim3(kLmThreads), 0, s, mode, lvl, tracker, n, in, out, states, partials,
                       partial_stride, spec ? 1 : 0, spec_off, helper ? 1 : 0);
  else
    hipLaunchKernelGGL(diag_lm_step_kernel<false>, dim3(n), dim3(kLmThreads), 0, s, mode, lvl, tracker, n, in, out, states, partials,
                       partial_stride, spec ? 1 : 0, spec_off, helper ? 1 : 0);
}

// dsm_diag_tick_stage: one wave per slot, every slot of the call in one launch (the list's and the ring's atomics contend).  The slot's
// state -- built by the host, as it stands after a step -- is staged into LDS as tick_lm_kernel holds it; the wave makes the slot's
// reservation through TickReserve itself (or takes the caller's base and total) and calls tick_after_step as tick_lm_kernel does.
__global__ __launch_bounds__(64) void diag_tick_stage_kernel(int mode, int n, const ::dsm_tick_slot *__restrict__ slots, const TrackerDev **trackers,
                                                             LMState *states, TickList L, TickModeCtl *mc, const TickPending *pending,
                                                             TickResult *results, unsigned long long *slot_ticket, int stepped) {
  __shared__ __attribute__((aligned(16))) LMState st;
  __shared__ __attribute__((aligned(16))) TrackerDev trk;
  const int prob = blockIdx.x, lane = threadIdx.x;
  if (prob >= n) return; // workgroup-uniform
  stage_in(st, &states[prob], lane, 64);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  const int req = slots[prob].reserve;
  TickReserve rsv{L, 0, 0};
  if (req == 1 || req == 2)
    rsv(st, lane, req == 2);
  else if (req == 3)
    rsv.base = slots[prob].res_base, rsv.total = slots[prob].res_total;
  const int res_base = __builtin_amdgcn_readfirstlane(rsv.base);
  tick_after_step(mode, prob, trackers, states, st, trk, L, mc, pending, results, slot_ticket, lane, stepped, res_base, rsv.total);
}
void launch_diag_tick_stage(hipStream_t s, int mode, int n, const ::dsm_tick_slot *slots, const TrackerDev **trackers, LMState *states,
                            const TickList &list, TickModeCtl *mc, const TickPending *pending, TickResult *results,
                            unsigned long long *slot_ticket, int stepped) {
  hipLaunchKernelGGL(diag_tick_stage_kernel, dim3(n), dim3(64), 0, s, mode, n, slots, trackers, states, list, mc, pending, results, slot_ticket,
                     stepped);
}

// dsm_diag_tick_step: the slots' states, built as dsm_diag_lm_step builds its problems; a free slot is the same state, idle
__global__ __launch_bounds__(kLmThreads) void diag_tick_fill_kernel(int mode, int lvl, const TrackerDev *__restrict__ Tg, int n,
                                                                    const ::dsm_lm_step_state *__restrict__ in,
                                                                    const ::dsm_tick_slot *__restrict__ slots, LMState *states) {
  const int prob = blockIdx.x, tid = threadIdx.x;
  if (prob >= n) return; // workgroup-uniform
  LMState &S = states[prob];
  diag_fill_state(S, in[prob], Tg, mode, lvl, tid);
  if (tid == 0) {
    S.stepped = slots[prob].stepped;
    if (slots[prob].status == ST_IDLE) S.status = ST_IDLE;
  }
}
void launch_diag_tick_fill(hipStream_t s, int mode, int lvl, const TrackerDev *tracker, int n, const ::dsm_lm_step_state *in,
                           const ::dsm_tick_slot *slots, LMState *states) {
  hipLaunchKernelGGL(diag_tick_fill_kernel, dim3(n), dim3(kLmThreads), 0, s, mode, lvl, tracker, n, in, slots, states);
}

// both tick diagnostics: every slot's state as a dsm_lm_step_state and what else an admission may have written, one thread per slot
__global__ __launch_bounds__(64) void diag_tick_unpack_kernel(int n, const LMState *__restrict__ states, const TrackerDev *const *__restrict__ trackers,
                                                              const TrackerDev *tracker, const unsigned long long *__restrict__ slot_ticket,
                                                              ::dsm_lm_step_state *__restrict__ state_out, ::dsm_tick_slot_out *__restrict__ slot_out) {
  const int prob = blockIdx.x * 64 + threadIdx.x;
  if (prob >= n) return;
  const LMState &S = states[prob];
  diag_state_out(state_out[prob], S, S.in.ppt > 0 ? chunks_of(S.in.n, S.in.ppt) : 0);
  ::dsm_tick_slot_out &O = slot_out[prob];
  O.status = S.status, O.lvl = S.lvl, O.stepped = S.stepped, O.n = S.in.n, O.ppt = S.in.ppt, O.spec_valid = S.spec_valid, O.n0 = S.n0;
  O.residual_only = S.in.residual_only;
  O.tracker_set = trackers[prob] == tracker ? 1 : 0, O.pad = 0;
  O.ticket = slot_ticket[prob];
}
void launch_diag_tick_unpack(hipStream_t s, int n, const LMState *states, const TrackerDev *const *trackers, const TrackerDev *tracker,
                             const unsigned long long *slot_ticket, ::dsm_lm_step_state *state_out, ::dsm_tick_slot_out *slot_out) {
  hipLaunchKernelGGL(diag_tick_unpack_kernel, dim3((n + 63) / 64), dim3(64), 0, s, n, states, trackers, tracker, slot_ticket, state_out, slot_out);
}

// dsm_diag_eval_facts: the facts of a pose evaluation of level lvl at `pose`, derived as the production path derives them -- the
// level part by make_eval_level, M and t by make_eval_rot, the pose fact by eval_chunk's own rule (one thread).
// out = {template fact, image fact of the new left frame, pose fact, eval_fast's answer: 1 fast / 0 general}, then the bits of the
// list's bounds {xmin, xmax, ymin, ymax, idmax} as the evaluation's inputs carry them
__global__ void diag_eval_facts_kernel(const TrackerDev *T, int lvl, const double *pose, int *out) {
  EvalIn e;
  make_eval_level(*T, e, 0, lvl);
  store_eval_facts(e, load_eval_facts(*T, 0, lvl));
  make_eval_rot(e, 0, pose, true);
  const TrackerFacts *F = T->facts;
  out[0] = F && F->lv[lvl].tpl_plain == 1 ? 1 : 0;
  out[1] = F && F->img_plain[T->img_set[0] & (kFactImageSets - 1)][lvl] == 1 ? 1 : 0;
  out[2] = pose_fact(e.M[6], e.M[7], e.M[8], e.t[2], e.bx0, e.bx1, e.by0, e.by1, e.bid) ? 1 : 0;
  out[3] = e.plain != 0 && out[2] ? 1 : 0;
  out[4] = __float_as_int(e.bx0), out[5] = __float_as_int(e.bx1), out[6] = __float_as_int(e.by0), out[7] = __float_as_int(e.by1);
  out[8] = __float_as_int(e.bid);
}
void launch_diag_eval_facts(hipStream_t s, const TrackerDev *tracker, int lvl, const double *d_pose, int *d_out) {
  hipLaunchKernelGGL(diag_eval_facts_kernel, dim3(1), dim3(1), 0, s, tracker, lvl, d_pose, d_out);
}

} // namespace dsm
