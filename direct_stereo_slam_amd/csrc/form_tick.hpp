// form_tick.hpp -- the tick engine of the tracker kernels (a part of tracker_kernels.hip, see the map at the top of that file;
// included after form_chain.hpp, whose tick_chain_round the chains of tick_eval_kernel run): reservation and admission of waiting
// problems, the item lists, tick_eval_kernel and tick_lm_kernel, each kernel with its launcher.
#pragma once

namespace dsm {

// ------------------------------------------------------------------------------------------
// Tick engine of the streaming form (dsm_stream_*, stream_capi.hip).  A tick advances EVERY resident problem by one LM round,
// whatever level it stands on: tick_eval_kernel evaluates a device-built list of (problem, chunk) items -- all levels mixed in
// one grid, the small levels' chunks filling what the large ones leave --, tick_lm_kernel (one workgroup per slot) steps the
// problems, stages the next tick's items, retires finished problems into a result array and refills their slots from the
// waiting list.  Kernel boundaries order everything: no cross-workgroup protocol, no tickets, no host round trip inside an
// advance.  Same chunks, same partials, same reduction order as every other form: bit-identical results.
// ------------------------------------------------------------------------------------------
// wave 0: the items of the evaluation(s) staged in `St` (the main candidate and, where staged, the speculative one) -- or, where chains
// are on and the evaluation is ONE chunk with no speculative twin, a chain entry: the problem's number behind the list's item slots
// res_base / res_total: item slots this problem reserved EARLY in its step (TickReserve below), to be used or filled with no-ops.
__device__ __forceinline__ void tick_push(const LMState &St, int prob, const TickList &L, TickModeCtl *mc, int lane, int res_base = 0, int res_total = 0) {
  const int nch = chunks_of(St.in.n, St.in.ppt), per_xcd = (nch + 7) >> 3;
  const bool chain = L.chain_cap > 0 && nch == 1 && !St.spec_valid && (L.chain_max_n0 <= 0 || St.n0 <= L.chain_max_n0);
  const int npos = nch < 8 ? nch : 8 * per_xcd;
  int total = chain ? 0 : St.spec_valid ? 2 * npos : npos;
  if (chain && lane == 0) {
    const int idx = atomicAdd(&L.seg->chain[L.buf], 1);
    if (idx < L.chain_cap)
      L.items[L.cap + idx] = (unsigned)prob;
    else
      L.seg->overflow = 1;
    // (the chain books its evaluations itself, round by round)
  }
  int base = res_base;
  if (total > res_total) { // nothing reserved (a reservation is never too short: it is made for the same level, with the twin counted)
    for (int i = lane; i < res_total; i += 64)
      if (res_base + i < L.cap) L.items[res_base + i] = kTickNoop; // (a reservation that ran over the list lies partly behind it: the chain entries are there)
    res_total = 0;
    if (lane == 0) {
      base = atomicAdd(&L.seg->count[L.buf], total);
      if (base + total > L.cap) L.seg->overflow = 1;
    }
    base = __builtin_amdgcn_readfirstlane(base);
  }
  if (total > 0 && lane == 0) {
    const int lvl = St.lvl;
    atomicAdd((unsigned long long *)&mc->sched_evals[lvl], 1ull);
    if (St.in.residual_only) atomicAdd((unsigned long long *)&mc->sched_ro[lvl], 1ull);
    atomicAdd((unsigned long long *)&mc->sched_items[lvl], (unsigned long long)total);
  }
  const int fill = total > res_total ? total : res_total; // (total == 0: an empty level -- nothing to evaluate, the LM step runs anyway)
  for (int i = lane; i < fill; i += 64) {
    const bool cand = i >= npos;
    const int p = cand ? i - npos : i;
    // position p runs on XCD (base + p) % 8 (workgroup index = list position + a constant): XCD-contiguous bands of the template, as eval_kernel
    const int chunk = nch < 8 ? p : (p & 7) * per_xcd + (p >> 3);
    const unsigned item = (i < total && chunk < nch) ? (((unsigned)prob << kTickChunkBits) | (unsigned)chunk | (cand ? kTickCand : 0u)) : kTickNoop;
    if (base + i < L.cap) L.items[base + i] = item;
  }
}
// The reservation: handed to the LM step as its `early` hook by tick_lm_kernel.  The step proposes, so the next evaluation is one of the
// level the state stands on: its items (and the speculative twin's, should one be staged) get their place in the list NOW, and the
// atomic's round trip -- 2 k of the 4.9 k cycles "items of the next tick" cost at the end of a step (profiles/r06_tick_stamps.json) --
// runs under the solve.
struct TickReserve {
  TickList L;
  int base, total;
  __device__ __forceinline__ void operator()(const LMState &St, int lane, bool want_spec) {
    const int nch = chunks_of(St.in.n, St.in.ppt), per_xcd = (nch + 7) >> 3;
    const int npos = nch < 8 ? nch : 8 * per_xcd;
    if (L.chain_cap > 0 && nch == 1 && !want_spec && (L.chain_max_n0 <= 0 || St.n0 <= L.chain_max_n0)) return; // (goes to the chain list)
    total = want_spec ? 2 * npos : npos;
    if (total == 0) return;
    int b = 0;
    if (lane == 0) {
      b = atomicAdd(&L.seg->count[L.buf], total);
      if (b + total > L.cap) L.seg->overflow = 1;
    }
    base = b; // (lane 0's value is broadcast where it is used: no wait for the atomic here)
  }
};

// wave 0: entry h of the waiting ring goes into slot `prob`: tracker pointer, ticket, state machine started, first items staged.
// st / trk: LDS scratch of the caller.  stepped: the value of the new state's `stepped` flag (1 when the admission happens inside an
// evaluation launch: the tick's LM launch must leave the newcomer alone).
__device__ __forceinline__ void tick_admit_entry(int mode, long long h, int prob, const TrackerDev **trackers, LMState *states, LMState &st, TrackerDev &trk,
                                                 const TickList &L, TickModeCtl *mc, const TickPending *pending,
                                                 unsigned long long *slot_ticket, int lane, int stepped) {
  const TickPending &Pn = pending[h & (mc->ring - 1)];
  const TrackerDev *tp = Pn.trk;
  stage_in(trk, tp, lane, 64);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  if (lane == 0) {
    trackers[prob] = tp;
    slot_ticket[prob] = Pn.ticket;
    lm_start_problem(trk, st, mode, Pn.start);
    st.stepped = stepped;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  stage_out(&states[prob], st, lane, 64);
  tick_push(st, prob, L, mc, lane);
}

// wave 0, inside a tick: the slot whose problem just retired takes the next waiting problem (if any) on the spot.
__device__ __forceinline__ void tick_try_admit(int mode, int prob, const TrackerDev **trackers, LMState *states, LMState &st, TrackerDev &trk,
                                               const TickList &L, TickModeCtl *mc,
                                               const TickPending *pending, unsigned long long *slot_ticket, int lane, int stepped) {
  // pending_head / pending_count are monotonic over the life of the stream (the waiting list is a ring the host appends to while the
  // device consumes): an index is taken by compare-and-swap so that the head never runs past the count -- an overshoot would skip
  // entries the host appends later.  (Few problems retire in one tick, so the swap is rarely contended; the start of an advance,
  // where every free slot wants an entry at once, goes through tick_reserve_kernel instead.)
  long long h = -1;
  if (lane == 0) {
    const long long cnt = __hip_atomic_load(&mc->pending_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    long long cur = __hip_atomic_load(&mc->pending_head, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (cur < cnt) {
      const long long seen = (long long)atomicCAS((unsigned long long *)&mc->pending_head, (unsigned long long)cur, (unsigned long long)(cur + 1));
      if (seen == cur) {
        h = cur;
        break;
      }
      cur = seen;
    }
  }
  h = ((long long)__builtin_amdgcn_readfirstlane((int)(h >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)h);
  if (h < 0) return;
  tick_admit_entry(mode, h, prob, trackers, states, st, trk, L, mc, pending, slot_ticket, lane, stepped);
}

// wave 0, after a problem's LM step (state in `st`, already written back): a running problem stages its next evaluation; a terminated
// one writes its result and its slot takes the next waiting problem on the spot
__device__ __forceinline__ void tick_after_step(int mode, int prob, const TrackerDev **trackers, LMState *states, LMState &st, TrackerDev &trk,
                                                const TickList &L, TickModeCtl *mc, const TickPending *pending, TickResult *results,
                                                unsigned long long *slot_ticket, int lane, int stepped, int res_base = 0, int res_total = 0) {
  if (st.status == ST_RUNNING) {
    tick_push(st, prob, L, mc, lane, res_base, res_total);
    return;
  }
  for (int i = lane; i < res_total; i += 64) // (cannot happen: a step that proposes does not terminate -- tests/test_tick_lists.py, E)
    if (res_base + i < L.cap) L.items[res_base + i] = kTickNoop;
  if (lane == 0) {
    const long long r = (long long)atomicAdd((unsigned long long *)&mc->retired, 1ull); // monotonic; the host never lets more problems in than the result ring has room for
    TickResult &R = results[r & (mc->ring - 1)];
    const LMState &F = st;
    R.ticket = slot_ticket[prob];
    R.status = F.status;
    R.ticks = F.ticks;
    for (int i = 0; i < 7; i++) R.cur[i] = F.cur[i];
    R.aff_cur[0] = F.aff_cur[0], R.aff_cur[1] = F.aff_cur[1];
    R.flow[0] = F.flow[0], R.flow[1] = F.flow[1], R.flow[2] = F.flow[2];
    R.scale_cur = F.scale_cur;
    for (int l = 0; l < DSM_MAX_LEVELS; l++) {
      R.last_residuals[l] = F.last_residuals[l];
      R.evals[l] = F.evals[l], R.evals_ro[l] = F.evals_ro[l], R.rounds[l] = F.rounds[l];
    }
  }
  tick_try_admit(mode, prob, trackers, states, st, trk, L, mc, pending, slot_ticket, lane, stepped);
}

// Start of an advance, on the context's stream before the stream groups fork (nothing else touches the stream's state then): one
// workgroup hands the entries of the waiting rings to the free slots -- admit_idx[slot] = ring index or -1.  Where fewer problems
// wait than slots are free, the segments (stream groups) of a kind share them in proportion to their free slots.  (Every free
// slot taking its entry by compare-and-swap on the one head word cost 250-350 us per advance: a retry per winner.)
__global__ __launch_bounds__(256) void tick_reserve_kernel(TickReserveArgs a, const LMState *__restrict__ states, TickModeCtl *__restrict__ mcs,
                                                           long long *__restrict__ admit_idx) {
  __shared__ int nfree[kTickMaxSegs], take[kTickMaxSegs], wave_tot[4], running;
  __shared__ long long base[kTickMaxSegs];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (tid < kTickMaxSegs) nfree[tid] = 0;
  __syncthreads();
  for (int si = 0; si < a.nseg; si++) {
    int c = 0;
    for (int j = tid; j < a.seg[si].ns; j += 256) c += states[a.seg[si].i0 + j].status != ST_RUNNING;
    if (c) atomicAdd(&nfree[si], c);
  }
  __syncthreads();
  if (tid == 0) {
    for (int mode = 0; mode < 2; mode++) {
      long long F = 0;
      for (int si = 0; si < a.nseg; si++)
        if (a.seg[si].mode == mode) F += nfree[si];
      const long long head = __hip_atomic_load(&mcs[mode].pending_head, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const long long cnt = __hip_atomic_load(&mcs[mode].pending_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      long long A = cnt - head;
      if (A < 0) A = 0;
      long long given = 0;
      for (int si = 0; si < a.nseg; si++)
        if (a.seg[si].mode == mode) {
          take[si] = F <= A ? nfree[si] : (int)(A * nfree[si] / (F > 0 ? F : 1));
          given += take[si];
        }
      for (int si = 0; si < a.nseg && F > A && given < A; si++) // (the rounding's remainder: one more each, from the first segment on)
        if (a.seg[si].mode == mode && take[si] < nfree[si]) take[si]++, given++;
      long long b = head;
      for (int si = 0; si < a.nseg; si++)
        if (a.seg[si].mode == mode) base[si] = b, b += take[si];
      __hip_atomic_store(&mcs[mode].pending_head, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  __syncthreads();
  for (int si = 0; si < a.nseg; si++) {
    if (tid == 0) running = 0;
    __syncthreads();
    for (int j0 = 0; j0 < a.seg[si].ns; j0 += 256) {
      const int j = j0 + tid;
      const bool fr = j < a.seg[si].ns && states[a.seg[si].i0 + j].status != ST_RUNNING;
      const unsigned long long m = __ballot(fr);
      if (lane == 0) wave_tot[wv] = __popcll(m);
      __syncthreads();
      int r = running + __popcll(m & ((1ull << lane) - 1ull));
      for (int w = 0; w < wv; w++) r += wave_tot[w];
      if (j < a.seg[si].ns) admit_idx[a.seg[si].i0 + j] = fr && r < take[si] ? base[si] + r : -1ll;
      __syncthreads();
      if (tid == 0) running += wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3];
      __syncthreads();
    }
  }
}
void launch_tick_reserve(hipStream_t s, const TickReserveArgs &a, const LMState *states, TickModeCtl *mcs, long long *admit_idx) {
  hipLaunchKernelGGL(tick_reserve_kernel, dim3(1), dim3(256), 0, s, a, states, mcs, admit_idx);
}

// start of an advance: the free slots take the entries tick_reserve_kernel gave them
__global__ __launch_bounds__(64) void tick_admit_kernel(int mode, const TrackerDev **trackers, LMState *states, TickList L, TickModeCtl *mc,
                                                        const TickPending *pending, unsigned long long *slot_ticket,
                                                        const long long *__restrict__ admit_idx) {
  const int prob = blockIdx.x;
  __shared__ __attribute__((aligned(16))) LMState st;
  __shared__ __attribute__((aligned(16))) TrackerDev trk;
  const long long h = admit_idx[prob];
  if (h < 0) return;
  stage_in(st, &states[prob], threadIdx.x, 64); // (fields the start does not write keep their old bits: none is read)
  tick_admit_entry(mode, h, prob, trackers, states, st, trk, L, mc, pending, slot_ticket, threadIdx.x, 0);
}
void launch_tick_admit(hipStream_t s, int mode, int nslots, const TrackerDev **trackers, LMState *states, const TickList &list, TickModeCtl *mc,
                       const TickPending *pending, unsigned long long *slot_ticket, const long long *admit_idx) {
  hipLaunchKernelGGL(tick_admit_kernel, dim3(nslots), dim3(64), 0, s, mode, trackers, states, list, mc, pending, slot_ticket, admit_idx);
}

// end of a chain, wave 0: the rounds beyond the first did not cost the problem a tick; state written back with the `stepped` flag up
// (this tick's LM launch leaves the slot alone), then what tick_lm_kernel does after a step
template <int MODE>
__device__ __attribute__((noinline)) void tick_chain_finish(DSM_LDS LmShared *shp, int prob, int rounds, const DSM_LDS TickChainArgs *cap, int lane) {
  LmShared &sh = *(LmShared *)shp;
  const TickChainArgs ca = *(const TickChainArgs *)cap; // (an LDS copy: a by-value struct would go through the stack of EVERY workgroup of the launch)
  if (lane == 0) {
    if (rounds > 1) sh.st.ticks -= rounds - 1;
    sh.st.stepped = 1;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  stage_out(&ca.states[prob], sh.st, lane, 64);
  tick_after_step(MODE, prob, ca.trackers, ca.states, sh.st, sh.trk, ca.next, ca.mc, ca.pending, ca.results, ca.slot_ticket, lane, 1);
}

// The tick's evaluation launch.  Items [0, count): (problem, chunk) evaluations of all levels mixed, their partials go to memory for
// tick_lm_kernel.  Chain entries [cap, cap + chain): problems whose pending evaluation is ONE chunk (the small pyramid levels -- half of
// a frame's LM rounds on the metric's pyramid, every level of a semi-dense template).  Nothing but this workgroup takes part in such a
// round, so the workgroup that evaluates the chunk also steps the problem -- state and descriptor in LDS, the partial never leaves it --
// and goes on to the NEXT round, for as long as the staged evaluation stays one chunk (at most max_rounds): the rounds that cost a frame
// a tick each (two launches, one trip of the state through memory, a wait for the tick's largest item) cost an evaluation and a step.
// Same chunk, same partial, same reduction order: bit-identical results.  The first workgroups of the grid take the chains (they run
// longest), the others stride over the items.
// CHAIN = false: the launch of a stream that never took in a problem the chains apply to (the host knows: dsm_stream's chain_possible) --
// the items alone, without the chains' code, LDS and stack behind them (the streamed bench of dense templates measured 1.2 % slower
// with them merely present: profiles/r06_ab_lm_opts.log).
template <int MODE, bool CHAIN>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(4))) void tick_eval_kernel(const LMState *__restrict__ states,
                                                                                                  float *__restrict__ partials, int partial_stride,
                                                                                                  const unsigned *__restrict__ items,
                                                                                                  TickSegCtl *__restrict__ seg, int buf, int cap, TickChainArgs ca) {
  __shared__ float red[16][kNumSlots];
  const int n_items = ((const DSM_GLOBAL TickSegCtl *)seg)->count[buf];
  const int n_chain = CHAIN ? ((const DSM_GLOBAL TickSegCtl *)seg)->chain[buf] : 0;
  int nc_wg = (int)(gridDim.x >> 1);
  nc_wg = n_chain < nc_wg ? n_chain : nc_wg;
  if (CHAIN && (int)blockIdx.x < nc_wg) {
    __shared__ LmShared sh;
    __shared__ __attribute__((aligned(16))) float part[kPartialStride];
    __shared__ TickChainArgs s_ca;
    const int tid = threadIdx.x;
    if (tid == 0) s_ca = ca;
    for (int ci = blockIdx.x; ci < n_chain; ci += nc_wg) {
      const int prob = (int)((const DSM_GLOBAL unsigned *)items)[cap + ci];
      stage_in(sh.st, &ca.states[prob], tid, kThreads);
      stage_in(sh.trk, ca.trackers[prob], tid, kThreads);
      __syncthreads();
      int rounds = 0;
      for (;;) {
        const int status = __builtin_amdgcn_readfirstlane(sh.st.status), lvl = __builtin_amdgcn_readfirstlane(sh.st.lvl);
        const int spec_valid = __builtin_amdgcn_readfirstlane(sh.st.spec_valid);
        EvalConsts c;
        eval_consts_from_lds(sh.st.in, c);
        const int nch = chunks_of(c.n, c.ppt);
        // one more round while the staged evaluation is one chunk (or none: an empty level), up to the bound: every tick waits for its
        // longest workgroup, and a chain that ran on alone would make every other resident problem wait (measured: the bound of 8)
        if (status != ST_RUNNING || nch > 1 || spec_valid || rounds >= ca.max_rounds) break; // workgroup-uniform
        if (nch == 1) {
          DSM_EVAL_CHUNK_DEEP(MODE, c, lvl, 0, tid, red, part);
          if (tid == 0) {
            atomicAdd((unsigned long long *)&ca.mc->sched_evals[lvl], 1ull);
            if (c.residual_only) atomicAdd((unsigned long long *)&ca.mc->sched_ro[lvl], 1ull);
            atomicAdd((unsigned long long *)&ca.mc->sched_items[lvl], 1ull);
          }
        }
        __syncthreads();
        tick_chain_round<MODE>((DSM_LDS LmShared *)&sh, (const DSM_LDS float *)part, nch, lvl, tid, (ca.flags & 1) != 0);
        rounds++;
      }
      if (tid < 64) tick_chain_finish<MODE>((DSM_LDS LmShared *)&sh, prob, rounds, (const DSM_LDS TickChainArgs *)&s_ca, tid);
      __syncthreads(); // sh is restaged for the next entry
    }
    return;
  }
  for (int it = (int)blockIdx.x - nc_wg; it < n_items; it += (int)gridDim.x - nc_wg) {
    const unsigned item = ((const DSM_GLOBAL unsigned *)items)[it];
    if (item & kTickNoop) continue; // (workgroup-uniform)
    const bool cand = (item & kTickCand) != 0;
    const int prob = (int)((item & ~(kTickNoop | kTickCand)) >> kTickChunkBits), chunk = (int)(item & ((1u << kTickChunkBits) - 1u));
    const DSM_GLOBAL LMState &S = ((const DSM_GLOBAL LMState *)states)[prob];
    const DSM_GLOBAL EvalIn &in = cand ? S.spec_in : S.in;
    const int lvl = S.lvl;
    EvalConsts c;
    DSM_EVAL_CONSTS_FROM_GLOBAL(c, in);
    float *const out = partials + (size_t)prob * partial_stride + (cand ? (partial_stride >> 1) : 0) + (size_t)chunk * kPartialStride;
    DSM_EVAL_CHUNK_DEEP(MODE, c, lvl, chunk, threadIdx.x, red, out); // (the two-point loop here too: this kernel is allocated 128 registers by its level-0 loop anyway)
    __syncthreads(); // red[] is reused by the next item (the arrival-ticket form of eval_kernel measured the same here: profiles/r05_ab_tick_arrival_ticket.log)
  }
}
void launch_tick_eval(hipStream_t s, int mode, int grid, const LMState *states, float *partials, int partial_stride, const unsigned *items,
                      TickSegCtl *seg, int buf, int cap, const TickChainArgs &chain, bool with_chains) {
  if (grid < 2) grid = 2; // (at least one workgroup for the items beside one for the chains)
  with_constant<2>(mode, [&](auto m) {
    with_constant<2>(with_chains, [&](auto ch) {
      hipLaunchKernelGGL((tick_eval_kernel<decltype(m)::value, decltype(ch)::value != 0>), dim3(grid), dim3(kThreads), 0, s, states, partials, partial_stride,
                         items, seg, buf, cap, chain);
    });
  });
}

template <int MODE>
__global__ __launch_bounds__(kLmThreads) void tick_lm_kernel(const TrackerDev **trackers, LMState *__restrict__ states, const float *__restrict__ partials,
                                                             int partial_stride, TickList next, TickModeCtl *__restrict__ mc,
                                                             const TickPending *__restrict__ pending, TickResult *__restrict__ results,
                                                             unsigned long long *__restrict__ slot_ticket, int speculate, int opts) {
  const int prob = blockIdx.x, tid = threadIdx.x;
  LMState &S = states[prob];
  __shared__ LmShared sh;
  __shared__ LmSpecShared sps;
  // the list this tick's evaluation launch consumed (every workgroup of it has finished): empty again for the tick after the next.
  // (Not by the evaluation launch itself: its chains append to the other list while it runs.)
  if (prob == 0 && tid == 0) next.seg->count[next.buf ^ 1] = 0, next.seg->chain[next.buf ^ 1] = 0;
  // ONE round trip for everything the step must know before it can ask for the partials: the slot's status and kind, the level and point
  // count of the pending evaluation, the tracker pointer -- and this thread's block of the state itself
  const int s_stepped = S.stepped;
  const LmHead hd = lm_read_head(S, trackers, prob, tid);
  if (s_stepped) { // a chain of this tick's evaluation launch stepped the slot (and staged, retired or refilled it)
    if (tid == 0) S.stepped = 0;
    return;
  }
  if (!(hd.status == ST_RUNNING && hd.kind == MODE)) return; // a free slot (refilled by the next advance's admit launch)
  // the speculative second candidate (dsm_params.speculate): on the small levels, as in the launch form (a tick's launch is
  // never bound by the doubled rows of a few small problems)
  const bool spec_lvl = speculate >= 2 || (speculate == 1 && hd.pre.n_lvl <= 8192);
  TickReserve rsv{next, 0, 0};
  lm_step_block<false, TickReserve>(MODE, hd.lvl, prob, hd.Tg, S, partials + (size_t)prob * partial_stride, sh, tid, nullptr, spec_lvl ? &sps : nullptr,
                                    partial_stride >> 1, &hd.pre, (opts & 2) ? &rsv : nullptr, (opts & 1) != 0);
  if (tid >= 64) return;
  const int res_base = __builtin_amdgcn_readfirstlane(rsv.base);
  tick_after_step(MODE, prob, trackers, states, sh.st, sh.trk, next, mc, pending, results, slot_ticket, tid, 0, res_base, rsv.total);
}
void launch_tick_lm(hipStream_t s, int mode, int nslots, const TrackerDev **trackers, LMState *states, const float *partials, int partial_stride,
                    const TickList &next, TickModeCtl *mc, const TickPending *pending, TickResult *results, unsigned long long *slot_ticket,
                    int speculate, int opts) {
  with_constant<2>(mode, [&](auto m) {
    hipLaunchKernelGGL((tick_lm_kernel<decltype(m)::value>), dim3(nslots), dim3(kLmThreads), 0, s, trackers, states, partials, partial_stride, next, mc,
                       pending, results, slot_ticket, speculate, opts);
  });
}

} // namespace dsm
