// form_queue.hpp -- the work-queue form of the tracker kernels (a part of tracker_kernels.hip, see the map at the top of that file):
// one launch of persistent workgroups that pull (problem, chunk) items from a device-side queue.
#pragma once

namespace dsm {

// ------------------------------------------------------------------------------------------
// queue_kernel: the whole call in ONE launch of persistent workgroups pulling (problem, chunk) items from a
// device-side queue.  The workgroup that completes a problem's evaluation (arrival ticket) performs its LM step
// and pushes the chunks of the problem's next evaluation, so every problem advances at its own pace: no
// lock-step launches sized for the slowest problem, no idle workgroups, LM steps overlapped with other
// problems' evaluations.  Same chunks, same partials, same reduction order as the launch-per-step path:
// bit-identical results.  Everything one workgroup writes and another reads inside the launch (queue
// items, partials, LMState, tickets) uses device-scope accesses; the XCD L2s are not mutually coherent.
// The grid is sized for co-residency (occupancy query) because that is what performs; correctness does not depend
// on it: the queue is seeded by its own launch and a workgroup only ever waits for an item that some running
// workgroup will publish.  One queue kernel per context at a time (the header and ring belong to the context).
// Waits are bounded and raise q->error instead of hanging.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned q_load(const unsigned *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// whole wave: append `nitems` chunk items of problem `prob`.  The caller has made the problem's new state visible.
// A ring slot is reused only after its previous item has been READ (the reader stores 0 into it): a workgroup that
// is delayed between taking its ticket and reading its slot can therefore never find the slot overwritten, however
// far the other problems have advanced meanwhile.
__device__ __forceinline__ void queue_push(WorkQueue *q, unsigned long long *items, unsigned qmask, int prob, int nitems, int lane) {
  unsigned base = 0;
  if (lane == 0) base = atomicAdd(&q->tail, (unsigned)nitems);
  base = (unsigned)__builtin_amdgcn_readfirstlane((int)base);
  for (int i = lane; i < nitems; i += 64) {
    const unsigned idx = base + (unsigned)i;
    unsigned long long *slot = &items[idx & qmask];
    for (unsigned spins = 0; __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0ull; spins++) {
      if (spins > (1u << 22)) { // never hang the GPU
        __hip_atomic_store(&q->error, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        break;
      }
      __builtin_amdgcn_s_sleep(8);
    }
    __hip_atomic_store(slot, ((unsigned long long)(idx + 1u) << 32) | ((unsigned)prob << kQueueChunkBits) | (unsigned)i,
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// The first evaluation of every problem enters the queue in a launch of its own (one wave per problem, after
// LM_OP_START): the persistent kernel's progress then never depends on which of its workgroups are resident.
__global__ __launch_bounds__(256) void queue_seed_kernel(int mode, const LMState *__restrict__ states, WorkQueue *__restrict__ q,
                                                         unsigned long long *__restrict__ items, unsigned qmask, int nprob) {
  const int p = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (p >= nprob) return;
  const LMState &S0 = states[p];
  if (S0.status == ST_RUNNING && S0.is_scale == mode) {
    const int nch = chunks_of(S0.in.n, S0.in.ppt);
    queue_push(q, items, qmask, p, nch > 0 ? nch : 1, lane);
  } else if (lane == 0) {
    atomicAdd(&q->done, 1u);
  }
}

template <int MODE>
__global__ __launch_bounds__(kThreads, 4) void queue_kernel(const TrackerDev *const *__restrict__ trackers, LMState *__restrict__ states,
                                                         float *__restrict__ partials, int partial_stride, int *__restrict__ tickets,
                                                         WorkQueue *__restrict__ q, unsigned long long *__restrict__ items, unsigned qmask,
                                                         int nprob) {
  __shared__ LmShared sh;
  __shared__ float red[16][kNumSlots];
  __shared__ __attribute__((aligned(16))) EvalIn s_in;
  __shared__ int s_ctl[4]; // problem (-1: leave), chunk, level, "last arrival" flag
  const int tid = threadIdx.x;

  constexpr int kIn16 = sizeof(EvalIn) / 16;
  static_assert(sizeof(EvalIn) % 16 == 0 && kIn16 < 63, "EvalIn is staged with 16-byte copies by wave 0");
  for (;;) {
    // wave 0 takes an item and stages the problem's evaluation inputs; three workgroup barriers per item in all
    if (tid < 64) {
      unsigned it = 0xFFFFFFFFu;
      if (tid == 0) {
        const unsigned t = atomicAdd(&q->head, 1u);
        for (unsigned spins = 0;; spins++) {
          const unsigned long long v = __hip_atomic_load(&items[t & qmask], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if ((unsigned)(v >> 32) == t + 1u) {
            it = (unsigned)v;
            __hip_atomic_store(&items[t & qmask], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); // slot free again
            break;
          }
          if (q_load(&q->done) >= (unsigned)nprob || q_load((const unsigned *)&q->error)) break;
          if (spins > (1u << 22)) { // ~ a second of polling: something is wrong -- never hang the GPU
            __hip_atomic_store(&q->error, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            break;
          }
          __builtin_amdgcn_s_sleep(8);
        }
      }
      it = (unsigned)__builtin_amdgcn_readfirstlane((int)it);
      if (it != 0xFFFFFFFFu) {
        xwg_acquire(); // the item's publication tag announced the problem's new state
        const LMState &Sp = states[it >> kQueueChunkBits];
        if (tid < kIn16) ((uint4 *)&s_in)[tid] = load16_coherent((const uint4 *)&Sp.in + tid);
        if (tid == kIn16) s_ctl[2] = __hip_atomic_load(&Sp.lvl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      if (tid == 0) {
        s_ctl[0] = it == 0xFFFFFFFFu ? -1 : (int)(it >> kQueueChunkBits);
        s_ctl[1] = (int)(it & ((1u << kQueueChunkBits) - 1u));
      }
    }
    __syncthreads();
    const int prob = s_ctl[0], chunk = s_ctl[1];
    if (prob < 0) break; // workgroup-uniform
    LMState &S = states[prob];
    const int lvl = __builtin_amdgcn_readfirstlane(s_ctl[2]);
    EvalConsts c;
    eval_consts_from_lds(s_in, c);
    const int nch = chunks_of(c.n, c.ppt);
    const int nitems = nch > 0 ? nch : 1; // an empty level still needs its LM step
    float *partials_prob = partials + (size_t)prob * partial_stride;
    if (chunk < nch) {
      if (lvl == 0)
        eval_chunk<MODE, true>(c, chunk, tid, true, red, partials_prob + (size_t)chunk * kPartialStride); // (no LDS window here: the kernel's LDS holds the LM
                                                                                                   // step's workspace; a tile-ordered template is gathered -- the same sums)
      else
        eval_chunk<MODE, false>(c, chunk, tid, true, red, partials_prob + (size_t)chunk * kPartialStride);
    }
    if (tid < 64) { // the chunk's partial was stored by threads of wave 0 only (eval_chunk's final sum)
      xwg_release(); // the partial is performed at device scope before the arrival ticket
      if (tid == 0) {
        const int tk = atomicAdd(&tickets[prob], 1);
        const int last = tk == nitems - 1;
        if (last) __hip_atomic_store(&tickets[prob], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_ctl[3] = last;
      }
    }
    __syncthreads();
    if (s_ctl[3]) { // workgroup-uniform: the problem's evaluation is complete -> its LM step, then its next evaluation
      xwg_acquire(); // the other chunks' partials were announced by their tickets
      lm_step_block<true>(MODE, lvl, prob, trackers[prob], S, partials_prob, sh, tid, nullptr);
      if (tid < 64) {
        xwg_release(); // new state (and the ticket reset) performed at device scope before the items appear
        if (sh.st.status == ST_RUNNING) {
          const int nn = chunks_of(sh.st.in.n, sh.st.in.ppt);
          queue_push(q, items, qmask, prob, nn > 0 ? nn : 1, tid);
        } else if (tid == 0) {
          atomicAdd(&q->done, 1u);
        }
      }
    }
    // no barrier here: wave 0 rewrites s_ctl[0..2] / s_in only after every wave has passed the barrier above, and all
    // waves read them before the evaluation; the next writes of red[] / sh / s_ctl[3] follow the next item's first barrier
  }
}

int queue_kernel_blocks_per_cu(int mode) {
  int nb = 0;
  with_constant<3>(mode, [&](auto m) { hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, queue_kernel<decltype(m)::value>, kThreads, 0); });
  return nb;
}

void launch_queue(hipStream_t s, int mode, int nblocks, int nprob, const TrackerDev *const *trackers, LMState *states,
                  float *partials, int partial_stride, int *tickets, WorkQueue *q, unsigned long long *items, unsigned qmask) {
  hipLaunchKernelGGL(queue_seed_kernel, dim3((nprob + 3) / 4), dim3(256), 0, s, mode, states, q, items, qmask, nprob);
  with_constant<3>(mode, [&](auto m) {
    hipLaunchKernelGGL((queue_kernel<decltype(m)::value>), dim3(nblocks), dim3(kThreads), 0, s, trackers, states, partials, partial_stride, tickets,
                       q, items, qmask, nprob);
  });
}

} // namespace dsm
