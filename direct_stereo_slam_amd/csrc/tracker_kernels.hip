// tracker_kernels.hip -- hand-written gfx950 (CDNA4) kernels of the direct photometric hot path.
//
//   eval_kernel<MODE, ...>    fused calcResPose+calcGSSSEPose (TrackerAndScaler.cpp:699-852,
//                              640-697) or calcResScale+calcGSSSEScale (:1007-1172, :966-1005)
//                              for a batch of independent problems: grid = (chunks, problems).
//   lm_kernel                  per problem: fixed-order reduction of the chunk partials and one
//                              step of the Levenberg-Marquardt state machine of
//                              trackNewestCoarse (:451-638) / optimizeScale (:854-964).
//   queue / tick / chain forms the same evaluation and step under the other schedulers, the diagnostic LM kernels,
//                              and desc_scatter_kernel (descriptors of a batch in one launch).
// The template helpers live in template_kernels.hip, the pyramid and frame helpers in frame_kernels.hip.
//
// Map.  This is ONE translation unit in layers; the headers below belong to it alone, are included nowhere else, open namespace dsm
// themselves and rely on what stands before them here (they include nothing):
//   wave_ops.hpp      DPP row sums, vector types, DSM_GLOBAL / DSM_LDS, lane masks.  First: the evaluation core and the LM step's
//                     reductions (fvec4) both use it.
//   (this file)       the evaluation core: taps, EvalConsts, eval_chunk_impl, eval_chunk -- the per-point loop of every form.
//                     Then with_constant, the launchers' run-time mode -> template argument dispatch.
//   lm_step.hpp       the LM state machine: make_eval_*, wave_ldlt_solve8, propose_*, reduce_partials_*, lm_step_wave0, lm_step_block;
//                     stage_in / stage_out, load16_coherent / store16_coherent, g_lm_spin_expired and lm_spin_expired().
//   form_launch.hpp   launch-per-step form: eval_kernel, lm_start_problem, lm_kernel, launch_eval, launch_lm.
//   form_queue.hpp    work-queue form: queue_seed_kernel, queue_kernel, queue_kernel_blocks_per_cu, launch_queue.
//   form_chain.hpp    chain form: tick_chain_round, chain_kernel, launch_chain.
//   form_tick.hpp     tick engine: tick_push, admission, tick_chain_finish, tick_eval_kernel, tick_lm_kernel, the five launch_tick_*.
//                     After form_chain.hpp (tick_chain_round) and form_launch.hpp (lm_start_problem).
//   form_diag.hpp     diag_chain_eval_kernel, diag_lm_propose_kernel, diag_lm_step_kernel, diag_tick_stage_kernel, diag_tick_fill_kernel,
//                     diag_tick_unpack_kernel and their launchers.  Last: the tick diagnostics run form_tick.hpp's device functions.
//   (this file)       desc_scatter_kernel.
// Why one translation unit: g_lm_spin_expired must have one copy, and the two noinline functions tick_chain_round / tick_chain_finish
// are shared by the kernels that call them; build time is no reason to split (a full compile takes about 16 s).
// Why the evaluation core stays in this file: bench.py hashes tracker_kernels.hip by name (kernel_source_sha) to decide whether a
// stored PMC profile still speaks for the evaluation loop, so the loop must stay in the file that is hashed.
// The generated code of these kernels is sensitive to how the source is spelled (tools/experiments/README.md, "Kernel source
// tidy-ups"): compare the device assembly before and after any edit here or in the headers with tools/isa_compare.py.
//
// Numerics contract: compiled with -ffp-contract=off; every per-point
// value (warp, bounds test, bilinear taps, residual, Huber weight, cut-off test) is computed
// with the same IEEE float32 operation sequence as the CPU oracle, so the integer outputs
// (numTermsInE, numSaturated, warped count) are bit-exact.  Sums are reduced in a fixed tree
// (thread-sequential -> 16-lane DPP rows -> 16 rows sequential -> chunks sequential in
// double): deterministic run to run, equal to the reference's SSE lane order only up to
// float rounding (quirk Q4 is a CPU artefact, not reproduced).  No float atomics.
#include "../../include/dsm_hotpath.h"
#include "dsm_kernels.hpp"
#include "lm_math.hpp"
#include "xwg_sync.hpp"
#include <type_traits>

#include "wave_ops.hpp"

namespace dsm {

// getInterpolatedElement33 (upstream DSO), call sites TrackerAndScaler.cpp:790,1106, split in two
// so that the tap loads of one point can be in flight while the previous point is consumed.
//
// The target lives in HBM as its intensities only (4 bytes per texel).  The reference's texel is
// (I, dx, dy) with dx = 0.5 (I[x+1] - I[x-1]), dy = 0.5 (I[y+1] - I[y-1]) (upstream DSO FrameHessian::makeImages), so the
// interpolated gradients follow from a 4 x 4 neighbourhood of intensities of which only 12 values are needed:
//   rows y, y+1: columns x-1 .. x+2 (two 16-byte loads),  rows y-1, y+2: columns x, x+1 (two 8-byte loads)
// -- as many vector-memory instructions and registers as four 12-byte texels, one third of the image bytes.
struct Taps {
  float r1[4], r2[4]; // rows y, y+1: columns x-1 .. x+2
  float r0[2], r3[2]; // rows y-1, y+2: columns x, x+1
  float dx, dy;       // fractional position
};

// The four row bases of a target plane (wave-uniform, kept in SGPRs): every tap load of a point then shares ONE 32-bit
// vector offset (global_load with saddr + voffset, no 64-bit vector address arithmetic).
struct TapBases {
  const DSM_GLOBAL char *r0, *r1, *r2, *r3;
};
__device__ __forceinline__ TapBases tap_bases(const DSM_GLOBAL float *img, int w) {
  const DSM_GLOBAL char *cb = (const DSM_GLOBAL char *)img;
  const long pitch = 4l * w;
  return TapBases{cb - pitch, cb - 4, cb + pitch - 4, cb + 2 * pitch};
}
// byte offset of the taps of position (x, y): texel (floor x, floor y), or the safe texel (2, 2) for lanes outside `ok` -- ONE
// select, on the finished offset (an unusable lane's x / y may be anything, NaN included: its fractions and values are masked later)
__device__ __forceinline__ unsigned tap_offset(float x, float y, int w, lmask ok, unsigned safe_off, float &dx, float &dy) {
  const int ix = (int)x, iy = (int)y;
  // x - (float)(int)x for x >= 0 is exact and equals v_fract_f32(x) (= x - floor(x))
  dx = __builtin_amdgcn_fractf(x);
  dy = __builtin_amdgcn_fractf(y);
  const unsigned off = 4u * ((unsigned)ix + (unsigned)iy * (unsigned)w);
  return sel_u(ok, safe_off, off);
}
// GRAD = false (residual-only evaluations): the intensity needs columns x, x+1 of rows y, y+1 only -- two 8-byte loads.
template <bool GRAD = true>
__device__ __forceinline__ void taps_load(const TapBases &B, float x, float y, int w, lmask ok, unsigned safe_off, Taps &T) {
  const unsigned off = tap_offset(x, y, w, ok, safe_off, T.dx, T.dy);
  if (GRAD) {
    const fvec4u a = *(const DSM_GLOBAL fvec4u *)(B.r1 + off); // (x-1 .. x+2, y)
    const fvec4u b = *(const DSM_GLOBAL fvec4u *)(B.r2 + off); // (x-1 .. x+2, y+1)
    const fvec2u c = *(const DSM_GLOBAL fvec2u *)(B.r0 + off); // (x, x+1; y-1)
    const fvec2u d = *(const DSM_GLOBAL fvec2u *)(B.r3 + off); // (x, x+1; y+2)
    T.r1[0] = a.x, T.r1[1] = a.y, T.r1[2] = a.z, T.r1[3] = a.w;
    T.r2[0] = b.x, T.r2[1] = b.y, T.r2[2] = b.z, T.r2[3] = b.w;
    T.r0[0] = c.x, T.r0[1] = c.y;
    T.r3[0] = d.x, T.r3[1] = d.y;
  } else { // the intensity alone: (x, x+1) of rows y and y+1
    const fvec2u a = *(const DSM_GLOBAL fvec2u *)(B.r1 + off + 4u);
    const fvec2u b = *(const DSM_GLOBAL fvec2u *)(B.r2 + off + 4u);
    T.r1[0] = T.r1[3] = T.r2[0] = T.r2[3] = 0.f;
    T.r1[1] = a.x, T.r1[2] = a.y;
    T.r2[1] = b.x, T.r2[2] = b.y;
    T.r0[0] = T.r0[1] = T.r3[0] = T.r3[1] = 0.f;
  }
}

// h0 (the intensity) decides in/out, Huber and cut-off: exact reference operation order.  g1 / g2 are TWICE the
// interpolated gradients (the 0.5 of the central difference is a power of two: it commutes with every rounding of the
// chain and is folded into the focal length by the caller); they only enter the Jacobian sums, which are compared to
// float tolerance: FMA allowed.  makeImages replaces a non-finite gradient by zero; some tap difference is non-finite
// exactly when the interpolated value is (the weights are finite), which the caller tests per wave: EXACT = the rare
// path that applies the replacement tap by tap.
template <bool EXACT>
__device__ __forceinline__ void taps_gradients(const Taps &T, float w00, float w10, float w01, float w11, float &g1, float &g2) {
  auto fix = [](float d) { return EXACT ? (__builtin_isfinite(d) ? d : 0.0f) : d; };
  const float d00 = fix(T.r1[2] - T.r1[0]), d10 = fix(T.r1[3] - T.r1[1]);
  const float d01 = fix(T.r2[2] - T.r2[0]), d11 = fix(T.r2[3] - T.r2[1]);
  const float e00 = fix(T.r2[1] - T.r0[0]), e10 = fix(T.r2[2] - T.r0[1]);
  const float e01 = fix(T.r3[0] - T.r1[1]), e11 = fix(T.r3[1] - T.r1[2]);
  g1 = __builtin_fmaf(w00, d00, __builtin_fmaf(w10, d10, __builtin_fmaf(w01, d01, w11 * d11)));
  g2 = __builtin_fmaf(w00, e00, __builtin_fmaf(w10, e10, __builtin_fmaf(w01, e01, w11 * e11)));
}
template <bool EXACT, bool GRAD = true>
__device__ __forceinline__ void taps_interp(const Taps &T, float &h0, float &g1, float &g2) {
  const float dx = T.dx, dy = T.dy;
  const float dxdy = dx * dy;
  const float w11 = dxdy, w01 = dy - dxdy, w10 = dx - dxdy, w00 = 1 - dx - dy + dxdy;
  h0 = ((w11 * T.r2[2] + w01 * T.r2[1]) + w10 * T.r1[2]) + w00 * T.r1[1];
  if (GRAD)
    taps_gradients<EXACT>(T, w00, w10, w01, w11, g1, g2);
  else
    g1 = g2 = 0.f;
}

// per-point state carried from the warp stage to the consume stage
struct Warped {
  float u, v, new_idepth, refColor;
  float x, y, id; // scale mode only (rx = M (x,y,1) / id, :1068)
  lmask inb;      // lanes whose point is usable (:786 / :1102): wave-uniform, lives in an SGPR pair
};

// ------------------------------------------------------------------------------------------
// eval kernel
// ------------------------------------------------------------------------------------------
// Wave-uniform inputs of one evaluation (kept in SGPRs): a copy of EvalIn.
struct EvalConsts {
  const float4 *pts;
  const float *img;
  int n, w, h;
  int ppt; // EvalIn::ppt
  float fx, fy, cx, cy;
  float Ki[9];
  float huber;
  float M[9];
  float t[3];
  float aff0, aff1, b0, scale, cutoff, max_energy;
  int residual_only; // EvalIn::residual_only
  int plain;         // EvalIn::plain
  float bx0, bx1, by0, by1, bid; // EvalIn's template bounds
};
// wave-uniform evaluation inputs: global memory (`in`: a const DSM_GLOBAL EvalIn, scalar loads) -> SGPRs.  A macro: as a function that
// takes the address-space-qualified reference the same statements compile to other code in eval_kernel and tick_eval_kernel
// (tools/experiments/README.md, "Kernel source tidy-ups").
#define DSM_EVAL_CONSTS_FROM_GLOBAL(c, in)                                                                                     \
  do {                                                                                                                         \
    c.pts = in.pts, c.img = in.img, c.n = in.n, c.w = in.w, c.h = in.h, c.ppt = in.ppt;                                        \
    c.fx = in.fx, c.fy = in.fy, c.cx = in.cx, c.cy = in.cy, c.huber = in.huber;                                                \
    _Pragma("unroll") for (int i = 0; i < 9; i++) c.Ki[i] = in.Ki[i], c.M[i] = in.M[i];                                        \
    c.t[0] = in.t[0], c.t[1] = in.t[1], c.t[2] = in.t[2];                                                                      \
    c.aff0 = in.aff0, c.aff1 = in.aff1, c.b0 = in.b0, c.scale = in.scale, c.cutoff = in.cutoff, c.max_energy = in.max_energy; \
    c.residual_only = in.residual_only;                                                                                        \
    c.plain = in.plain, c.bx0 = in.bx0, c.bx1 = in.bx1, c.by0 = in.by0, c.by1 = in.by1, c.bid = in.bid;                         \
  } while (0)
// wave-uniform evaluation inputs: LDS -> SGPRs
__device__ __forceinline__ void eval_consts_from_lds(const EvalIn &in, EvalConsts &c) {
  auto rf = [](float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); };
  const unsigned long long pp = (unsigned long long)in.pts, ip = (unsigned long long)in.img;
  c.pts = (const float4 *)(((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(pp >> 32)) << 32) |
                           (unsigned)__builtin_amdgcn_readfirstlane((int)pp));
  c.img = (const float *)(((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(ip >> 32)) << 32) |
                          (unsigned)__builtin_amdgcn_readfirstlane((int)ip));
  c.n = __builtin_amdgcn_readfirstlane(in.n);
  c.ppt = __builtin_amdgcn_readfirstlane(in.ppt);
  c.w = __builtin_amdgcn_readfirstlane(in.w);
  c.h = __builtin_amdgcn_readfirstlane(in.h);
  c.fx = rf(in.fx), c.fy = rf(in.fy), c.cx = rf(in.cx), c.cy = rf(in.cy), c.huber = rf(in.huber);
#pragma unroll
  for (int i = 0; i < 9; i++) c.Ki[i] = rf(in.Ki[i]), c.M[i] = rf(in.M[i]);
  c.t[0] = rf(in.t[0]), c.t[1] = rf(in.t[1]), c.t[2] = rf(in.t[2]);
  c.aff0 = rf(in.aff0), c.aff1 = rf(in.aff1), c.b0 = rf(in.b0), c.scale = rf(in.scale);
  c.cutoff = rf(in.cutoff), c.max_energy = rf(in.max_energy);
  c.residual_only = __builtin_amdgcn_readfirstlane(in.residual_only);
  c.plain = __builtin_amdgcn_readfirstlane(in.plain);
  c.bx0 = rf(in.bx0), c.bx1 = rf(in.bx1), c.by0 = rf(in.by0), c.by1 = rf(in.by1), c.bid = rf(in.bid);
}

// One chunk of one evaluation by 256 threads (tid = 0..255 inside the chunk's thread group):
// the per-point loop, the flow-indicator pass and the fixed-order reduction into the chunk's 52-slot
// partial `out` (global memory in eval_kernel, LDS in the chains).  `red` is this thread group's
// [16][kNumSlots] LDS scratch.  Contains two workgroup barriers: every thread of the workgroup must
// call it.  `active` is true at every call site (a thread group without a chunk does not call); the parameter is still there
// because removing it changes the generated code of 22 kernels (tools/experiments/README.md, "Kernel source tidy-ups").
// RO = residual-only (EvalIn::residual_only): the residual side alone -- energy, counts, flow indicators; no gradients, no
// Jacobian, no normal-equation sums (their partial slots are written as zeros), two tap loads per point instead of four.
// arrive != nullptr (eval_kernel without the fused LM step): instead of a workgroup barrier between the row sums and the
// final sum, every wave takes a ticket on an LDS counter after its rows are written and only the LAST one stays to add the 16
// rows and store the partial -- the same additions in the same order by another wave; the other waves leave at once instead
// of waiting for the slowest wave's gathers (measured: a mid-level workgroup spent a third of its life between the end of
// its first wave's loop and the partial store).
// DEEP: the two-points-per-trip loop with fixed register roles: level 0 everywhere, and every level inside the tick engine's kernel,
// which runs at four waves per SIMD whatever the level.  (Round 5 measured it there on the 16-point chunks of the other levels and saw
// no change, profiles/r05_ab_flow_first_deep16_b1.log; round 6's shader-clock stamps found the one-point loop's items of levels 1-2
// resident 13 % longer than level 0's for the same 4096 points -- 34 % for the residual-only ones, which have two gathers and little
// arithmetic between them -- and the same A/B now gives + 1.3 % frames/s, the kernel 0.61 -> 0.63 of peak: profiles/r06_ab_deep_all_levels.log)
// It also keeps the warp's twelve wave-uniform constants in VGPRs (pose mode; see where they are pinned below); the one-point loop's
// kernels of five waves per SIMD have no registers for that.
// FAST (mode 0; eval_chunk decides, wave-uniform): the template, image and pose facts of eval_facts.hpp hold for this evaluation, so
// the tests they settle are not made -- the quotients' range test with its IEEE-division path, new_idepth > 0, the finiteness tests of
// g1, g2 and h0 with the tap refetch.  Each of them is all-true on every listed lane under the facts: the same masks, the same bits.
template <int MODE, bool LVL0, bool RO, bool DEEP = LVL0, bool FAST = false>
__device__ __forceinline__ void eval_chunk_impl(const EvalConsts &c, int chunk, int tid, bool active, float (*red)[kNumSlots],
                                                float *out, int *arrive = nullptr) {
  const int n = c.n;
  const int P = c.ppt;
  constexpr int NACC = MODE == 1 ? 3 : kNumAcc;
  float acc[NACC];
#pragma unroll
  for (int a = 0; a < NACC; a++) acc[a] = 0.f;
  float E = 0.f;
  int n_terms = 0, n_sat = 0, n_warped = 0;
  float fT = 0.f, fRT = 0.f, fNum = 0.f;
  if (active) {
    const float M0 = c.M[0], M1 = c.M[1], M2 = c.M[2], M3 = c.M[3], M4 = c.M[4], M5 = c.M[5],
                M6 = c.M[6], M7 = c.M[7], M8 = c.M[8];
    const float t0 = c.t[0], t1 = c.t[1], t2 = c.t[2];
    const float cutoff = c.cutoff;
    const float huber = c.huber;
    const float fxl = c.fx, fyl = c.fy, cxl = c.cx, cyl = c.cy;
    const float hfx = 0.5f * fxl, hfy = 0.5f * fyl; // the central differences' 0.5 (see taps_interp)
    const int wl = c.w, hl = c.h;
    const float wm3 = (float)(wl - 3), hm3 = (float)(hl - 3);
    const int pitch = wl; // floats per row of what the taps are fetched from
    const TapBases img = tap_bases((const DSM_GLOBAL float *)c.img, wl);
    const DSM_GLOBAL fvec4 *pts = (const DSM_GLOBAL fvec4 *)c.pts;
    // scale mode: (scale * M) is formed once per evaluation, as `scale * rot_f1_f0_K0_i` is (:1061)
    const float sc = c.scale;
    const float S0 = sc * M0, S1 = sc * M1, S2 = sc * M2, S3 = sc * M3, S4 = sc * M4, S5 = sc * M5,
                S6 = sc * M6, S7 = sc * M7, S8 = sc * M8;
    const float aff0 = c.aff0, aff1 = c.aff1, b0 = c.b0;

    const int chunk_start = chunk * kThreads * P;

    // Software-pipelined, branch-free loop.  Stage A warps template point k+1 and issues its four
    // bilinear tap loads; stage B consumes the taps of point k (residual, Huber, Jacobian, 45 FMAs)
    // while those loads are in flight.  Predicates are lane masks (see "Lane masks" in wave_ops.hpp): unusable lanes fetch from a safe
    // address and their values are ANDed to zero, so the accumulators never cross a divergent join.
    const lmask full = __builtin_amdgcn_ballot_w64(true);
    unsigned safe_off = 4u * (2u + 2u * (unsigned)pitch); // byte offset of texel (2, 2): held in a VGPR (a select takes no SGPR besides its mask)
    asm volatile("" : "+v"(safe_off));
    // The warp's twelve constants in VGPRs: an SGPR source costs an instruction 4.65 instead of 2.5 cycles (level-0 loop: 1163 -> 1111
    // cycles per two points).  The register budget of four waves per SIMD (128) has room for these and no more.
    float vM0 = M0, vM1 = M1, vM2 = M2, vM3 = M3, vM4 = M4, vM5 = M5, vM6 = M6, vM7 = M7, vM8 = M8, vt0 = t0, vt1 = t1, vt2 = t2;
    if (DEEP && MODE == 0) asm volatile("" : "+v"(vM0), "+v"(vM1), "+v"(vM2), "+v"(vM3), "+v"(vM4), "+v"(vM5), "+v"(vM6), "+v"(vM7), "+v"(vM8), "+v"(vt0), "+v"(vt1), "+v"(vt2));
    auto stage_a = [&](const fvec4 &p, lmask in_list, Warped &W, Taps &T) {
      const float x = p.x, y = p.y, id = p.z;
      float pt0, pt1, pt2;
      if (MODE == 0) { // :747
        pt0 = ((vM0 * x + vM1 * y) + vM2) + vt0 * id;
        pt1 = ((vM3 * x + vM4 * y) + vM5) + vt1 * id;
        pt2 = ((vM6 * x + vM7 * y) + vM8) + vt2 * id;
      } else if (MODE == 2) { // PoseEstimator.cpp:192: pt = R (x,y,z) + t ; the float4 is (x, y, z, refColor[lvl])
        pt0 = ((M0 * x + M1 * y) + M2 * id) + t0;
        pt1 = ((M3 * x + M4 * y) + M5 * id) + t1;
        pt2 = ((M6 * x + M7 * y) + M8 * id) + t2;
      } else { // :1061
        pt0 = ((S0 * x + S1 * y) + S2) + t0 * id;
        pt1 = ((S3 * x + S4 * y) + S5) + t1 * id;
        pt2 = ((S6 * x + S7 * y) + S8) + t2 * id;
      }
      // u = pt0/pt2, v = pt1/pt2, new_idepth = id/pt2 (:748-752).  u and v position the bilinear
      // taps and decide in/out, so they must equal the IEEE quotients bit for bit; new_idepth only
      // enters the sign test and the Jacobian.  The three quotients share one refined reciprocal
      // and use the hardware's own correction sequence (what `a / d` expands to) without the
      // range scaling / fix-up instructions, which are identities for ordinary operands: 2^-33 <= |pt2| < 2^32 and
      // |id| >= 2^-64 or id = 0.  A wave that holds a lane outside that range takes the full IEEE divisions instead.
      {
        const float apt2 = __builtin_fabsf(pt2);
        lmask ordinary = DSM_FCMP(apt2, 0x1p-33f, kOGE) & DSM_FCMP(apt2, 0x1p32f, kOLT);
        if (MODE != 2) ordinary &= DSM_FCMP(__builtin_fabsf(id), 0x1p-64f, kOGE) | DSM_FCMP(id, 0.0f, kOEQ);
        if (!FAST && __builtin_expect(ordinary != full, 0)) {
          W.u = pt0 / pt2;
          W.v = pt1 / pt2;
          W.new_idepth = (MODE == 2 ? 1.0f : id) / pt2; // PoseEstimator.cpp:197: 1 / pt[2]
        } else {
          const float r0 = __builtin_amdgcn_rcpf(pt2);
          const float r1 = __builtin_fmaf(__builtin_fmaf(-pt2, r0, 1.0f), r0, r0);
          auto quot = [pt2, r1](float a) {
            const float q0 = a * r1;
            const float q1 = __builtin_fmaf(__builtin_fmaf(-pt2, q0, a), r1, q0);
            return __builtin_fmaf(__builtin_fmaf(-pt2, q1, a), r1, q1);
          };
          W.u = quot(pt0);
          W.v = quot(pt1);
          W.new_idepth = MODE == 2 ? r1 : id * r1;
        }
      }
      const float Ku = fxl * W.u + cxl, Kv = fyl * W.v + cyl;
      W.refColor = p.w;
      W.x = x, W.y = y, W.id = id;
      // :786 / :1102 (every comparison is false for a NaN, as in the reference)
      W.inb = in_list & DSM_FCMP(Ku, 2.0f, kOGT) & DSM_FCMP(Kv, 2.0f, kOGT) & DSM_FCMP(Ku, wm3, kOLT) & DSM_FCMP(Kv, hm3, kOLT);
      if (!FAST) W.inb &= DSM_FCMP(W.new_idepth, 0.0f, kOGT); // (FAST: id >= 2^-64 and 2^-21 <= pt2 < 2^31, the product is positive or +inf)
      taps_load<!RO>(img, Ku, Kv, pitch, W.inb, safe_off, T); // (unusable lanes fetch around texel (2, 2))
    };
    auto stage_b = [&](const Warped &W, const Taps &T) {
      float h0, g1, g2;
      taps_interp<false, !RO>(T, h0, g1, g2);
      // makeImages' "non-finite gradient -> 0", the rare path: the taps are fetched again (so that the common path
      // does not keep twelve registers alive for it) and the replacement is applied tap by tap
      if (!FAST && !RO && __builtin_expect((W.inb & ~(lanes_finite(g1) & lanes_finite(g2))) != 0ull, 0)) {
        Taps Tx;
        taps_load(img, fxl * W.u + cxl, fyl * W.v + cyl, wl, W.inb, safe_off, Tx);
        taps_interp<true>(Tx, h0, g1, g2);
      }
      const float refColor = W.refColor;
      const lmask fin = FAST ? W.inb : W.inb & lanes_finite(h0); // :791 (FAST: a bilinear sum of pixels of magnitude <= 2^100)
      const float residual = MODE != 1 ? h0 - (aff0 * refColor + aff1) : h0 - refColor; // :793 / :1109
      const float ar = __builtin_fabsf(residual);
      // Huber weight (:794-795): 1 for |r| < huber, huber / |r| beyond.  It is off the per-point decision path (in/out, cut-off):
      // it only scales this point's terms of E and of the normal equations -- sums that are compared to tolerance, E then
      // entering the LM accept test like any other rounding of the sum -- so the hardware reciprocal (1 ulp) replaces the IEEE
      // division and the branch is a minimum (huber / |r| > 1 exactly where |r| < huber, up to that ulp; 1 for r = 0).
      const float hw = __builtin_fminf(1.0f, huber * __builtin_amdgcn_rcpf(ar));
      const lmask sat = DSM_FCMP(ar, cutoff, kOGT); // :797
      const lmask use = fin & ~sat;
      // integer outputs are counted per wave on the scalar unit (s_bcnt1 of the lane masks)
      n_terms += __builtin_popcountll(fin);
      n_sat += __builtin_popcountll(fin & sat);
      n_warped += __builtin_popcountll(use);
      const unsigned m = lane_bits(use);
      // :809 for the usable lanes; a saturated lane's term is the constant max_energy (:800): n_sat x max_energy joins E where the
      // partials are reduced (build_rs)
      E += and_f(hw * residual * residual * (2 - hw), m);
      const float wgt = and_f(hw, m);
      if (RO) {
        // nothing else: the sums below feed calcGSSSE*, whose output the ending loop never reads
      } else if (MODE != 1) {
        // calcGSSSEPose :658-678 on the values calcResPose would have buffered (:812-819); masked
        // lanes get all-zero inputs so that they add exact zeros
        const float u = and_f(W.u, m), v = and_f(W.v, m), nid = and_f(W.new_idepth, m);
        const float dx = and_f(g1 * hfx, m), dy = and_f(g2 * hfy, m); // dxInterp = hitColor[1] * fx (:814), 0.5 folded
        float J[9];
        J[0] = nid * dx;
        J[1] = nid * dy;
        J[2] = -(nid * __builtin_fmaf(u, dx, v * dy));
        J[3] = -__builtin_fmaf(u * v, dx, dy * __builtin_fmaf(v, v, 1.0f));
        J[4] = __builtin_fmaf(u * v, dy, dx * __builtin_fmaf(u, u, 1.0f));
        J[5] = __builtin_fmaf(u, dy, -(v * dx));
        J[6] = and_f(aff0 * (b0 - refColor), m);
        J[7] = -1.0f;
        J[8] = and_f(residual, m);
        int idx = 0;
  #pragma unroll
        for (int r = 0; r < 9; r++) { // Accumulator9::updateSSE_eighted: H(r,c) += (J_r w) J_c
          const float Jw = J[r] * wgt;
  #pragma unroll
          for (int c = r; c < 9; c++) {
            acc[idx] = __builtin_fmaf(Jw, J[c], acc[idx]);
            idx++;
          }
        }
      } else {
        // calcResScale :1068 and calcGSSSEScale :983-999
        const float x = W.x, y = W.y, id = W.id;
        const float rx1 = ((M0 * x + M1 * y) + M2) / id;
        const float rx2 = ((M3 * x + M4 * y) + M5) / id;
        const float rx3 = ((M6 * x + M7 * y) + M8) / id;
        const float dxfx = g1 * hfx, dyfy = g2 * hfy;
        const float deno_sqrt = sc * rx3 + t2;
        const float deno = 1.0f / (deno_sqrt * deno_sqrt);
        const float xno = rx1 * t2 - rx3 * t0;
        const float yno = rx2 * t2 - rx3 * t1;
        const float J0 = and_f(dxfx * (deno * xno) + dyfy * (deno * yno), m);
        const float J1 = and_f(residual, m);
        const float J0w = J0 * wgt;
        acc[0] = __builtin_fmaf(J0w, J0, acc[0]);
        acc[1] = __builtin_fmaf(J0w, J1, acc[1]);
        acc[2] = __builtin_fmaf(J1 * wgt, J1, acc[2]);
      }
    };

    // flow indicators (:754-784 / :1070-1100): level 0, every 32nd template index.  Two waves handle the 8*P such points of this chunk
    // in a single pass.  In the two-point loop's kernels (FLOW_FIRST) the pass runs BEFORE the loop, its point load travelling with the
    // first template entries the workgroup has to wait for anyway, and its three row sums wait in the reduction scratch instead of
    // in registers: after the loop the pass was a dependent HBM round trip plus four divisions in front of the reduction -- 5 k of a
    // level-0 workgroup's 65 k cycles (shader-clock stamps, profiles/r05_queue_probe_and_geometry.log); same operations on the same
    // values, same row sums: the same bits.  Measured: tick_eval_kernel + 2.4 %, stream + 1.4 % (profiles/r05_ab_flow_first.log).
    constexpr bool FLOW_FIRST = LVL0 && DEEP;
    auto flow_pass = [&]() {
    if (LVL0 && tid < 8 * P) {
      const int i = chunk_start + 32 * tid;
      if (i < n) {
        const fvec4 p = pts[i];
        const float x = p.x, y = p.y, id = p.z;
        const float *Ki = c.Ki;
        if (MODE == 2) {
          // PoseEstimator.cpp:185-229, as written: shifts are measured against the reference
          // projection (Ku0,Kv0) and the "translation only" points use (x, y, 1)
          const float z = id;
          const float Ku0 = fxl * (x / z) + cxl, Kv0 = fyl * (y / z) + cyl;
          const float ptz = ((M6 * x + M7 * y) + M8 * z) + t2;
          const float Ku = fxl * ((((M0 * x + M1 * y) + M2 * z) + t0) / ptz) + cxl;
          const float Kv = fyl * ((((M3 * x + M4 * y) + M5 * z) + t1) / ptz) + cyl;
          const float KuT = fxl * ((x + t0) / (1.0f + t2)) + cxl, KvT = fyl * ((y + t1) / (1.0f + t2)) + cyl;
          const float KuT2 = fxl * ((x - t0) / (1.0f - t2)) + cxl, KvT2 = fyl * ((y - t1) / (1.0f - t2)) + cyl;
          const float p3z = ((M6 * x + M7 * y) + M8) - t2;
          const float Ku3 = fxl * ((((M0 * x + M1 * y) + M2) - t0) / p3z) + cxl;
          const float Kv3 = fyl * ((((M3 * x + M4 * y) + M5) - t1) / p3z) + cyl;
          fT += (KuT - Ku0) * (KuT - Ku0) + (KvT - Kv0) * (KvT - Kv0);
          fT += (KuT2 - Ku0) * (KuT2 - Ku0) + (KvT2 - Kv0) * (KvT2 - Kv0);
          fRT += (Ku - Ku0) * (Ku - Ku0) + (Kv - Kv0) * (Kv - Kv0);
          fRT += (Ku3 - Ku0) * (Ku3 - Ku0) + (Kv3 - Kv0) * (Kv3 - Kv0);
        } else {
          float kx0, kx1, kx2, rx0, rx1, rx2;
          if (MODE == 0) {
            kx0 = (Ki[0] * x + Ki[1] * y) + Ki[2];
            kx1 = (Ki[3] * x + Ki[4] * y) + Ki[5];
            kx2 = (Ki[6] * x + Ki[7] * y) + Ki[8];
            rx0 = (M0 * x + M1 * y) + M2;
            rx1 = (M3 * x + M4 * y) + M5;
            rx2 = (M6 * x + M7 * y) + M8;
          } else {
            kx0 = ((sc * Ki[0]) * x + (sc * Ki[1]) * y) + (sc * Ki[2]);
            kx1 = ((sc * Ki[3]) * x + (sc * Ki[4]) * y) + (sc * Ki[5]);
            kx2 = ((sc * Ki[6]) * x + (sc * Ki[7]) * y) + (sc * Ki[8]);
            rx0 = (S0 * x + S1 * y) + S2;
            rx1 = (S3 * x + S4 * y) + S5;
            rx2 = (S6 * x + S7 * y) + S8;
          }
          const float a0 = t0 * id, a1 = t1 * id, a2 = t2 * id;
          const float ptz = rx2 + a2;
          const float Ku = fxl * ((rx0 + a0) / ptz) + cxl, Kv = fyl * ((rx1 + a1) / ptz) + cyl;
          const float pTz = kx2 + a2;
          const float KuT = fxl * ((kx0 + a0) / pTz) + cxl, KvT = fyl * ((kx1 + a1) / pTz) + cyl;
          const float pT2z = kx2 - a2;
          const float KuT2 = fxl * ((kx0 - a0) / pT2z) + cxl, KvT2 = fyl * ((kx1 - a1) / pT2z) + cyl;
          const float p3z = rx2 - a2;
          const float Ku3 = fxl * ((rx0 - a0) / p3z) + cxl, Kv3 = fyl * ((rx1 - a1) / p3z) + cyl;
          fT += (KuT - x) * (KuT - x) + (KvT - y) * (KvT - y);
          fT += (KuT2 - x) * (KuT2 - x) + (KvT2 - y) * (KvT2 - y);
          fRT += (Ku - x) * (Ku - x) + (Kv - y) * (Kv - y);
          fRT += (Ku3 - x) * (Ku3 - x) + (Kv3 - y) * (Kv3 - y);
        }
        fNum += 2;
      }
    }
    };
    {
      // Template stream: entry (start + tid) of the list = one coalesced 16-byte load per lane from a wave-uniform base (SGPR pair)
      // plus this thread's constant byte offset -- no per-point index arithmetic.  The two-point loop fetches the entries of the wave's
      // trips and one more (its last steady trip prefetches for a trip that is peeled), the one-point loop two more; such an entry is
      // never used: its lanes are masked, and an entry past the list reads as zeros (the buffer descriptor checks the range).
      const unsigned voff = 16u * (unsigned)tid;
      const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)c.pts, 0, 16 * n, 0x00020000);
      auto load_pt = [=](int start) {
        // streamed once: non-temporal (aux = 2), so the template does not evict target rows from the 32 KiB L1 (+2.5 %).
        // buffer_load ... offen: descriptor and the trip's byte offset in SGPRs, this thread's constant offset in a VGPR -- no vector
        // address arithmetic at all; an entry beyond the list reads as zeros (range-checked by the descriptor).
        const uvec4 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, 16 * start, 2);
        return fvec4{__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w)};
      };
      // lanes whose entry `start + tid` exists and whose trip belongs to the chunk: every lane except in the list's last chunk
      const bool tail = chunk_start + kThreads * P > n;
      auto listed = [=](int start, bool trip) -> lmask {
        if (!trip) return 0ull;
        return mask_sgpr(tail ? (lmask)__builtin_amdgcn_sicmp(tid, n - start, kSLT) : full);
      };
      // This wave's trip bound: the trips in which one of its lanes holds a point of the list, at least one (a wave wholly past the
      // list runs one masked trip: no zero-trip case) -- P in every chunk but the list's last, where the loop used to run P trips
      // whatever the chunk held.  Wave-uniform (an SGPR).  stage_b is still called for this thread's points k = 0 .. Pw - 1 in that
      // order and is the only place the accumulators, E and the counts are added to; what the trips from Pw on added were and_f(.., 0)
      // to E, popcount(0) to the counts and fma(+-0, x, acc) to accumulators that are never -0: the bits stay what they were.
      int Pw = P;
      if (tail) {
        const int left = n - chunk_start - (__builtin_amdgcn_readfirstlane(tid) & ~63); // points from this wave's first lane on
        const int trips = (left + kThreads - 1) / kThreads;                              // (kThreads is a power of two: a shift)
        Pw = left <= 0 ? 1 : trips < P ? trips : P;
      }
      const int i = chunk_start;
      const fvec4 p0 = load_pt(i);
      if (DEEP) {
        // Level 0 (long loops, HBM-resident targets): two points per trip with FIXED register roles (sets a / b).
        // The taps of point k+1 are issued before the arithmetic of point k and awaited only after the taps of
        // point k+2 have been issued, so two points' gathers are in flight per wave; template entries are fetched
        // two points ahead.  (The rotating single-body loop below makes the compiler copy the freshly loaded tap
        // registers at the back-edge, which waits for them -- vmcnt(0) -- and leaves only the arithmetic of one
        // point to cover the memory latency; it needs 7 VGPRs less, which is one more resident wave per SIMD and
        // worth more than the deeper pipeline on the small, cache-resident levels: level 0 +5 %, levels 1-3 -7..-10 %
        // with this form.)  Points beyond the chunk / the list are masked (they add exact zeros), so odd P needs
        // no special case.
        fvec4 ea = load_pt(i + kThreads), eb = load_pt(i + 2 * kThreads);
        if (FLOW_FIRST) {
          flow_pass();
          const float sT = row16_sum(fT), sRT = row16_sum(fRT), sN = row16_sum(fNum);
          if ((tid & 15) == 0) {
            const int row_ = (tid >> 6) * 4 + ((tid & 63) >> 4);
            red[row_][kSlotFlowT] = sT, red[row_][kSlotFlowRT] = sRT, red[row_][kSlotFlowNum] = sN;
          }
          fT = fRT = fNum = 0.f;
        }
        __builtin_amdgcn_s_waitcnt(0); // drain the prologue loads so the loop's waits only cover its own loads
        Warped Wa, Wb;
        Taps Ta, Tb;
        stage_a(p0, listed(i, true), Wa, Ta);
        int ia = i + kThreads; // start of the entries held in ea (eb: ia + kThreads)
        // The last trip is peeled: it has no point k+2 to warp and nothing to fetch.  (As a trip of the loop it made the call under an
        // empty lane mask -- 18 warp operations, the quotients, the compares and four gathers at the safe texel, P + 1 warp stages for
        // P points -- and loaded two entries past the chunk.)  The steady trip is what it was.
        int k = 0;
        for (; k + 2 < Pw; k += 2) {
          stage_a(ea, listed(ia, true), Wb, Tb); // point k+1
          ea = load_pt(ia + 2 * kThreads);
          stage_b(Wa, Ta); // point k
          stage_a(eb, listed(ia + kThreads, true), Wa, Ta); // point k+2
          eb = load_pt(ia + 3 * kThreads); // (the last steady trip's is entry Pw, or Pw + 1 at odd Pw: the one entry fetched and not used)
          stage_b(Wb, Tb); // point k+1
          ia += 2 * kThreads;
        }
        stage_a(ea, listed(ia, k + 1 < Pw), Wb, Tb); // point k+1 (masked when k+1 == Pw: odd Pw)
        stage_b(Wa, Ta); // point k
        stage_b(Wb, Tb); // point k+1
      } else {
        // Template stream prefetched one point ahead.
        int i2 = i + kThreads;
        fvec4 p_next = load_pt(i2);
        __builtin_amdgcn_s_waitcnt(0); // drain the prologue loads so the loop's waits only cover its own loads
        Warped Wc;
        Taps Tc;
        stage_a(p0, listed(i, true), Wc, Tc);
        // Pw trips; the last one's stage A (point Pw) runs under an empty lane mask.  Not peeled as the two-point loop's last trip is: with
        // a second stage B behind the loop the kernels of five waves per SIMD spill (eval_kernel<0 / 2, false, false, *>: 8 and 12 bytes).
        for (int k = 0; k < Pw; k++) {
          // stage A for point k+1 (its template entry was prefetched one iteration ago)
          const fvec4 p = p_next;
          const lmask in_next = listed(i2, k + 1 < Pw);
          const int i3 = i2 + kThreads;
          p_next = load_pt(i3);
          Warped Wn;
          Taps Tn;
          stage_a(p, in_next, Wn, Tn);
          // stage B for point k
          stage_b(Wc, Tc);
          Wc = Wn;
          Tc = Tn;
          i2 = i3;
        }
      }
    }

    if (!FLOW_FIRST) flow_pass();
  } // active
  // ---- workgroup reduction: DPP row sums -> LDS [16 rows][slots] -> fixed-order sum ----
  const int lane = tid & 63, wave = tid >> 6;
  const int row = wave * 4 + (lane >> 4);
  const bool writer = (lane & 15) == 0;
#pragma unroll
  for (int i = 0; i < NACC; i++) {
    const float s = RO ? 0.0f : row16_sum(acc[i]);
    if (writer) red[row][i] = s;
  }
  {
    // flow indicators: level 0 only; `parked`: this thread group's sums already sit in red[][] (FLOW_FIRST above)
    const bool parked = LVL0 && DEEP && active;
    const bool flow_here = LVL0 && !parked;
    const float sE = row16_sum(E), sT = flow_here ? row16_sum(fT) : 0.f, sRT = flow_here ? row16_sum(fRT) : 0.f, sN = flow_here ? row16_sum(fNum) : 0.f;
    // n_terms / n_sat / n_warped are wave totals (identical in every lane): count them once per wave
    const bool first = lane == 0;
    const int iT = first ? n_terms : 0, iS = first ? n_sat : 0, iW = first ? n_warped : 0; // (a row's writer is its lane 0: the wave's first row carries the totals)
    if (writer && !parked) {
      red[row][kSlotFlowT] = sT;
      red[row][kSlotFlowRT] = sRT;
      red[row][kSlotFlowNum] = sN;
    }
    if (writer) {
      red[row][kSlotE] = sE;
      red[row][kSlotNTerms] = __int_as_float(iT);
      red[row][kSlotNSat] = __int_as_float(iS);
      red[row][kSlotNWarped] = __int_as_float(iW);
    }
  }
  int slot = tid;
  if (arrive) {
    // a wave's LDS operations are performed in order: its rows are in place before its ticket is counted
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    int t = 0;
    if (lane == 0) t = __hip_atomic_fetch_add(arrive, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (__builtin_amdgcn_readfirstlane(t) != kThreads / 64 - 1) return; // not the last wave of the workgroup: done
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    slot = lane;
  } else {
    __syncthreads();
  }
  const bool is_float_slot = slot < NACC || (slot >= kSlotE && slot < kSlotNTerms);
  if (!active) {
  } else if (is_float_slot) {
    float s = red[0][slot];
#pragma unroll
    for (int r = 1; r < 16; r++) s += red[r][slot];
    store_partial(out + slot, s);
  } else if (slot >= kSlotNTerms && slot < kNumSlots) {
    int s = 0;
#pragma unroll
    for (int r = 0; r < 16; r++) s += __float_as_int(red[r][slot]);
    store_partial(out + slot, __int_as_float(s));
  }
}

// The three facts of a pose evaluation (eval_facts.hpp), once per chunk: the template and image facts travel with the evaluation's
// inputs (EvalIn::plain and the list's bounds), the pose fact is derived here from this evaluation's M and t -- a dozen vector
// instructions on wave-uniform values, the result an SGPR.  Depends on the problem's own data alone: every form, every chunk of an
// evaluation decides alike.
__device__ __forceinline__ int eval_fast(const EvalConsts &c) {
  const bool fast = c.plain != 0 && pose_fact(c.M[6], c.M[7], c.M[8], c.t[2], c.bx0, c.bx1, c.by0, c.by1, c.bid);
  return __builtin_amdgcn_readfirstlane((int)fast);
}
// fast: eval_fast(c) from the callers that have the FAST instantiation built in (mode 0, the two-point loop: the tick engine's kernel and
// the chains on every level, the launch form's level-0 kernel), 0 = the general instantiation (everything else; queue_kernel, whose
// spill budget has no room for two more loops).  Where the decision is taken matters to the register allocator: with eval_fast inside
// this function tick_eval_kernel<0, false> spilled two registers in the general loop's tap-refetch block (12 bytes of scratch).
template <int MODE, bool LVL0, bool DEEP = LVL0>
__device__ __forceinline__ void eval_chunk(const EvalConsts &c, int chunk, int tid, bool active, float (*red)[kNumSlots],
                                           float *out, int *arrive = nullptr, int fast = 0) {
  const bool take_fast = MODE == 0 && DEEP && fast != 0; // wave-uniform
  if (!take_fast) {
    if (c.residual_only) // wave-uniform
      eval_chunk_impl<MODE, LVL0, true, DEEP>(c, chunk, tid, active, red, out, arrive);
    else
      eval_chunk_impl<MODE, LVL0, false, DEEP>(c, chunk, tid, active, red, out, arrive);
  } else if (c.residual_only) {
    eval_chunk_impl<MODE, LVL0, true, DEEP, MODE == 0 && DEEP>(c, chunk, tid, active, red, out, arrive);
  } else {
    eval_chunk_impl<MODE, LVL0, false, DEEP, MODE == 0 && DEEP>(c, chunk, tid, active, red, out, arrive);
  }
}

// a chunk of whatever level inside the kernels that run at four waves per SIMD (tick_eval_kernel, the chains): the two-point loop on
// every level (DEEP above), the flow indicators on level 0.  lvl is workgroup-uniform.  A macro: as a function the same two calls
// compile to other code in all ten kernels that use it (tools/experiments/README.md, "Kernel source tidy-ups").
#define DSM_EVAL_CHUNK_DEEP(MODE, c, lvl, chunk, tid, red, out)          \
  do {                                                                   \
    const int fast_ = MODE == 0 ? eval_fast(c) : 0;                      \
    if (lvl == 0)                                                        \
      eval_chunk<MODE, true>(c, chunk, tid, true, red, out, nullptr, fast_);             \
    else                                                                 \
      eval_chunk<MODE, false, true>(c, chunk, tid, true, red, out, nullptr, fast_);      \
  } while (0)

// Host side, for the launchers of the forms: a run-time selector as a compile-time constant.  Calls f(Const<I>{}) with I = v for
// 0 <= v < N - 1 and I = N - 1 for every other v -- the `mode == 0 ... else` ladders, written once.  f is a generic lambda that names
// its kernel instantiation by decltype(arg)::value; N bounds what gets instantiated (the tick engine has no mode 2).
template <int I>
using Const = std::integral_constant<int, I>;
template <int N, int I = 0, class F>
static void with_constant(int v, F &&f) {
  if constexpr (I + 1 < N) {
    if (v != I) return with_constant<N, I + 1>(v, f);
  }
  f(Const<I>{});
}

} // namespace dsm

#include "lm_step.hpp"
#include "form_launch.hpp"
#include "form_queue.hpp"
#include "form_chain.hpp"
#include "form_tick.hpp"
#include "form_diag.hpp"

namespace dsm {

// descriptors of many trackers in one copy + one launch (after a batched hand-over every tracker's exposure changed)
__global__ void desc_scatter_kernel(const TrackerDev *__restrict__ src, TrackerDev *const *__restrict__ dst) {
  static_assert(sizeof(TrackerDev) % 16 == 0, "TrackerDev is copied in 16-byte units");
  const uint4 *s = (const uint4 *)(src + blockIdx.x);
  uint4 *d = (uint4 *)dst[blockIdx.x];
  for (int i = threadIdx.x; i < (int)(sizeof(TrackerDev) / 16); i += blockDim.x) d[i] = s[i];
}
void launch_desc_scatter(hipStream_t s, int n, const TrackerDev *d_src, TrackerDev *const *d_dst) {
  if (n > 0) hipLaunchKernelGGL(desc_scatter_kernel, dim3(n), dim3(64), 0, s, d_src, d_dst);
}

} // namespace dsm
