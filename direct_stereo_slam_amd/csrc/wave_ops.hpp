// wave_ops.hpp -- wave64 building blocks of the tracker kernels (a part of tracker_kernels.hip, which includes it first: see the map
// at the top of that file): DPP row sums, the clang vector types and address spaces of the kernels' loads, lane masks.
#pragma once

namespace dsm {

// ------------------------------------------------------------------------------------------
// wave64 helpers: DPP butterflies inside 16-lane rows (v_add_f32 ... quad_perm / row_mirror)
// ------------------------------------------------------------------------------------------
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}
template <int CTRL>
__device__ __forceinline__ int dpp_i(int v) {
  return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, false);
}
// after this every lane holds the sum over its 16-lane row: the balanced tree ((l0 + l1) + (l2 + l3)) + ... over the row's lanes.
// (An add with a DPP operand costs 4.65 cycles where a plain v_add_f32 costs 2.5, and a chunk's 52 row sums are 970 vector cycles per
// wave -- 1.8 points' worth of the loop.  Round 5 tried the exchange through the LDS crossbar instead (ds_swizzle + plain add: the same
// tree, the same bits): level 0 5.2 -> 4.7 TB/s, 61.1 k -> 54.7 k frames/s -- four dependent LDS round trips per sum cost more than they
// save; profiles/r05_ab_swizzle_row_sums.log.)
__device__ __forceinline__ float row16_sum(float v) {
  v = v + dpp_f<0xB1>(v);  // quad_perm [1,0,3,2]
  v = v + dpp_f<0x4E>(v);  // quad_perm [2,3,0,1]
  v = v + dpp_f<0x141>(v); // row_half_mirror
  v = v + dpp_f<0x140>(v); // row_mirror
  return v;
}

// clang vector types: loads through address_space(1) pointers compile on the host pass too
typedef float fvec4 __attribute__((ext_vector_type(4)));
typedef unsigned uvec4 __attribute__((ext_vector_type(4)));
typedef float fvec4u __attribute__((ext_vector_type(4), aligned(4))); // four / two neighbouring texels, dword aligned
typedef float fvec2u __attribute__((ext_vector_type(2), aligned(4)));
#define DSM_GLOBAL __attribute__((address_space(1)))
// the local (LDS) address space: the chains' LDS copies of the state and the partial are addressed through it
#define DSM_LDS __attribute__((address_space(3)))

// ------------------------------------------------------------------------------------------
// Lane masks.  What a vector instruction costs on gfx950 depends on its FORM (tools/microbench/valu_issue_cost.hip,
// profiles/r05_valu_issue_cost_w*.json; cycles a wave64 instruction occupies its SIMD): v_mul / v_add / v_sub / v_fmac / v_and /
// v_mov / v_add_u32 in the 4-byte encoding with VGPR or inline-constant sources 2.5; their 8-byte encodings and v_fma_f32 3.1;
// ANYTHING with an SGPR source, every v_cmp, v_cndmask, v_cvt, v_fract, v_min / v_max, shifts, integer multiplies 4.65; v_rcp 8.5.
// The level-0 loop is bound by exactly that sum (a padding experiment follows it to 1 %: profiles/r05_ab_pad_level0.log), and
// the compiler's handling of C++ bools was a fifth of it: a bool that crosses a loop edge or feeds a ballot is materialised as
// v_cndmask 0/1 + v_cmp_ne (two 4.65-cycle instructions per ballot), `cond ? x : 0` is a 4.65-cycle select per value.  The
// per-point code therefore keeps its predicates as explicit 64-bit lane masks in SGPR pairs -- a compare writes one (its only
// cost), logic and population counts on them are scalar instructions -- turns a mask into all-ones / zero lane bits ONCE
// (one v_cndmask) and masks values with v_and (2.5 cycles).
// ------------------------------------------------------------------------------------------
typedef unsigned long long lmask;
// LLVM's compare predicate codes (llvm.amdgcn.fcmp / icmp)
enum { kOEQ = 1, kOGT = 2, kOGE = 3, kOLT = 4, kSLT = 40 };
#define DSM_FCMP(a, b, pred) ((lmask)__builtin_amdgcn_fcmpf((a), (b), (pred)))
__device__ __forceinline__ lmask lanes_finite(float x) { return DSM_FCMP(__builtin_fabsf(x), __builtin_inff(), kOLT); } // false for NaN
// A lane mask is the same in every lane by construction; where the compiler cannot see that (a mask chosen under a condition it takes
// for divergent) this pins it to an SGPR pair -- no instruction where it already is one.
__device__ __forceinline__ lmask mask_sgpr(lmask m) {
  return ((lmask)(unsigned)__builtin_amdgcn_readfirstlane((int)(m >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)m);
}
// bit set -> t, clear -> f  (v_cndmask_b32 with the mask in an SGPR pair)
__device__ __forceinline__ float sel_f(lmask m, float f, float t) {
  float r;
  asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(f), "v"(t), "s"(mask_sgpr(m)));
  return r;
}
__device__ __forceinline__ unsigned sel_u(lmask m, unsigned f, unsigned t) {
  unsigned r;
  asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(f), "v"(t), "s"(mask_sgpr(m)));
  return r;
}
// all-ones where the lane's bit is set, zero elsewhere (opaque to the optimiser on purpose: `x & lane_bits(m)` stays a v_and)
__device__ __forceinline__ unsigned lane_bits(lmask m) {
  unsigned r;
  asm("v_cndmask_b32_e64 %0, 0, -1, %1" : "=v"(r) : "s"(mask_sgpr(m)));
  return r;
}
__device__ __forceinline__ float and_f(float x, unsigned bits) { return __uint_as_float(__float_as_uint(x) & bits); }

} // namespace dsm
