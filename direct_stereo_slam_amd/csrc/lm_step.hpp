// lm_step.hpp -- the Levenberg-Marquardt state machine of the tracker kernels (a part of tracker_kernels.hip, see the map at the top
// of that file): the inputs of an evaluation (make_eval_*), the wave-parallel LDLT solve, the proposals, the fixed-order reduction of
// the chunk partials and one step of the machine by a wave (lm_step_wave0) or a workgroup (lm_step_block).  Every scheduling form
// (form_*.hpp) steps its problems through these.  Also the 16-byte staging copies between memory and LDS and the bounded-wait counter.
#pragma once

namespace dsm {

// ------------------------------------------------------------------------------------------
// LM state machine.  One workgroup of 256 threads per problem: all four waves reduce the chunk
// partials (fixed order), then wave 0 advances the state machine: the 8x8 normal equations live
// one element per lane (lane = 8*row + col), the pivoted LDLT solve runs across the wave with
// shuffles, lane 0 does the scalar double precision work (SE3 exp, pose composition).
// ------------------------------------------------------------------------------------------
constexpr int kLmThreads = 256;

// The inputs of an evaluation, in parts (round 6 -- an LM step is ONE wave's chain of dependent instructions, every one of them is
// time: shader-clock stamps in profiles/r06_tick_stamps.json had make_eval at 6 k of a step's 22 k cycles):
//   make_eval_level  what depends on the level alone (and, for the scale problem, everything but the scale: R10 K^-1 and tsl_f1_f0 are
//                    constants of the level) -- written ONCE when a level begins, into both candidates' blocks;
//   make_eval_rot    M and t of a proposed pose;  make_eval_aff  affLL of a proposed affine pair (the only exp of the step);
//   make_eval_cutoff cutoff, max_energy, the residual-only mark.
// Every value is formed by the same operations on the same operands as the one-piece form of rounds 1-5: same bits.
// `st`: this lane stores (the callers run on wave-uniform values; lane 0 writes).
__device__ __forceinline__ void make_eval_level(const TrackerDev &T, EvalIn &e, int mode, int lvl) {
  const LevelDev &L = T.lv[lvl];
  float Ki[9];
#pragma unroll
  for (int i = 0; i < 9; i++) Ki[i] = L.Ki[i];
#pragma unroll
  for (int i = 0; i < 9; i++) e.Ki[i] = Ki[i];
  e.pts = L.pts;
  e.img = L.img[mode == 1 ? 1 : 0]; // new left frame (:709) / right frame fh1_ (:1016)
  e.n = L.n;
  e.ppt = pts_per_thread(L.n, T.p.geometry), e.pad0 = 0.f;
  e.plain = 0, e.bx0 = e.bx1 = e.by0 = e.by1 = e.bid = 0.f; // no fact established (make_eval_facts)
  e.w = L.w;
  e.h = L.h;
  if (mode == 1) { // cam-1 intrinsics (:1017-1020)
    e.fx = L.fx1, e.fy = L.fy1, e.cx = L.cx1, e.cy = L.cy1;
  } else {
    e.fx = L.fx, e.fy = L.fy, e.cx = L.cx, e.cy = L.cy;
  }
  e.huber = T.p.huber_th;
  e.b0 = mode == 0 ? (float)T.ref_b : 0.0f; // :646 (pose); the loop-closure estimator's reference has b = 0 (PoseEstimator.cpp:90)
  e.scale = 1.0f;
  if (mode == 1) {
    double Rd[9];
    quat_to_rot(T.T10, Rd);
    float Rf[9];
#pragma unroll
    for (int i = 0; i < 9; i++) Rf[i] = (float)Rd[i];
    float M[9];
    mat3f_mul(Rf, Ki, M); // :1022-1023
#pragma unroll
    for (int i = 0; i < 9; i++) e.M[i] = M[i];
    e.t[0] = (float)T.T10[4]; // :1024
    e.t[1] = (float)T.T10[5];
    e.t[2] = (float)T.T10[6];
    e.aff0 = 1.0f;
    e.aff1 = 0.0f;
  }
}
// The facts the producers of this level's list and plane left behind (eval_facts.hpp), pose mode only: the one part of the level's
// inputs that is read through a pointer -- a round trip to memory in the step's chain, so it is asked for ONCE per level and copied to
// the other candidate's block (begin_level).  (Held across make_eval_rot's double-precision work, which would hide the round trip,
// the six values take tick_lm_kernel<0> from 96 to 98 registers: one wave per SIMD less.)
struct EvalFacts {
  int plain;
  float bx0, bx1, by0, by1, bid;
};
__device__ __forceinline__ EvalFacts load_eval_facts(const TrackerDev &T, int mode, int lvl) {
  const TrackerFacts *F = T.facts;
  const bool known = mode == 0 && F != nullptr;
  const LevelFacts lf = known ? F->lv[lvl] : LevelFacts{};
  const int img_ok = known ? F->img_plain[T.img_set[0] & (kFactImageSets - 1)][lvl] : 0;
  const int general = known ? F->force_general : 1;
  EvalFacts f;
  f.plain = (lf.tpl_plain == 1 && img_ok == 1 && !general) ? 1 : 0;
  f.bx0 = ordered_value(lf.xmin), f.bx1 = ordered_value(lf.xmax), f.by0 = ordered_value(lf.ymin), f.by1 = ordered_value(lf.ymax);
  f.bid = ordered_value(lf.idmax);
  return f;
}
__device__ __forceinline__ void store_eval_facts(EvalIn &e, const EvalFacts &f) {
  e.plain = f.plain, e.bx0 = f.bx0, e.bx1 = f.bx1, e.by0 = f.by0, e.by1 = f.by1, e.bid = f.bid;
}
// pose (mode 0): M = R K^-1 (:715), t (:716); loop-closure pose (mode 2, PoseEstimator.cpp:155-163): M = R.  e.Ki holds the level's K^-1.
__device__ __forceinline__ void make_eval_rot(EvalIn &e, int mode, const double pose[7], bool st) {
  double Rd[9];
  quat_to_rot(pose, Rd);
  float Rf[9];
#pragma unroll
  for (int i = 0; i < 9; i++) Rf[i] = (float)Rd[i];
  float M[9];
  if (mode == 2) {
#pragma unroll
    for (int i = 0; i < 9; i++) M[i] = Rf[i];
  } else {
    float Ki[9];
#pragma unroll
    for (int i = 0; i < 9; i++) Ki[i] = e.Ki[i];
    mat3f_mul(Rf, Ki, M);
  }
  if (st) {
#pragma unroll
    for (int i = 0; i < 9; i++) e.M[i] = M[i];
    e.t[0] = (float)pose[4];
    e.t[1] = (float)pose[5];
    e.t[2] = (float)pose[6];
  }
}
// affLL = fromToVecExposure(lastRef->ab_exposure, new_frame_->ab_exposure, lastRef_aff_g2l, aff_g2l) (:717-720); the loop-closure
// estimator's reference affine is (0, 0) (PoseEstimator.cpp:317)
__device__ __forceinline__ void make_eval_aff(const TrackerDev &T, EvalIn &e, int mode, const double aff[2], bool st) {
  double affd[2];
  aff_from_to(T.ref_exposure, T.exposure[0], mode == 2 ? 0.0 : T.ref_a, mode == 2 ? 0.0 : T.ref_b, aff[0], aff[1], affd);
  if (st) {
    e.aff0 = (float)affd[0];
    e.aff1 = (float)affd[1];
  }
}
__device__ __forceinline__ void make_eval_cutoff(const TrackerDev &T, EvalIn &e, float cutoff, bool residual_only, bool st) {
  const float h = T.p.huber_th;
  if (st) {
    e.cutoff = cutoff;
    e.max_energy = 2 * h * cutoff - h * h; // :726-728 / :1030-1032
    e.residual_only = residual_only ? 1 : 0;
  }
}

// The complete inputs of an evaluation at `lvl` into the problem state: one thread (a level's first evaluation, a single evaluation
// of dsm_tracker_calc_res_*).
__device__ __forceinline__ void make_eval_any(const TrackerDev &T, LMState &S, int mode, int lvl, const double pose[7], const double aff[2],
                              float scale, float cutoff, bool residual_only = false) {
  EvalIn &e = S.in;
  const EvalFacts facts = load_eval_facts(T, mode, lvl); // (asked for in front of the level's own copies)
  make_eval_level(T, e, mode, lvl);
  store_eval_facts(e, facts);
  if (mode == 1) {
    e.scale = scale;
  } else {
    make_eval_rot(e, mode, pose, true);
    make_eval_aff(T, e, mode, aff, true);
  }
  make_eval_cutoff(T, e, cutoff, residual_only, true);
}

// lane 0 only
__device__ __forceinline__ void begin_level(const TrackerDev &T, LMState &S, int lvl) {
  S.lvl = lvl;
  S.phase = PH_INIT;
  S.iteration = 0;
  S.level_cutoff_repeat = 1.0f;
  S.spec_valid = 0;
  const float cutoff = T.p.coarse_cutoff_th * S.level_cutoff_repeat;
  make_eval_any(T, S, S.is_scale, lvl, S.cur, S.aff_cur, S.scale_cur, cutoff);
  make_eval_level(T, S.spec_in, S.is_scale, lvl); // (the speculative candidate's block: a proposal writes its own part only)
  S.spec_in.plain = S.in.plain, S.spec_in.bx0 = S.in.bx0, S.spec_in.bx1 = S.in.bx1, S.spec_in.by0 = S.in.by0, S.spec_in.by1 = S.in.by1;
  S.spec_in.bid = S.in.bid; // (the level's facts: the same for both candidates)
}

// iteration bound of a level: maxIterations[lvl] (:463,:505 / :862,:897), or the benchmark schedule's K (dsm_params.fixed_schedule)
__device__ __forceinline__ int level_max_it(const ParamsDev &p, int lvl) { return p.fixed_schedule > 0 ? p.fixed_schedule : p.max_iterations[lvl]; }

// Vec6 rs of calcResPose / calcResScale (:843-851) from the reduced sums
// The E slot of the partials holds the energy of the USABLE lanes; every saturated lane contributes the evaluation's constant
// max_energy (:800 / :809), added here as n_sat x max_energy (no per-point select for it in the loop).
__device__ __forceinline__ void build_rs(const double *sums, const long long *isums, float max_energy, double rs[6]) {
  const float E = (float)(sums[kSlotE] + (double)max_energy * (double)isums[1]);
  const float sT = (float)sums[kSlotFlowT], sRT = (float)sums[kSlotFlowRT], sN = (float)sums[kSlotFlowNum];
  const int n_terms = (int)isums[0], n_sat = (int)isums[1];
  rs[0] = E;
  rs[1] = n_terms;
  rs[2] = sT / (sN + 0.1);
  rs[3] = 0;
  rs[4] = sRT / (sN + 0.1);
  rs[5] = n_sat / (float)n_terms;
}

__device__ __forceinline__ double scale_of(const ParamsDev &p, int i) { // SCALE_* per tangent index (:685-696)
  return i < 3 ? (double)p.scale_xi_rot : i < 6 ? (double)p.scale_xi_trans : i == 6 ? (double)p.scale_a : (double)p.scale_b;
}

// index of (r,c), r<=c, in the row-major upper triangle of the 9x9 accumulator
__device__ __forceinline__ int tri_idx(int r, int c) { return r * 9 - (r * (r - 1)) / 2 + (c - r); }

// H_out(r,c) of calcGSSSEPose (:681-692) for this lane's (r,c); b_out(r) (:683,:693-696)
__device__ __forceinline__ double build_H_elem(const ParamsDev &p, const double *sums, int n4, int r, int c) {
  const float hf = (float)sums[r <= c ? tri_idx(r, c) : tri_idx(c, r)];
  const float invn = 1.0f / n4; // (1.0f / n), n padded to a multiple of 4 (quirk Q3)
  return (((double)hf * (double)invn) * scale_of(p, c)) * scale_of(p, r);
}
__device__ __forceinline__ double build_b_elem(const ParamsDev &p, const double *sums, int n4, int r) {
  const float hf = (float)sums[tri_idx(r, 8)];
  const float invn = 1.0f / n4;
  return ((double)hf * (double)invn) * scale_of(p, r);
}

// Eigen LDLT<Lower> + solve (call sites :509,:513,:518,:529): the unblocked in-place algorithm restated from its published
// form -- the same restatement the CPU checker (orc_ldlt_solve) carries, and it is THAT checker the
// increments are bit-identical to.  Real Eigen is not in this image and was never run against either: its A21 update goes
// through the gemv kernel (column blocks of four, alpha = -1 folded into the accumulation), so last-bit differences from the
// reference's own solve are possible; the pivot-order argument below does not depend on that.  Executed by one wave on
// wave-uniform data.
//
// Eigen's unblocked LDLT is LEFT-looking: at step k it looks for the first maximum of |diagonal| among the rows not yet
// eliminated, swaps it into position k, and only then applies the pending updates to column k.  The diagonal entries it
// compares have therefore not been touched by the elimination: the whole pivot order is a function of the input diagonal
// alone (a selection sort with Eigen's swap bookkeeping).  That allows a form with a short dependent chain:
//   1. the pivot order from ONE all-pairs comparison of the diagonal (lane (r,c) tests |d_c| > |d_r|; a row's rank is the
//      population count of its byte of the ballot).  Exact ties and NaNs -- where Eigen's swaps, not the ranks, decide --
//      take a literal, sequential restatement of the selection loop instead (wave-uniform rare branch);
//   2. lane i reads row i of the symmetrically permuted lower triangle from the LDS copy of H;
//   3. the factorisation and the substitution passes run fully unrolled with static register indices, one ROW per lane:
//      the d_j A[k][j] products of a step are wave-uniform (lane reads), each lane forms the dot product over its own row
//      -- the update of A(k,k) in lane k, of column k's entries in the lanes below -- and the column is divided by the pivot
//      with ONE division per step; no pivot search and no divergence inside the chain; L^-T gets its columns through a
//      64-word LDS transpose;
//   4. the solution is un-permuted through eight LDS words.
// Every element sees the checker's operations in the checker's order: given bitwise equal H and b the increments are bitwise
// equal to the checker's (not: proven equal to Eigen's, see above).  (The fully wave-uniform form of the same arithmetic -- every lane all 36 entries --
// took 6.8-7.7 k shader cycles, issue-bound by its 36 IEEE double divisions; the cross-lane right-looking form of rounds
// 1-2, another pivot order, 7.7 k.)
// Rows / columns whose bit is clear in `active` do not take part (the 6- and 7-dim sub-solves): they are ordered last and
// enter as zero rows, zero columns and a zero right-hand side, which leaves every operation on the active block unchanged
// (x - 0 * 0 = x) and yields 0 for them.  The padding rows are KEPT zero by selection, not by arithmetic: 0 - 0 * y is a NaN for a
// non-finite y, and would reach the active unknowns through L^-T where the checker's smaller system has no such row.  stitch: row / column 6 of the system is row / column 7 of H (:521-534).
struct LdltScratch {
  double x[8];
  double av[8];
  double L[8][8]; // the factor, for its transpose
  int ix[8];
  int perm[8];
};

__device__ __forceinline__ void wave_ldlt_solve8(const double *Hlds, const double *blds, float lambda, unsigned active, bool stitch,
                                                 int lane, LdltScratch &scr, double inc[8]) {
  const int r = lane >> 3, c = lane & 7;
  const double lam1 = (double)(1 + lambda); // Hl(i,i) *= (1 + lambda): a float sum, widened (:506-508)
  auto src = [stitch](int i) { return stitch && i == 6 ? 7 : i; };
  const int nact = __builtin_popcount(active & 0xFFu);
  // ---- 1. pivot order ----
  int perm[8];
  {
    const double ar = fabs(Hlds[9 * src(r)] * lam1), ac = fabs(Hlds[9 * src(c)] * lam1);
    const bool act_r = (active >> r) & 1u, act_c = (active >> c) & 1u;
    const unsigned long long gt = __ballot(act_r && act_c && ac > ar);
    const bool odd = act_r && ((act_c && r != c && ac == ar) || ar != ar);
    const bool slow = __ballot(odd) != 0ull; // wave-uniform
    const int rank = act_r ? __builtin_popcount((unsigned)(gt >> (8 * r)) & 0xFFu) : nact + __builtin_popcount(~active & ((1u << r) - 1u) & 0xFFu);
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const unsigned long long m = __ballot(c == 0 && rank == k);
      perm[k] = m ? (__builtin_ctzll(m) >> 3) : k;
    }
    if (__builtin_expect(slow, 0)) {
      // Eigen's selection loop as written: first maximum of the remaining diagonal IN ITS CURRENT ARRANGEMENT, swapped to
      // position k (comparisons with NaN are false: a NaN is only ever taken where it already stands)
      if (lane == 0) {
        int n = 0;
        for (int i = 0; i < 8; i++)
          if ((active >> i) & 1u) {
            scr.av[n] = fabs(Hlds[9 * src(i)] * lam1);
            scr.ix[n] = i;
            n++;
          }
        for (int k = 0; k < n; k++) {
          int big = k;
          double bigv = scr.av[k];
          for (int i = k + 1; i < n; i++)
            if (scr.av[i] > bigv) bigv = scr.av[i], big = i;
          const double tv = scr.av[k];
          const int ti = scr.ix[k];
          scr.av[k] = scr.av[big], scr.ix[k] = scr.ix[big];
          scr.av[big] = tv, scr.ix[big] = ti;
        }
        for (int i = 0; i < 8; i++)
          if (!((active >> i) & 1u)) scr.ix[n++] = i;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#pragma unroll
      for (int k = 0; k < 8; k++) perm[k] = __builtin_amdgcn_readfirstlane(scr.ix[k]);
    }
  }
  // ---- 2. the permuted system, ONE ROW PER LANE (row i = lane & 7, replicated in every group of eight lanes): lower
  // triangle of P A P^T (LDLT<Lower> reads the lower triangle of its input), P rhs ----
  const int i = lane & 7;
  int pl = perm[0]; // this lane's unknown (logical index)
#pragma unroll
  for (int k = 1; k < 8; k++) pl = i == k ? perm[k] : pl;
  const int pi = src(pl);
  const bool act_i = i < nact;
  double a[8]; // a[j] = A[i][j], j <= i
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const int pj = src(perm[j]);
    const int hi = pi > pj ? pi : pj, lo = pi > pj ? pj : pi;
    const double v = Hlds[8 * hi + lo];
    const double vd = v * lam1;
    a[j] = (act_i && j <= i) ? (i == j ? vd : v) : 0.0; // (j <= i: j active whenever i is)
  }
  double y = act_i ? -blds[pi] : 0.0;
  // ---- 3. factorisation, left-looking (no pivoting left to do), Eigen's operation order.  At step k every lane forms
  // s = sum_j A[i][j] temp[j] over ITS row -- the dot product of A(k,k)'s update in lane k, the A21 update in the lanes below
  // -- from the wave-uniform temp[j] = d_j A[k][j] (lane reads); ONE division per step instead of 7 - k. ----
  double du[8]; // the diagonal D, wave-uniform
  double d_own = 0.0;
  bool all_zero = false;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    if (k > 0) {
      double sacc = 0;
#pragma unroll
      for (int j = 0; j < k; j++) {
        const double temp = du[j] * lane_value_d(a[j], k);
        sacc += a[j] * temp;
      }
      a[k] = act_i ? a[k] - sacc : 0.0; // (a padding row stays zero by selection: 0 - 0 * NaN would not)
    }
    const double akk = lane_value_d(a[k], k);
    const bool valid = fabs(akk) > 0.0;
    if (k == 0 && !valid) all_zero = true;
    const double q = a[k] / akk;
    a[k] = (i > k && valid && act_i) ? q : a[k];
    du[k] = akk;
    d_own = i == k ? akk : d_own;
  }
  // L^-1: y[i] -= A[i][j] y[j], j ascending (lane j's value is final when its turn comes)
#pragma unroll
  for (int j = 0; j < 7; j++) {
    const double yj = lane_value_d(y, j);
    y = (i > j && act_i) ? y - a[j] * yj : y;
  }
  {
    const double tol = 1.0 / 1.7976931348623157e308; // Eigen: 1 / NumTraits<double>::highest()
    y = fabs(d_own) > tol ? y / d_own : 0.0;
  }
  // L^-T needs column i of L in lane i: transpose through LDS
  if (lane < 8) {
#pragma unroll
    for (int j = 0; j < 8; j++) scr.L[i][j] = a[j];
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  double cl[8];
#pragma unroll
  for (int j = 0; j < 8; j++) cl[j] = scr.L[j][i]; // A[j][i]
  // y[i] -= A[j][i] y[j] for i = 6 .. 0, j = i + 1 .. 7 ascending (Eigen's order); x_j is final once row j is done
  double xu[8];
  xu[7] = lane_value_d(y, 7);
#pragma unroll
  for (int ii = 6; ii >= 0; ii--) {
#pragma unroll
    for (int j = ii + 1; j < 8; j++) y = i == ii ? y - cl[j] * xu[j] : y;
    xu[ii] = lane_value_d(y, ii);
  }
  // ---- 4. P^T: row i of the permuted system is unknown pl ----
  if (lane < 8) scr.x[pl] = (all_zero || !act_i) ? 0.0 : y;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#pragma unroll
  for (int k = 0; k < 8; k++) inc[k] = scr.x[k];
  if (stitch) {
    inc[7] = inc[6];
    inc[6] = 0;
  }
}

// value of an LDS word that another wave of the workgroup writes
__device__ __forceinline__ int lds_flag(const int *p) { return __hip_atomic_load(p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void lds_flag_set(int *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP); }

// A proposing wave's HELPER (round 6).  Of what follows the solve, the affine part of the next evaluation's inputs -- affLL: the
// step's only exp, a division -- and its cut-off need nothing of the new pose: a wave that would otherwise sit idle forms them while
// the proposing wave runs SE3::exp, the pose product and R K^-1.  The proposing wave posts the candidate's affine pair as soon as the
// increment is known, and meets the helper again before it leaves.
struct LmHelp {
  int cmd;  // proposing wave -> helper: 0 wait, 1 go, 2 nothing to do this step
  int done; // helper -> proposing wave
  int spec, last;
  float cutoff, pad;
  double aff[2];
};
constexpr int kLmSpinBound = 1 << 22; // polls of an LDS flag before a wave gives up (seconds; a step is microseconds): waits are bounded
__device__ int g_lm_spin_expired;      // ... and say so: nonzero once any bounded wait of an LM step has expired (read by the host with the statistics)
__device__ __forceinline__ int lds_wait_nonzero(const int *p) {
  int v = 0;
  for (int spins = 0; (v = lds_flag(p)) == 0; spins++) {
    if (spins > kLmSpinBound) {
      atomicAdd(&g_lm_spin_expired, 1);
      return -1;
    }
    __builtin_amdgcn_s_sleep(1);
  }
  return v;
}
int lm_spin_expired() {
  int v = 0;
  if (hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_lm_spin_expired), sizeof v) != hipSuccess) return -1;
  return v;
}
__device__ __forceinline__ void lm_help_wave(const TrackerDev &T, LMState &S, LmHelp &h, int lane) {
  const int cmd = lds_wait_nonzero(&h.cmd);
  if (cmd != 1) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  EvalIn &e = h.spec ? S.spec_in : S.in;
  const double aff[2] = {h.aff[0], h.aff[1]};
  make_eval_aff(T, e, S.is_scale, aff, lane == 0);
  make_eval_cutoff(T, e, h.cutoff, h.last != 0, lane == 0);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  if (lane == 0) lds_flag_set(&h.done, 1);
}

// lane 0 only: :612-637
__device__ __forceinline__ void finish_track(const TrackerDev &T, LMState &S) {
  const float modeA = T.p.affine_opt_mode_a, modeB = T.p.affine_opt_mode_b;
  int status = ST_GOOD;
  if ((modeA != 0 && (__builtin_fabsf((float)S.aff_cur[0]) > 1.2)) ||
      (modeB != 0 && (__builtin_fabsf((float)S.aff_cur[1]) > 200)))
    status = ST_BAD_AFFINE;
  if (status == ST_GOOD) {
    double rel[2];
    aff_from_to(T.ref_exposure, T.exposure[0], T.ref_a, T.ref_b, S.aff_cur[0], S.aff_cur[1], rel);
    const float rel0 = (float)rel[0], rel1 = (float)rel[1];
    if ((modeA == 0 && (__builtin_fabsf(logf(rel0)) > 1.5)) || (modeB == 0 && (__builtin_fabsf(rel1) > 200)))
      status = ST_BAD_AFFINE;
  }
  if (status == ST_GOOD) {
    if (modeA < 0) S.aff_cur[0] = 0;
    if (modeB < 0) S.aff_cur[1] = 0;
  }
  S.status = status;
}

// the unknowns of the pose solve under the affine modes (wave_ldlt_solve8's `active`, `stitch`)
__device__ __forceinline__ void lm_solve_unknowns(const TrackerDev &T, unsigned &active, bool &stitch) {
  const float modeA = T.p.affine_opt_mode_a, modeB = T.p.affine_opt_mode_b;
  active = 0xFFu;
  stitch = false;
  if (modeA < 0 && modeB < 0) { // :511-515 fix a, b
    active = 0x3Fu;
  } else if (!(modeA < 0) && modeB < 0) { // :516-520 fix b
    active = 0x7Fu;
  } else if (modeA < 0 && !(modeB < 0)) { // :521-534 fix a: row/col 6 := row/col 7
    stitch = true;
    active = 0x7Fu;
  }
}

// whole wave: solve + propose for the pose problem (:505-554) from the H, b of the problem state (LDS).
// spec: the proposal is the speculative one (S.spec_*).  hp: this wave's helper (lm_help_wave), or null.
__device__ __forceinline__ void propose_pose(const TrackerDev &T, LMState &S, float lambda, int lane, LdltScratch &scr, bool spec = false,
                                             LmHelp *hp = nullptr) {
  unsigned active;
  bool stitch;
  lm_solve_unknowns(T, active, stitch);
  double inc[8];
  wave_ldlt_solve8(S.H, S.b, lambda, active, stitch, lane, scr, inc);
  // From here on every lane computes the same (wave-uniform) values; lane 0 stores them.  The two
  // sincos evaluations of SE3::exp run side by side in lanes 0 and 1.
  float extrapFac = 1; // :536-539
  const float lim = T.p.lambda_extrapolation_limit;
  if (lambda < lim) extrapFac = sqrtf(sqrtf(lim / lambda));
#pragma unroll
  for (int i = 0; i < 8; i++) inc[i] *= extrapFac;
  double incScaled[8], sum = 0; // :541-548
#pragma unroll
  for (int i = 0; i < 8; i++) {
    incScaled[i] = inc[i] * scale_of(T.p, i);
    sum += incScaled[i];
  }
  if (!__builtin_isfinite(sum)) {
#pragma unroll
    for (int i = 0; i < 8; i++) incScaled[i] = 0;
  }
  double aff_cand[2] = {S.aff_cur[0] + incScaled[6], S.aff_cur[1] + incScaled[7]};
  double nrm = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) nrm += inc[i] * inc[i];
  const double inc_norm = sqrt(nrm);
  // Is this the loop's last evaluation?  The step that consumes it ends the level when the increment is small (:588) or the
  // iteration bound is reached (:505) -- both known now; the speculative proposal is consumed one iteration later.
  const bool last = (T.p.fixed_schedule <= 0 && !(inc_norm > 1e-3)) || S.iteration + (spec ? 2 : 1) >= level_max_it(T.p, S.lvl);
  const float cutoff = T.p.coarse_cutoff_th * S.level_cutoff_repeat;
  EvalIn &e = spec ? S.spec_in : S.in; // (its level part is in place since begin_level)
  if (hp) { // the affine pair and the cut-off go to the helper now; the pose part follows here
    if (lane == 0) {
      hp->aff[0] = aff_cand[0], hp->aff[1] = aff_cand[1];
      hp->cutoff = cutoff;
      hp->last = last ? 1 : 0;
      hp->spec = spec ? 1 : 0;
      lds_flag_set(&hp->cmd, 1);
    }
  }
  double ex[7], cur[7], cand[7];
#pragma unroll
  for (int i = 0; i < 7; i++) cur[i] = S.cur[i];
  se3_exp_wave(incScaled, ex, lane);
  se3_mul(ex, cur, cand); // :550-551
  if (lane == 0) {
    if (spec) {
#pragma unroll
      for (int i = 0; i < 7; i++) S.spec_cand[i] = cand[i];
      S.spec_aff_cand[0] = aff_cand[0];
      S.spec_aff_cand[1] = aff_cand[1];
      S.spec_inc_norm = inc_norm;
    } else {
#pragma unroll
      for (int i = 0; i < 7; i++) S.cand[i] = cand[i];
      S.aff_cand[0] = aff_cand[0];
      S.aff_cand[1] = aff_cand[1];
      S.inc_norm = inc_norm;
      S.phase = PH_ITER;
    }
  }
  make_eval_rot(e, S.is_scale, cand, lane == 0);
  if (hp) {
    (void)lds_wait_nonzero(&hp->done);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  } else {
    make_eval_aff(T, e, S.is_scale, aff_cand, lane == 0);
    make_eval_cutoff(T, e, cutoff, last, lane == 0);
  }
}

// lane 0 only: :897-913
__device__ __forceinline__ void propose_scale(const TrackerDev &T, LMState &S, float lambda, bool spec = false) {
  float Hl = S.Hs;
  Hl *= (1 + lambda);
  float inc = -S.bs / Hl;
  float extrapFac = 1;
  const float lim = T.p.lambda_extrapolation_limit;
  if (lambda < lim) extrapFac = sqrtf(sqrtf(lim / lambda));
  inc *= extrapFac;
  if (!__builtin_isfinite(inc) || __builtin_fabsf(inc) > S.scale_cur) inc = 0.0f;
  const float cand = S.scale_cur + inc;
  if (spec) {
    S.spec_inc_f = inc;
    S.spec_scale_cand = cand;
  } else {
    S.inc_f = inc;
    S.scale_cand = cand;
    S.phase = PH_ITER;
  }
  const bool last = (T.p.fixed_schedule <= 0 && !(inc > 1e-3)) || S.iteration + (spec ? 2 : 1) >= level_max_it(T.p, S.lvl); // :937 (signed, Q7) / :897
  EvalIn &e = spec ? S.spec_in : S.in; // (R10 K^-1, tsl_f1_f0 and the camera are the level's: in place since begin_level)
  e.scale = cand;
  make_eval_cutoff(T, e, T.p.coarse_cutoff_th * S.level_cutoff_repeat, last, true);
}

// lane 0 only
__device__ __forceinline__ void end_level(const TrackerDev &T, LMState &S) {
  const int lvl = S.lvl;
  S.last_residuals[lvl] = sqrtf((float)(S.res_old[0] / S.res_old[1])); // :596 / :945
  S.last_inners[lvl] = S.res_old[1];                                     // PoseEstimator.cpp:463
  if (S.is_scale == 0) {
    S.flow[0] = S.res_old[2]; // :597
    S.flow[1] = S.res_old[3];
    S.flow[2] = S.res_old[4];
    if (T.p.fixed_schedule <= 0 && S.last_residuals[lvl] > 1.5 * S.min_res[lvl]) { // :598
      S.status = ST_ABORTED;
      return;
    }
  }
  int next = lvl - 1;
  if (S.level_cutoff_repeat > 1 && !S.have_repeated) { // :601-604 / :947-950
    next = lvl;
    S.have_repeated = 1;
  }
  if (next < 0) {
    if (S.is_scale == 1)
      S.status = ST_GOOD;
    else
      finish_track(T, S); // the same affine plausibility checks end PoseEstimator::estimate (:470-482)
    return;
  }
  begin_level(T, S, next);
}

// LDS workspace of the partial reduction / LM step (the LM kernels and the chains)
struct RedBuf { // fixed-order reduction of one evaluation's chunk partials
  double psum[19][kNumSlots];
  long long pisum[19][4];
  double sums[kNumSlots];
  long long isums[4];
};
// second reduction buffer and the wave 0 <-> wave 1 hand-shake of a step that handles a speculative candidate
struct LmSpecShared {
  RedBuf red;
  LdltScratch ldlt; // wave 1's
  LmHelp help;      // wave 1's helper (wave 3)
  int cmd;      // wave 0 -> wave 1: 0 wait, 1 stage the speculative proposal with `lambda`, 2 nothing to do
  int done;     // wave 1 -> wave 0
  float lambda;
};
struct LmShared {
  RedBuf red;
  LdltScratch ldlt; // wave 0's
  LmHelp help;      // wave 0's helper (wave 2)
  // The problem's LMState and its tracker descriptor are staged here for the duration of a step
  // (lm_kernel) or of a whole chain (chain_kernel, the tick engine's chains): the state machine then runs on LDS
  // latencies instead of a chain of dependent global-memory round trips.
  __attribute__((aligned(16))) LMState st;
  __attribute__((aligned(16))) TrackerDev trk;
};
static_assert(sizeof(LMState) % 16 == 0 && sizeof(TrackerDev) % 16 == 0, "staged with 16-byte copies");

// 16-byte block copies between global memory and LDS by `nthreads` threads
template <class T>
__device__ __forceinline__ void stage_in(T &dst_lds, const T *src_global, int tid, int nthreads) {
  constexpr int n16 = sizeof(T) / 16;
  const uint4 *src = (const uint4 *)src_global;
  uint4 *dst = (uint4 *)&dst_lds;
  for (int i = tid; i < n16; i += nthreads) dst[i] = src[i];
}
template <class T>
__device__ __forceinline__ void stage_out(T *dst_global, const T &src_lds, int tid, int nthreads) {
  constexpr int n16 = sizeof(T) / 16;
  const uint4 *src = (const uint4 *)&src_lds;
  uint4 *dst = (uint4 *)dst_global;
  for (int i = tid; i < n16; i += nthreads) dst[i] = src[i];
}

// Device-coherent 16-byte accesses (two 8-byte device-scope atomics): for state that one workgroup writes and a
// workgroup on another XCD reads inside the SAME launch (work-queue kernel); the XCD L2s are not coherent with
// each other for ordinary accesses.
__device__ __forceinline__ uint4 load16_coherent(const void *p) {
  const unsigned long long a = __hip_atomic_load((const unsigned long long *)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const unsigned long long b = __hip_atomic_load((const unsigned long long *)p + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  uint4 v;
  v.x = (unsigned)a, v.y = (unsigned)(a >> 32), v.z = (unsigned)b, v.w = (unsigned)(b >> 32);
  return v;
}
__device__ __forceinline__ void store16_coherent(void *p, const uint4 &v) {
  __hip_atomic_store((unsigned long long *)p, ((unsigned long long)v.y << 32) | v.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store((unsigned long long *)p + 1, ((unsigned long long)v.w << 32) | v.z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- fixed-order reduction over the chunk partials (double / int64), first 247 threads of the
// workgroup.  Thread (g, q) sums the slot quad q (one float4 = 4 of the 52 slots) over chunks
// g, g+19, g+38, ...: every load is a 16-byte read and up to kRedBatch of them are in flight per
// thread.  `P` may point to global memory (lm_kernel) or LDS (the chains): same order, same sums.
// reduce_partials_groups2: TWO evaluations' partials -- the main and the speculative candidate's -- reduced side by side, each in
// exactly the order above, their loads requested TOGETHER (two reductions one after the other were two memory round trips in front of
// every LM step of the small levels; shader-clock stamps: profiles/r06_tick_stamps.json).  A speculative candidate exists on levels of at
// most 8192 points only, i.e. at most 32 chunks = two per group: a batch of two is the whole job, and the registers stay few -- an LM
// kernel must fit the hole ONE retiring evaluation wave leaves on a SIMD (128 VGPRs): with 138 the scale segment's LM launches, which
// run beside the pose evaluations, took 68 us instead of 12 (profiles/r06_lm_vgpr_regression.txt).
__device__ __forceinline__ void reduce_partials_groups(const float *P, int nch, int tid, RedBuf &sh) {
  constexpr int kGroups = 19, kQuads = kNumSlots / 4, kRedBatch = 8;
  const int q = tid % kQuads, g = tid / kQuads;
  if (g < kGroups) {
    double sd[4] = {0, 0, 0, 0};
    long long si[4] = {0, 0, 0, 0};
    for (int c0 = g; c0 < nch; c0 += kGroups * kRedBatch) {
      fvec4 v[kRedBatch];
#pragma unroll
      for (int j = 0; j < kRedBatch; j++) {
        const int cc = c0 + j * kGroups;
        v[j] = cc < nch ? load_partial4(P + ((size_t)cc * (kPartialStride / 4) + q) * 4) : fvec4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int j = 0; j < kRedBatch; j++) {
        sd[0] += (double)v[j].x, sd[1] += (double)v[j].y, sd[2] += (double)v[j].z, sd[3] += (double)v[j].w;
        si[0] += __float_as_int(v[j].x), si[1] += __float_as_int(v[j].y), si[2] += __float_as_int(v[j].z),
            si[3] += __float_as_int(v[j].w);
      }
    }
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const int slot = 4 * q + e;
      if (slot < kSlotNTerms)
        sh.psum[g][slot] = sd[e];
      else
        sh.pisum[g][slot - kSlotNTerms] = si[e];
    }
  }
}
__device__ __forceinline__ void reduce_partials_groups2(const float *P, const float *P2, int nch, int tid, RedBuf &sh, RedBuf &sh2) {
  constexpr int kGroups = 19, kQuads = kNumSlots / 4, kRedBatch = 2;
  const int q = tid % kQuads, g = tid / kQuads;
  if (g < kGroups) {
    double sd[4] = {0, 0, 0, 0}, td[4] = {0, 0, 0, 0};
    long long si[4] = {0, 0, 0, 0}, ti[4] = {0, 0, 0, 0};
    for (int c0 = g; c0 < nch; c0 += kGroups * kRedBatch) {
      fvec4 v[kRedBatch], w[kRedBatch];
#pragma unroll
      for (int j = 0; j < kRedBatch; j++) {
        const int cc = c0 + j * kGroups;
        v[j] = cc < nch ? load_partial4(P + ((size_t)cc * (kPartialStride / 4) + q) * 4) : fvec4{0.f, 0.f, 0.f, 0.f};
        w[j] = cc < nch ? load_partial4(P2 + ((size_t)cc * (kPartialStride / 4) + q) * 4) : fvec4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int j = 0; j < kRedBatch; j++) {
        sd[0] += (double)v[j].x, sd[1] += (double)v[j].y, sd[2] += (double)v[j].z, sd[3] += (double)v[j].w;
        si[0] += __float_as_int(v[j].x), si[1] += __float_as_int(v[j].y), si[2] += __float_as_int(v[j].z),
            si[3] += __float_as_int(v[j].w);
        td[0] += (double)w[j].x, td[1] += (double)w[j].y, td[2] += (double)w[j].z, td[3] += (double)w[j].w;
        ti[0] += __float_as_int(w[j].x), ti[1] += __float_as_int(w[j].y), ti[2] += __float_as_int(w[j].z),
            ti[3] += __float_as_int(w[j].w);
      }
    }
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const int slot = 4 * q + e;
      if (slot < kSlotNTerms)
        sh.psum[g][slot] = sd[e], sh2.psum[g][slot] = td[e];
      else
        sh.pisum[g][slot - kSlotNTerms] = si[e], sh2.pisum[g][slot - kSlotNTerms] = ti[e];
    }
  }
}

// wave 0, after a workgroup barrier: the 19 group sums are added in group order by the slot's lane
__device__ __forceinline__ void reduce_partials_final(int lane, RedBuf &sh) {
  if (lane < kSlotNTerms) {
    double s = sh.psum[0][lane];
#pragma unroll
    for (int g = 1; g < 19; g++) s += sh.psum[g][lane];
    sh.sums[lane] = s;
  } else if (lane < kNumSlots) {
    long long s = 0;
#pragma unroll
    for (int g = 0; g < 19; g++) s += sh.pisum[g][lane - kSlotNTerms];
    sh.isums[lane - kSlotNTerms] = s;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); // LDS writes above are read by other lanes below
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}


// One step of the LM state machine by wave 0 (all 64 lanes; lane 0 writes the state).
// sp != nullptr: the launch also evaluated the speculative candidates (where S.spec_valid) -- their reduced sums are in
// sp->red -- and new proposals may stage one; wave 1 of the workgroup runs lm_spec_wave1 beside this function.
// hp: wave 0's helper is running beside it (lm_help_wave on sh.help): it is told what to do, or that there is nothing, exactly once.
// early: called (whole wave) as soon as the step knows that it proposes -- i.e. that the next evaluation is one of THIS level -- and
// whether a speculative twin may be staged: before the solve and everything after it (the tick engine asks for its place in the item
// list then, a returning atomic whose round trip used to follow the step).
struct LmNoEarly {
  __device__ __forceinline__ void operator()(const LMState &, int, bool) const {}
};
template <class EARLY = LmNoEarly>
__device__ __forceinline__ void lm_step_wave0(int mode, int lvl, const TrackerDev &T, LMState &S, LmShared &sh, int lane,
                                              LmSpecShared *sp = nullptr, bool helped = false, EARLY *early = nullptr) {
  const bool pose_like = mode != 1;
  const double *sums = sh.red.sums;
  const long long *isums = sh.red.isums;
  double rs[6];
  build_rs(sums, isums, S.in.max_energy, rs);
  const int n_warped = (int)isums[2];
  const int n4 = (n_warped + 3) & ~3; // :824-835 padding counts in n (quirk Q3)
  const int r = lane >> 3, c = lane & 7;
  // ---- LM_OP_STEP: every lane of wave 0 evaluates the same (uniform) decisions; lane 0 writes ----
  const int max_it = level_max_it(T.p, lvl);
  const bool fixed = T.p.fixed_schedule > 0; // benchmark schedule: every step is taken, nothing ends a level but the bound
  const float lim = T.p.lambda_extrapolation_limit;
  const int phase = S.phase;
  const bool had_spec = sp && S.spec_valid; // wave-uniform; read before lane 0 clears it
  bool level_done = false, do_propose = false;
  float lambda_next = 0.01f; // computed by every lane: nothing lane 0 writes below is re-read by the wave
  int iteration = 0;
  if (lane == 0) {
    S.rounds[lvl]++;
    S.ticks++; // (a chain of the tick engine takes its extra rounds off again)
    S.spec_valid = 0;
  }
  if (phase == PH_INIT) {
    if (!fixed && rs[5] > 0.6 && S.level_cutoff_repeat < 50) { // :477-485 / :875-883
      if (lane == 0) {
        S.evals[lvl]++;
        S.level_cutoff_repeat *= 2;
        const float cutoff = T.p.coarse_cutoff_th * S.level_cutoff_repeat;
        make_eval_cutoff(T, S.in, cutoff, false, true); // (the same pose or scale once more, with the wider cut-off: nothing else changes)
      }
    } else {
      if (pose_like) {
        S.H[lane] = build_H_elem(T.p, sums, n4, r, c); // :487
        if (c == 0) S.b[r] = build_b_elem(T.p, sums, n4, r);
      }
      if (lane == 0) {
        S.evals[lvl]++;
        for (int i = 0; i < 6; i++) S.res_old[i] = rs[i];
        if (!pose_like) {
          S.Hs = (float)sums[0] * (1.0f / n4); // :885
          S.bs = (float)sums[1] * (1.0f / n4);
        }
        S.lambda = lambda_next; // 0.01, :489
        S.iteration = 0;
      }
      if (max_it <= 0)
        level_done = true;
      else
        do_propose = true;
    }
  } else {
    const double old_ratio = S.res_old[0] / S.res_old[1];
    const bool accept = fixed || (rs[0] / rs[1]) < old_ratio; // :559 / :915
    const bool small = !fixed && (pose_like ? !(S.inc_norm > 1e-3) : !(S.inc_f > 1e-3)); // :588 / :937 (signed, Q7)
    iteration = S.iteration + 1;
    {
      const float l_old = S.lambda;
      float l4 = l_old * 4;
      if (l4 < lim) l4 = lim;
      lambda_next = accept ? l_old * 0.5f : l4; // :581 / :583-585
    }
    if (pose_like && accept) { // :576-577
      S.H[lane] = build_H_elem(T.p, sums, n4, r, c);
      if (c == 0) S.b[r] = build_b_elem(T.p, sums, n4, r);
    }
    if (lane == 0) {
      S.evals[lvl]++;
      S.evals_ro[lvl] += S.in.residual_only;
      if (accept) { // :576-581 / :926-930
        for (int i = 0; i < 6; i++) S.res_old[i] = rs[i];
        if (pose_like) {
          for (int i = 0; i < 7; i++) S.cur[i] = S.cand[i];
          S.aff_cur[0] = S.aff_cand[0];
          S.aff_cur[1] = S.aff_cand[1];
        } else {
          S.Hs = (float)sums[0] * (1.0f / n4);
          S.bs = (float)sums[1] * (1.0f / n4);
          S.scale_cur = S.scale_cand;
        }
      }
    }
    if (small || iteration >= max_it) {
      level_done = true;
    } else if (!accept && had_spec) {
      // The proposal the loop makes next -- same H, b and current pose, lambda = lambda_next -- is the speculative candidate:
      // it was evaluated in this launch.  Consume it as the loop's next iteration (:505-590 once more).
      const double *sums2 = sp->red.sums;
      const long long *isums2 = sp->red.isums;
      double rs2[6];
      build_rs(sums2, isums2, S.spec_in.max_energy, rs2);
      const int n4b = ((int)isums2[2] + 3) & ~3;
      const bool accept2 = (rs2[0] / rs2[1]) < old_ratio; // res_old is unchanged by the rejection
      const bool small2 = pose_like ? !(S.spec_inc_norm > 1e-3) : !(S.spec_inc_f > 1e-3);
      iteration += 1;
      {
        const float l_old = lambda_next;
        float l4 = l_old * 4;
        if (l4 < lim) l4 = lim;
        lambda_next = accept2 ? l_old * 0.5f : l4;
      }
      if (pose_like && accept2) {
        S.H[lane] = build_H_elem(T.p, sums2, n4b, r, c);
        if (c == 0) S.b[r] = build_b_elem(T.p, sums2, n4b, r);
      }
      if (lane == 0) {
        S.evals[lvl]++;
        S.evals_ro[lvl] += S.spec_in.residual_only;
        if (accept2) {
          for (int i = 0; i < 6; i++) S.res_old[i] = rs2[i];
          if (pose_like) {
            for (int i = 0; i < 7; i++) S.cur[i] = S.spec_cand[i];
            S.aff_cur[0] = S.spec_aff_cand[0];
            S.aff_cur[1] = S.spec_aff_cand[1];
          } else {
            S.Hs = (float)sums2[0] * (1.0f / n4b);
            S.bs = (float)sums2[1] * (1.0f / n4b);
            S.scale_cur = S.spec_scale_cand;
          }
        }
      }
      if (small2 || iteration >= max_it)
        level_done = true;
      else
        do_propose = true;
    } else {
      do_propose = true;
    }
    if (lane == 0) {
      S.lambda = lambda_next;
      S.iteration = iteration;
    }
  }
  // make lane 0's state writes (lambda, cur, ...) visible to the whole wave (and to wave 1) before proposing
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  // the speculative proposal: what the loop proposes after rejecting the main one -- lambda four times larger (:583-585);
  // it exists only if the loop would go on after that rejection (one more iteration allowed; the main step not "too small")
  const bool want_spec = sp && do_propose && !fixed && iteration + 1 < max_it;
  if (early && do_propose) (*early)(S, lane, want_spec);
  if (sp && lane == 0) {
    float l4 = lambda_next * 4;
    if (l4 < lim) l4 = lim;
    sp->lambda = l4;
    lds_flag_set(&sp->cmd, want_spec ? 1 : 2);
  }
  if (do_propose) {
    if (pose_like)
      propose_pose(T, S, lambda_next, lane, sh.ldlt, false, helped ? &sh.help : nullptr);
    else if (lane == 0)
      propose_scale(T, S, lambda_next);
  }
  if (helped && !(do_propose && pose_like) && lane == 0) lds_flag_set(&sh.help.cmd, 2);
  if (want_spec) {
    (void)lds_wait_nonzero(&sp->done);
    if (lane == 0) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      const bool main_small = pose_like ? !(S.inc_norm > 1e-3) : !(S.inc_f > 1e-3); // the loop breaks after the main step
      S.spec_valid = main_small ? 0 : 1;
    }
  }
  if (lane == 0 && level_done) end_level(T, S);
}

// wave 1 beside lm_step_wave0: stages the speculative proposal when wave 0 asks for it (helped: its own helper runs on sp.help)
__device__ __forceinline__ void lm_spec_wave1(int mode, const TrackerDev &T, LMState &S, LmSpecShared &sp, int lane, bool helped = false) {
  const int cmd = lds_wait_nonzero(&sp.cmd);
  if (cmd != 1 || mode == 1) {
    if (helped && lane == 0) lds_flag_set(&sp.help.cmd, 2);
    if (cmd != 1) return;
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  const float lambda = sp.lambda;
  if (mode != 1) {
    propose_pose(T, S, lambda, lane, sp.ldlt, true, helped ? &sp.help : nullptr);
  } else if (lane == 0) {
    propose_scale(T, S, lambda, true);
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  if (lane == 0) lds_flag_set(&sp.done, 1);
}

// One LM step by a workgroup of >= 256 threads on the problem's partials: state and tracker descriptor
// staged through LDS, fixed-order reduction, wave 0 advances the state machine and writes the state
// back.  Shared by lm_kernel (LM_OP_STEP) and by the last-arriving workgroup of a fused eval kernel.
// All threads of the workgroup must call it; S must be at this level (status RUNNING, lvl, mode).
// sp != nullptr: speculative candidates (their partials sit spec_off floats behind the main ones).
// What a caller already holds when it calls lm_step_block (round 6: the step's memory phase was three to four DEPENDENT round trips
// -- tracker pointer -> descriptor, point count of the pending evaluation -> partials, main then speculative partials -- 11 k of the
// 37 k cycles an LM workgroup of the tick engine lives, shader-clock stamps in profiles/r06_tick_stamps.json).  With the point
// count known up front the descriptor, the state block and every partial are requested together: one round trip.
struct LmPre {
  int n_lvl, ppt_lvl; // S.in.n / S.in.ppt of the pending evaluation
  bool have_sv;       // sv holds this thread's 16-byte block of the state (already loaded with the caller's own first reads)
  uint4 sv;
};
constexpr int kLmS16 = sizeof(LMState) / 16, kLmT16 = sizeof(TrackerDev) / 16;
// The first reads of a kernel that steps problem `prob` from memory (lm_kernel, tick_lm_kernel), all requested together -- ONE round
// trip: status, kind and level, the pending evaluation's point count, the tracker pointer and this thread's 16-byte block of the state.
struct LmHead {
  int status, kind, lvl;
  const TrackerDev *Tg;
  LmPre pre;
};
template <class TRACKERS>
__device__ __forceinline__ LmHead lm_read_head(const LMState &S, TRACKERS trackers, int prob, int tid) {
  LmHead h;
  h.status = S.status, h.kind = S.is_scale, h.lvl = S.lvl;
  h.pre.n_lvl = S.in.n, h.pre.ppt_lvl = S.in.ppt, h.pre.have_sv = true;
  h.Tg = trackers[prob];
  h.pre.sv = tid < kLmS16 ? ((const uint4 *)&S)[tid] : uint4{0, 0, 0, 0};
  return h;
}
template <bool COH = false, class EARLY = LmNoEarly>
__device__ __forceinline__ void lm_step_block(int mode, int lvl, int prob, const TrackerDev *Tg, LMState &S,
                                              const float *partials_prob, LmShared &sh, int tid, int *status_out,
                                              LmSpecShared *sp = nullptr, int spec_off = 0, const LmPre *pre = nullptr, EARLY *early = nullptr,
                                              bool help = true) {
  constexpr int kS16 = kLmS16, kT16 = kLmT16;
  static_assert(kS16 <= kThreads && kT16 <= kThreads, "one 16-byte block per thread");
  // one round trip: state block, tracker descriptor and the chunk partials together
  uint4 sv = {0, 0, 0, 0}, tv = {0, 0, 0, 0};
  if (pre && pre->have_sv)
    sv = pre->sv;
  else if (tid < kS16)
    sv = COH ? load16_coherent((const uint4 *)&S + tid) : ((const uint4 *)&S)[tid];
  if (tid < kT16) tv = ((const uint4 *)Tg)[tid];
  // the pending evaluation was built for this level
  const int n_lvl = pre ? pre->n_lvl : COH ? __hip_atomic_load(&S.in.n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : S.in.n;
  const int ppt_lvl = pre ? pre->ppt_lvl : COH ? __hip_atomic_load(&S.in.ppt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : S.in.ppt;
  if (sp) { // (garbage where no speculative candidate was evaluated: never looked at then)
    reduce_partials_groups2(partials_prob, partials_prob + spec_off, chunks_of(n_lvl, ppt_lvl), tid, sh.red, sp->red);
    if (tid == 0) sp->cmd = 0, sp->done = 0, sp->help.cmd = 0, sp->help.done = 0;
  } else {
    reduce_partials_groups(partials_prob, chunks_of(n_lvl, ppt_lvl), tid, sh.red);
  }
  if (tid == 0) sh.help.cmd = 0, sh.help.done = 0;
  if (tid < kS16) ((uint4 *)&sh.st)[tid] = sv;
  if (tid < kT16) ((uint4 *)&sh.trk)[tid] = tv;
  __syncthreads();
  // waves 2 and 3: the helpers of the proposing waves 0 and 1 (the pose problems' affine part, lm_help_wave)
  const bool helped = mode != 1 && help;
  if (sp && tid >= 64 && tid < 128) lm_spec_wave1(mode, sh.trk, sh.st, *sp, tid - 64, helped);
  if (helped && tid >= 128 && tid < 192) lm_help_wave(sh.trk, sh.st, sh.help, tid - 128);
  if (helped && sp && tid >= 192 && tid < 256) lm_help_wave(sh.trk, sh.st, sp->help, tid - 192);
  if (tid >= 64) return; // wave 0 carries on
  const int lane = tid;
  reduce_partials_final(lane, sh.red);
  if (sp) reduce_partials_final(lane, sp->red);
  lm_step_wave0(mode, lvl, sh.trk, sh.st, sh, lane, sp, helped, early);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); // lane 0's LDS writes -> the whole wave
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  if (COH) {
    for (int i = lane; i < kS16; i += 64) store16_coherent((uint4 *)&S + i, ((const uint4 *)&sh.st)[i]);
  } else {
    stage_out(&S, sh.st, lane, 64);
  }
  if (lane == 0 && status_out) {
    status_out[2 * prob] = sh.st.status;
    status_out[2 * prob + 1] = sh.st.lvl;
  }
}

} // namespace dsm
