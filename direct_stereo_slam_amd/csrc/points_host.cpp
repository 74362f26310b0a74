// points_host.cpp -- the three point calls of the front end as the reference runs them, one sequential loop each, and the rules for
// their jobs: activation (dsm_activate_points_host), optimisation of immature points
// (dsm_optimize_immature_points_host, section 13), tracing (dsm_trace_points_host, section 14) and, before them all, the selection of
// the pixels that become points (dsm_select_pixels_host, section 15); and the linearisation of the window optimisation's active
// residuals (dsm_linearize_residuals_host, section 16) with the accumulation of the Hessian and Schur terms over them
// (dsm_window_hessian_host, section 17).  The host forms are what the CPU suite checks against the numpy
// checkers and what the device forms (distmap_kernels.hip, immature_kernels.hip, trace_kernels.hip, select_kernels.hip,
// linearize_kernels.hip, hessian_kernels.hip) must equal bit for bit: the arithmetic is shared through point_math.hpp, immature_math.hpp,
// trace_math.hpp, select_math.hpp, linearize_math.hpp and hessian_math.hpp, the job rules through the *_error functions below.  Plain C++; no device code.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "dsm_internal.hpp"
#include "immature_math.hpp"
#include "hessian_math.hpp"
#include "linearize_math.hpp"
#include "select_math.hpp"
#include "trace_math.hpp"

// ---------------------------------------------------------------------------------------------
// What both forms of a call refuse in its settings and in the arrays of one job; NULL when the rules hold.  A form adds only what is
// its own: the device form its handles, the one geometry per call and the size caps, the host form w, h and the planes.
// ---------------------------------------------------------------------------------------------
namespace dsm {
const char *activation_job_error(const dsm_activation_job &J, bool with_cand) {
  const int nc = with_cand ? J.n_cand : 0;
  if (J.n_hosts < 0 || J.n_seeds < 0 || nc < 0 || (J.n_hosts && (!J.krki || !J.kt)) ||
      (J.n_seeds && (!J.seed_host || !J.seed_u || !J.seed_v || !J.seed_idepth)) ||
      (nc && (!J.cand_host || !J.cand_u || !J.cand_v || !J.cand_idepth || !J.cand_type || !J.decision_out)))
    return "negative count or NULL array";
  for (int i = 0; i < J.n_seeds; i++)
    if (J.seed_host[i] < 0 || J.seed_host[i] >= J.n_hosts) return "seed_host outside [0, n_hosts)";
  for (int i = 0; i < nc; i++)
    if (J.cand_host[i] < 0 || J.cand_host[i] >= J.n_hosts) return "cand_host outside [0, n_hosts)";
  return nullptr;
}

const char *immature_settings_error(float huber_th, float min_idepth_h_act, int gn_iterations) {
  if (gn_iterations < 0 || gn_iterations > DSM_IMMATURE_GN_ITERATIONS_LIMIT || !std::isfinite(huber_th) || !std::isfinite(min_idepth_h_act))
    return "gn_iterations outside [0, 16], or a non-finite threshold";
  return nullptr;
}
const char *immature_job_error(const dsm_immature_job &J) {
  if (J.n_frames < 1 || J.n_frames > DSM_IMMATURE_MAX_FRAMES || J.n_pts < 0 || !J.frame_ids || !J.pre_R || !J.pre_t || !J.pre_aff)
    return "n_frames outside [1, 9], a negative count or a NULL array";
  if (J.n_pts && (!J.host || !J.u || !J.v || !J.idepth_min || !J.idepth_max || !J.energy_th || !J.color || !J.weights || !J.status ||
                  !J.idepth_out || !J.res_state))
    return "NULL array";
  for (int i = 0; i < J.n_pts; i++)
    if (J.host[i] < 0 || J.host[i] >= J.n_frames) return "host outside [0, n_frames)";
  return nullptr;
}

const char *trace_params_error(const dsm_trace_params *p) {
  if (!p) return "no parameters";
  if (p->gn_iterations < 0 || p->gn_iterations > 16) return "gn_iterations outside [0, 16]";
  if (!std::isfinite(p->stepsize) || !(p->stepsize > 0)) return "a non-finite or non-positive stepsize";
  if (!std::isfinite(p->max_pix_search) || !std::isfinite(p->slack_interval) || !std::isfinite(p->min_improvement) ||
      !std::isfinite(p->gn_threshold) || !std::isfinite(p->extra_slack_on_th) || !std::isfinite(p->huber_th))
    return "a non-finite parameter";
  if (p->min_test_radius < 0) return "a negative min_test_radius";
  return nullptr;
}
const char *trace_job_error(const dsm_trace_job &J) {
  if (J.n_hosts < 0 || J.n_hosts > DSM_TRACE_MAX_HOSTS || J.n_pts < 0) return "n_hosts outside [0, 16] or a negative count";
  if (J.n_hosts && (!J.krki || !J.kt || !J.aff)) return "NULL host array";
  if (J.n_pts && (!J.host || !J.u || !J.v || !J.energy_th || !J.grad_h || !J.color || !J.weights || !J.status || !J.idepth_min ||
                  !J.idepth_max || !J.quality || !J.trace_uv || !J.trace_interval))
    return "NULL point array";
  for (int i = 0; i < J.n_pts; i++) {
    if (J.host[i] < 0 || J.host[i] >= J.n_hosts) return "host outside [0, n_hosts)";
    if (J.status[i] > DSM_IPS_UNINITIALIZED) return "a status byte above 5";
  }
  return nullptr;
}

const char *select_params_error(const dsm_select_params *p) {
  if (!p) return "no parameters";
  if (p->recursions < 0 || p->recursions > 4) return "recursions outside [0, 4]";
  if (p->pattern_padding < 2 || p->pattern_padding > 8) return "pattern_padding outside [2, 8]";
  if (!std::isfinite(p->min_grad_hist_cut) || !std::isfinite(p->min_grad_hist_add) || !std::isfinite(p->grad_downweight_per_level) ||
      !std::isfinite(p->th_factor) || !std::isfinite(p->outlier_th) || !std::isfinite(p->outlier_th_sum_component) ||
      !std::isfinite(p->overall_energy_th_weight))
    return "a non-finite parameter";
  return nullptr;
}
const char *select_geometry_error(int w, int h) {
  if (w < 32 || h < 32) return "the frame is smaller than 32 x 32";
  if ((long long)w * h > (1ll << 26)) return "the frame is larger than 2^26 pixels";
  return nullptr;
}
const char *select_job_error(const dsm_select_job &J) {
  if (!J.potential_io || !J.n_pts_out || !J.num_total_out) return "NULL potential_io, n_pts_out or num_total_out";
  if (*J.potential_io < 1 || *J.potential_io > DSM_SELECT_MAX_POTENTIAL) return "a potential outside [1, 4096]";
  if (!std::isfinite(J.density) || !(J.density > 0)) return "a density that is not finite or not positive";
  if (J.max_pts < 0) return "a negative max_pts";
  if (J.max_pts && (!J.u || !J.v || !J.energy_th || !J.grad_h || !J.color || !J.weights || !J.status || !J.idepth_min || !J.idepth_max ||
                    !J.quality || !J.type))
    return "NULL point array";
  return nullptr;
}

const char *linearize_params_error(const dsm_linearize_params *p) {
  if (!p) return "no parameters";
  if (!std::isfinite(p->huber_th) || !std::isfinite(p->outlier_th_sum_component) || !std::isfinite(p->scale_idepth) ||
      !std::isfinite(p->scale_f) || !std::isfinite(p->scale_c) || !std::isfinite(p->thn) || !std::isfinite(p->fac_median) ||
      !std::isfinite(p->cw) || !std::isfinite(p->ow))
    return "a non-finite parameter";
  if (!(p->thn >= 0.0f && p->thn < 1.0f)) return "thn outside [0, 1)";
  return nullptr;
}
const char *linearize_job_error(const dsm_linearize_job &J) {
  if (J.n_frames < 1 || J.n_frames > DSM_WINDOW_MAX_FRAMES || J.n_pts < 0 || J.n_res < 0 || !J.frame_ids || !J.pre_RTll_0 || !J.pre_tTll_0 ||
      !J.pre_KRKiTll || !J.pre_KtTll || !J.pre_aff_mode || !J.pre_b0_mode || !J.frame_energy_th || !J.energy_out || !J.new_frame_energy_th_out)
    return "n_frames outside [1, 16], a negative count or a NULL array";
  if (J.n_pts && (!J.host || !J.u || !J.v || !J.idepth_scaled || !J.idepth_zero_scaled || !J.color || !J.weights)) return "NULL point array";
  if (J.n_res && (!J.point || !J.target || !J.state_in || !J.energy_in || !J.new_state || !J.new_energy || !J.new_energy_with_outlier ||
                  (J.fix_linearization && !J.is_new)))
    return "NULL residual array";
  for (int i = 0; i < J.n_pts; i++)
    if (J.host[i] < 0 || J.host[i] >= J.n_frames) return "host outside [0, n_frames)";
  for (int r = 0; r < J.n_res; r++) {
    if (J.point[r] < 0 || J.point[r] >= J.n_pts) return "point outside [0, n_pts)";
    if (J.target[r] < 0 || J.target[r] >= J.n_frames) return "target outside [0, n_frames)";
    if (J.target[r] == J.host[J.point[r]]) return "a residual whose target is its point's host";
    if (J.state_in[r] != DSM_RES_IN && J.state_in[r] != DSM_RES_OOB && J.state_in[r] != DSM_RES_OUTLIER) return "a state_in that is no residual state";
  }
  return nullptr;
}

// B1: the double sum of the returned values in residual order.  B2: setNewFrameEnergyTH (:79-120) on the residuals against the newest frame.
void linearize_job_summary(const dsm_linearize_job &J, const dsm_linearize_params &S) {
  double energy = 0;
  std::vector<float> all;
  for (int r = 0; r < J.n_res; r++) {
    energy += J.new_energy[r];
    if (J.target[r] == J.n_frames - 1 && J.new_energy_with_outlier[r] >= 0) all.push_back(J.new_energy_with_outlier[r]);
  }
  *J.energy_out = energy;
  float th = DSM_LINEARIZE_EMPTY_FRAME_ENERGY_TH;
  if (!all.empty()) {
    const int nth = (int)(S.thn * (float)all.size()); // a float32 product, below the count for every thn < 1
    std::nth_element(all.begin(), all.begin() + nth, all.end());
    th = sqrtf(all[nth]) * S.fac_median;
    th = 26.0f * S.cw + th * (1 - S.cw);
    th = th * th;
    th *= S.ow * S.ow;
  }
  *J.new_frame_energy_th_out = th;
}

// V of DESIGN.md section 17, after linearize_job_error has passed
const char *hessian_job_error(const dsm_hessian_job &J, bool stitched_required) {
  const dsm_linearize_job &L = J.lin;
  if (!J.ad_host || !J.ad_target) return "NULL ad_host or ad_target";
  if (stitched_required && (!J.H_A || !J.b_A || !J.H_sc || !J.b_sc)) return "NULL H_A, b_A, H_sc or b_sc";
  const size_t n_ad = (size_t)L.n_frames * L.n_frames * 64;
  for (size_t i = 0; i < n_ad; i++)
    if (!std::isfinite(J.ad_host[i]) || !std::isfinite(J.ad_target[i])) return "a non-finite ad_host or ad_target";
  const float *per_point[] = {J.prior, J.delta, J.hdd_lin, J.bd_lin};
  for (const float *a : per_point)
    for (int i = 0; a && i < L.n_pts; i++)
      if (!std::isfinite(a[i])) return "a non-finite prior, delta, hdd_lin or bd_lin";
  for (int i = 0; J.hcd_lin && i < 4 * L.n_pts; i++)
    if (!std::isfinite(J.hcd_lin[i])) return "a non-finite hcd_lin";
  std::vector<unsigned> seen((size_t)L.n_pts, 0u); // n_frames <= 16: one bit per target
  for (int r = 0; r < L.n_res; r++) {
    const unsigned bit = 1u << L.target[r];
    if (seen[L.point[r]] & bit) return "a point with two residuals against one target";
    seen[L.point[r]] |= bit;
  }
  return nullptr;
}

namespace {
// C (M x N) = A (M x K) * B (K x N): every entry the double sum over ascending k, from 0.0.  The k loop is the outer one of a row, so
// that the compiler may work on the N entries of the row at once; each entry's own order is unchanged.
template <int M, int K, int N>
inline void small_mul(const double *A, int lda, const double *B, int ldb, double *C) {
  for (int i = 0; i < M; i++) {
    double s[N];
    for (int j = 0; j < N; j++) s[j] = 0.0;
    for (int q = 0; q < K; q++) {
      const double a = A[i * lda + q];
      for (int j = 0; j < N; j++) s[j] += a * B[q * ldb + j];
    }
    for (int j = 0; j < N; j++) C[i * N + j] = s[j];
  }
}
void add_block(double *H, int N, int r0, int c0, const double *C, int m, int n, bool transposed = false) {
  for (int i = 0; i < m; i++)
    for (int j = 0; j < n; j++) H[(size_t)(r0 + i) * N + c0 + j] += transposed ? C[j * m + i] : C[i * n + j];
}
void mirror_upper(double *H, int N) {
  for (int i = 0; i < N; i++)
    for (int j = i + 1; j < N; j++) H[(size_t)j * N + i] = H[(size_t)i * N + j];
}
} // namespace

void hessian_stitch(const dsm_hessian_job &J, const double *top, const double *D, const double *E, const double *EB, const double *Hcc,
                    const double *bc) {
  const int nf = J.lin.n_frames, N = 4 + 8 * nf;
  double *HA = J.H_A, *bA = J.b_A, *HS = J.H_sc, *bS = J.b_sc;
  std::fill(HA, HA + (size_t)N * N, 0.0), std::fill(HS, HS + (size_t)N * N, 0.0);
  std::fill(bA, bA + N, 0.0), std::fill(bS, bS + N, 0.0);
  double C[64], Mh[64], Mt[64];
  // the transposes of every ad_host / ad_target block, once: the products below then read both factors row by row
  const size_t n_blocks = (size_t)nf * nf;
  std::vector<double> adT(2 * n_blocks * 64);
  for (size_t p = 0; p < n_blocks; p++)
    for (int i = 0; i < 8; i++)
      for (int j = 0; j < 8; j++)
        adT[p * 64 + 8 * j + i] = J.ad_host[p * 64 + 8 * i + j], adT[(n_blocks + p) * 64 + 8 * j + i] = J.ad_target[p * 64 + 8 * i + j];
  const double *hostT = adT.data(), *targetT = adT.data() + n_blocks * 64;
  for (int h = 0; h < nf; h++) // H_A, b_A: pairs in (h, t) order; a frame is no target of its own points
    for (int t = 0; t < nf; t++) {
      if (t == h) continue;
      const double *A = top + (size_t)(h * nf + t) * 169, *Ah = J.ad_host + (size_t)(h * nf + t) * 64, *At = J.ad_target + (size_t)(h * nf + t) * 64;
      const double *AhT = hostT + (size_t)(h * nf + t) * 64, *AtT = targetT + (size_t)(h * nf + t) * 64;
      const int ih = 4 + 8 * h, it = 4 + 8 * t;
      for (int a = 0; a < 4; a++) {
        for (int b = 0; b < 4; b++) HA[(size_t)a * N + b] += A[a * 13 + b];
        bA[a] += A[a * 13 + 12];
      }
      small_mul<4, 8, 8>(A + 4, 13, AhT, 8, C), add_block(HA, N, 0, ih, C, 4, 8);
      small_mul<4, 8, 8>(A + 4, 13, AtT, 8, C), add_block(HA, N, 0, it, C, 4, 8);
      small_mul<8, 8, 8>(Ah, 8, A + 4 * 13 + 4, 13, Mh), small_mul<8, 8, 8>(At, 8, A + 4 * 13 + 4, 13, Mt);
      small_mul<8, 8, 8>(Mh, 8, AhT, 8, C), add_block(HA, N, ih, ih, C, 8, 8);
      small_mul<8, 8, 8>(Mh, 8, AtT, 8, C), add_block(HA, N, ih, it, C, 8, 8);
      small_mul<8, 8, 8>(Mt, 8, AhT, 8, C), add_block(HA, N, it, ih, C, 8, 8);
      small_mul<8, 8, 8>(Mt, 8, AtT, 8, C), add_block(HA, N, it, it, C, 8, 8);
      small_mul<8, 8, 1>(Ah, 8, A + 4 * 13 + 12, 13, C), add_block(bA, 1, ih, 0, C, 8, 1);
      small_mul<8, 8, 1>(At, 8, A + 4 * 13 + 12, 13, C), add_block(bA, 1, it, 0, C, 8, 1);
    }
  mirror_upper(HA, N);
  for (int c = 0; c < 4; c++) { // H_sc, b_sc
    for (int d = 0; d < 4; d++) HS[(size_t)c * N + d] = Hcc[4 * c + d];
    bS[c] = bc[c];
  }
  for (int h = 0; h < nf; h++)
    for (int t1 = 0; t1 < nf; t1++) {
      if (t1 == h) continue;
      const size_t p1 = (size_t)(h * nf + t1);
      const double *Ah1 = J.ad_host + p1 * 64, *At1 = J.ad_target + p1 * 64;
      const int ih = 4 + 8 * h, i1 = 4 + 8 * t1;
      small_mul<8, 8, 4>(Ah1, 8, E + p1 * 32, 4, C), add_block(HS, N, 0, ih, C, 4, 8, true);
      small_mul<8, 8, 4>(At1, 8, E + p1 * 32, 4, C), add_block(HS, N, 0, i1, C, 4, 8, true);
      small_mul<8, 8, 1>(Ah1, 8, EB + p1 * 8, 1, C), add_block(bS, 1, ih, 0, C, 8, 1);
      small_mul<8, 8, 1>(At1, 8, EB + p1 * 8, 1, C), add_block(bS, 1, i1, 0, C, 8, 1);
      for (int t2 = 0; t2 < nf; t2++) {
        if (t2 == h) continue;
        const size_t p2 = (size_t)(h * nf + t2);
        const double *Ah2T = hostT + p2 * 64, *At2T = targetT + p2 * 64, *Dk = D + (p1 * nf + t2) * 64;
        const int i2 = 4 + 8 * t2;
        small_mul<8, 8, 8>(Ah1, 8, Dk, 8, Mh), small_mul<8, 8, 8>(At1, 8, Dk, 8, Mt);
        small_mul<8, 8, 8>(Mh, 8, Ah2T, 8, C), add_block(HS, N, ih, ih, C, 8, 8);
        small_mul<8, 8, 8>(Mh, 8, At2T, 8, C), add_block(HS, N, ih, i2, C, 8, 8);
        small_mul<8, 8, 8>(Mt, 8, Ah2T, 8, C), add_block(HS, N, i1, ih, C, 8, 8);
        small_mul<8, 8, 8>(Mt, 8, At2T, 8, C), add_block(HS, N, i1, i2, C, 8, 8);
      }
    }
  mirror_upper(HS, N);
  hessian_copy_raw(J, top, D, E, EB, Hcc, bc);
}

void hessian_copy_raw(const dsm_hessian_job &J, const double *top, const double *D, const double *E, const double *EB, const double *Hcc,
                      const double *bc) {
  const size_t nf = J.lin.n_frames, n2 = nf * nf;
  if (J.acc_top) memcpy(J.acc_top, top, 8 * n2 * 169);
  if (J.acc_D) memcpy(J.acc_D, D, 8 * n2 * nf * 64);
  if (J.acc_E) memcpy(J.acc_E, E, 8 * n2 * 32);
  if (J.acc_EB) memcpy(J.acc_EB, EB, 8 * n2 * 8);
  if (J.acc_Hcc) memcpy(J.acc_Hcc, Hcc, 8 * 16);
  if (J.acc_bc) memcpy(J.acc_bc, bc, 8 * 4);
}
} // namespace dsm

namespace {
int refuse(const char *call, const char *msg) {
  dsm::set_error(std::string(call) + ": " + msg);
  return DSM_ERR_INVALID;
}
} // namespace

// ---------------------------------------------------------------------------------------------
// CoarseDistanceMap + the activation walk of FrontEnd::activatePointsMT as the reference runs them: one sequential loop, the list
// BFS of growDistBFS (TrackerAndScaler.cpp:1235-1324) on a float map.  D1-D6: DESIGN.md section 12.
// ---------------------------------------------------------------------------------------------
namespace {
struct HostDistMap {
  int w1, h1;
  std::vector<float> map;
  std::vector<int> l1, l2; // bfs_list1_ / bfs_list2_ as cell indices
  // growDistBFS (:1235-1324): the list in l1 holds bfs_num cells
  void grow(int bfs_num) {
    static const int DX[8] = {1, -1, 0, 0, 1, -1, -1, 1}, DY[8] = {0, 0, 1, -1, 1, 1, -1, -1};
    for (int k = 1; k < 40 && bfs_num > 0; k++) { // (an empty list stays empty: the remaining levels do nothing)
      const int bfs_num2 = bfs_num;
      std::swap(l1, l2);
      bfs_num = 0;
      const int nd = (k % 2 == 0) ? 4 : 8;
      for (int i = 0; i < bfs_num2; i++) {
        const int x = l2[i] % w1, y = l2[i] / w1;
        if (x == 0 || y == 0 || x == w1 - 1 || y == h1 - 1) continue;
        for (int d = 0; d < nd; d++) {
          const int idx = (x + DX[d]) + (y + DY[d]) * w1;
          if (map[idx] > k) {
            map[idx] = (float)k;
            if ((size_t)bfs_num == l1.size()) l1.push_back(idx); else l1[bfs_num] = idx;
            bfs_num++;
          }
        }
      }
    }
  }
  void push_first(int idx, int at) {
    if ((size_t)at == l1.size()) l1.push_back(idx); else l1[at] = idx;
  }
};

// ptp = KRKi (u, v, 1) + Kt idepth (:1218, FrontEnd.cpp:432-433), then the bounds test; returns the cell or -1
inline int project_l1(const float *M, const float *T, float u, float v, float id, int w1, int h1, float *p0_out) {
  const dsm::pt::Vec3 p = dsm::pt::add_translation(dsm::pt::rotate_uv1(M, u, v), T, id);
  const float qu = p.x / p.z + 0.5f, qv = p.y / p.z + 0.5f;
  *p0_out = p.x;
  if (!(qu >= 1.0f && qv >= 1.0f && qu < (float)w1 && qv < (float)h1)) return -1;
  return (int)qu + w1 * (int)qv;
}
} // namespace

extern "C" int dsm_activate_points_host(int w, int h, const dsm_activation_job *job, float *map_out) {
  auto fail = [](const char *msg) { return refuse("dsm_activate_points_host", msg); };
  if (w < 2 || h < 2 || !job) return fail("bad argument");
  if (const char *e = dsm::activation_job_error(*job, true)) return fail(e);
  const dsm_activation_job &J = *job;
  HostDistMap D;
  D.w1 = w >> 1, D.h1 = h >> 1;
  D.map.assign((size_t)D.w1 * D.h1, 1000.0f); // :1202-1203
  int num_items = 0;
  float p0;
  for (int i = 0; i < J.n_seeds; i++) { // :1216-1226
    const int hst = J.seed_host[i];
    const int c = project_l1(J.krki + 9 * hst, J.kt + 3 * hst, J.seed_u[i], J.seed_v[i], J.seed_idepth[i], D.w1, D.h1, &p0);
    if (c < 0) continue;
    D.map[c] = 0;
    D.push_first(c, num_items++);
  }
  D.grow(num_items);
  int n_act = 0;
  for (int i = 0; i < J.n_cand; i++) { // FrontEnd.cpp:431-449
    const int hst = J.cand_host[i];
    const int c = project_l1(J.krki + 9 * hst, J.kt + 3 * hst, J.cand_u[i], J.cand_v[i], J.cand_idepth[i], D.w1, D.h1, &p0);
    if (c < 0) {
      J.decision_out[i] = 2;
      continue;
    }
    const float dist = D.map[c] + (p0 - floorf(p0));
    if (dist >= J.min_act_dist * J.cand_type[i]) {
      D.map[c] = 0; // addIntoDistFinal (:1326-1332)
      D.push_first(c, 0);
      D.grow(1);
      J.decision_out[i] = 1;
      n_act++;
    } else {
      J.decision_out[i] = 0;
    }
  }
  if (J.n_activated_out) *J.n_activated_out = n_act;
  if (map_out) memcpy(map_out, D.map.data(), sizeof(float) * D.map.size());
  return DSM_OK;
}

// ---------------------------------------------------------------------------------------------
// FrontEnd::optimizeImmaturePoint (dso_helpers/FrontEndOptPoint.cpp:35-138) as the reference runs it: one sequential loop over the
// points of a window, ImmaturePoint::linearizeResidual per residual with the accumulators passed by reference.  M1-M8, U1-U9:
// DESIGN.md section 13.  The pattern pixel (imm::tap) and the rules between the passes (imm::LM) are immature_math.hpp, shared with the
// device kernel.
// ---------------------------------------------------------------------------------------------
namespace {
struct ImmTmpRes { // ImmaturePointTemporaryResidual
  int state_state, state_NewState;
  float state_energy, state_NewEnergy;
  int target;
  void commit() { state_state = state_NewState, state_energy = state_NewEnergy; }
};

struct ImmPoint {
  const dsm_immature_job *J;
  dsm::imm::Cam C;
  const float *const *frame_I;
  int i; // the point
  float huber;
  // ImmaturePoint::linearizeResidual (UPSTREAM-DSO), U1-U9
  float linearize(float slack, ImmTmpRes &res, float &Hdd, float &bd, float idepth) const {
    using namespace dsm::imm;
    if (res.state_state == RES_OOB) { // U1
      res.state_NewState = RES_OOB;
      return res.state_energy;
    }
    const int nf = J->n_frames, pair = J->host[i] * nf + res.target;
    float energyLeft = 0;
    for (int idx = 0; idx < 8; idx++) {
      int dx, dy;
      dsm::pt::pattern(idx, dx, dy);
      float tE, tH, tb;
      if (!tap(C, frame_I[res.target], J->pre_R + 9 * pair, J->pre_t + 3 * pair, J->pre_aff + 2 * pair, J->u[i], J->v[i], dx, dy, idepth,
               J->color[8 * i + idx], J->weights[8 * i + idx], huber, tE, tH, tb)) { // U4 / U6: the earlier pixels' terms stay in Hdd / bd
        res.state_NewState = RES_OOB;
        return res.state_energy;
      }
      energyLeft += tE;
      Hdd += tH;
      bd += tb;
    }
    const float lim = J->energy_th[i] * slack; // U9
    if (energyLeft > lim) {
      energyLeft = lim;
      res.state_NewState = RES_OUTLIER;
    } else {
      res.state_NewState = RES_IN;
    }
    res.state_NewEnergy = energyLeft;
    return energyLeft;
  }
};
} // namespace

extern "C" int dsm_optimize_immature_points_host(int w, int h, const dsm_immature_job *job, const float *const *frame_I, float huber_th,
                                                 float min_idepth_h_act, int gn_iterations) {
  using namespace dsm::imm;
  auto fail = [](const char *msg) { return refuse("dsm_optimize_immature_points_host", msg); };
  if (w < 8 || h < 8 || !job || !frame_I) return fail("bad argument");
  if (const char *e = dsm::immature_settings_error(huber_th, min_idepth_h_act, gn_iterations)) return fail(e);
  if (const char *e = dsm::immature_job_error(*job)) return fail(e);
  const dsm_immature_job &J = *job;
  for (int f = 0; f < J.n_frames; f++)
    if (!frame_I[f]) return fail("NULL frame");
  ImmPoint P;
  P.J = job, P.frame_I = frame_I, P.huber = huber_th;
  P.C = Cam{J.cam[0], J.cam[1], J.cam[2], J.cam[3], J.cam_inv[0], J.cam_inv[1], w, h};
  const int nf = J.n_frames;
  for (int i = 0; i < J.n_pts; i++) {
    P.i = i;
    ImmTmpRes residuals[DSM_IMMATURE_MAX_FRAMES];
    int nres = 0;
    for (int f = 0; f < nf; f++) // :38-46
      if (f != J.host[i]) residuals[nres++] = ImmTmpRes{RES_IN, RES_OUTLIER, 0.f, 0.f, f};
    const float start = lm_start(J.idepth_min[i], J.idepth_max[i]); // M1
    float energy = 0, Hdd = 0, bd = 0;
    for (int k = 0; k < nres; k++) { // M2
      energy += P.linearize(1000, residuals[k], Hdd, bd, start);
      residuals[k].commit();
    }
    LM s = lm_begin(start, energy, Hdd, bd, min_idepth_h_act);
    while (!s.done && s.iterations < gn_iterations) {
      const float newIdepth = lm_propose(s); // M3
      float newHdd = 0, newbd = 0, newEnergy = 0;
      for (int k = 0; k < nres; k++) newEnergy += P.linearize(1, residuals[k], newHdd, newbd, newIdepth);
      if (lm_trial(s, newEnergy, newHdd, newbd, min_idepth_h_act)) // M4, M5
        for (int k = 0; k < nres; k++) residuals[k].commit();
    }
    int numGoodRes = 0;
    for (int k = 0; k < nres; k++) numGoodRes += residuals[k].state_state == RES_IN;
    lm_finish(s, numGoodRes, J.min_obs); // :121-138
    J.status[i] = (unsigned char)s.status;
    J.idepth_out[i] = s.idepth;
    J.res_state[(size_t)i * nf + J.host[i]] = DSM_RES_HOST;
    for (int k = 0; k < nres; k++) J.res_state[(size_t)i * nf + residuals[k].target] = (unsigned char)residuals[k].state_state;
    if (J.hdd_out) J.hdd_out[i] = s.Hdd;
    if (J.bd_out) J.bd_out[i] = s.bd;
    if (J.energy_out) J.energy_out[i] = s.energy;
    if (J.iterations_out) J.iterations_out[i] = s.iterations;
  }
  return DSM_OK;
}

// ---------------------------------------------------------------------------------------------
// The loop of FrontEnd::traceNewCoarse (FrontEnd.cpp:276-327) as the reference runs it: one sequential loop over the immature points,
// ImmaturePoint::traceOn per point.  T1-T16: DESIGN.md section 14.  The per-sample arithmetic is trace_math.hpp and point_math.hpp,
// shared with the device kernel; the sums over the pattern are plain loops in pattern order.
// ---------------------------------------------------------------------------------------------
extern "C" int dsm_trace_params_default(dsm_trace_params *p) {
  if (!p) return DSM_ERR_INVALID;
  p->max_pix_search = 0.027f, p->slack_interval = 1.5f, p->stepsize = 1.0f, p->min_improvement = 2.0f;
  p->min_test_radius = 2, p->gn_iterations = 3;
  p->gn_threshold = 0.1f, p->extra_slack_on_th = 1.2f, p->huber_th = 9.0f;
  return DSM_OK;
}

extern "C" int dsm_trace_points_host(int w, int h, const float *target_I, const dsm_trace_job *job, const dsm_trace_params *params) {
  using namespace dsm::trc;
  using namespace dsm::pt;
  auto fail = [](const char *msg) { return refuse("dsm_trace_points_host", msg); };
  if (w < 8 || h < 8 || !target_I || !job) return fail("bad argument");
  if (const char *e = dsm::trace_params_error(params)) return fail(e);
  if (const char *e = dsm::trace_job_error(*job)) return fail(e);
  const dsm_trace_job &J = *job;
  const dsm_trace_params &S = *params;
  int counts[6] = {0, 0, 0, 0, 0, 0};
  for (int i = 0; i < J.n_pts; i++) {
    const float *R = J.krki + 9 * J.host[i], *t = J.kt + 3 * J.host[i], *aff = J.aff + 2 * J.host[i];
    const float *color = J.color + 8 * i, *wt = J.weights + 8 * i;
    const int entered = J.status[i];
    Point P{entered, J.idepth_min[i], J.idepth_max[i], J.quality[i], J.trace_uv[2 * i], J.trace_uv[2 * i + 1], J.trace_interval[i]};
    Line L;
    int steps = 0;
    if (geometry(w, h, R, t, J.u[i], J.v[i], J.grad_h + 4 * i, S, P, L)) {
      steps = L.numSteps;
      float rx[8], ry[8], errors[DSM_TRACE_MAX_STEPS + 1];
      for (int k = 0; k < 8; k++) rotated_pattern(R, k, rx[k], ry[k]);
      float ptx = L.ptx, pty = L.pty, bestU = 0, bestV = 0, bestEnergy = 1e10f;
      int bestIdx = -1;
      for (int s = 0; s < steps; s++) { // T9
        float energy = 0;
        for (int k = 0; k < 8; k++) {
          const float x = ptx + rx[k], y = pty + ry[k];
          const bool ok = guard(x, y, w, h);
          energy += search_term(ok, ok ? interp_I(load4(target_I, w, x, y), x, y) : 0.f, aff, color[k], S.huber_th);
        }
        errors[s] = energy;
        if (energy < bestEnergy) bestU = ptx, bestV = pty, bestEnergy = energy, bestIdx = s;
        ptx += L.dx;
        pty += L.dy;
      }
      float secondBest = 1e10f; // T10
      for (int s = 0; s < steps; s++)
        if (outside_radius(s, bestIdx, test_radius(S)) && errors[s] < secondBest) secondBest = errors[s];
      quality_update(P, secondBest, bestEnergy, steps);
      GN g{bestU, bestV, bestU, bestV, 0.f, bestEnergy}; // T11
      if (S.gn_iterations > 0) g.bestEnergy = 1e5f;
      for (int it = 0; it < S.gn_iterations; it++) {
        float H = 1, b = 0, E = 0;
        for (int k = 0; k < 8; k++) {
          const float x = g.bestU + rx[k], y = g.bestV + ry[k];
          const bool ok = guard(x, y, w, h);
          float hI = 0, gx = 0, gy = 0, tH, tb, tE;
          if (ok) interp_Ig(load12(target_I, w, x, y), x, y, hI, gx, gy);
          if (gn_terms(ok, hI, gx, gy, aff, color[k], wt[k], S.huber_th, L.dx, L.dy, tH, tb, tE)) H += tH, b += tb;
          E += tE;
        }
        if (gn_update(g, H, b, E, L.dx, L.dy, S.gn_threshold)) break;
      }
      finish(P, L, g, t, J.energy_th[i], S, entered);
    }
    J.status[i] = (unsigned char)P.status;
    J.idepth_min[i] = P.idepth_min, J.idepth_max[i] = P.idepth_max, J.quality[i] = P.quality;
    J.trace_uv[2 * i] = P.uv0, J.trace_uv[2 * i + 1] = P.uv1, J.trace_interval[i] = P.interval;
    if (J.steps_out) J.steps_out[i] = steps;
    counts[P.status]++;
  }
  if (J.counts_out) memcpy(J.counts_out, counts, sizeof counts); // T16
  return DSM_OK;
}

// ---------------------------------------------------------------------------------------------
// FrontEnd::makeNewTraces (FrontEnd.cpp:936-962) as upstream runs it: PixelSelector::makeMaps with select() as ONE sequential loop --
// the direction of a cell is read through the running count n2 of the hits before it, and the bestIdx = -2 flags say that a block
// holds a hit of a finer level -- then the ImmaturePoint constructor per map entry.  P1-P14: DESIGN.md section 15.  The per-pixel
// expressions are select_math.hpp, shared with the device kernels, which run the same rules free of the scan order.
// ---------------------------------------------------------------------------------------------
extern "C" int dsm_select_params_default(dsm_select_params *p) {
  if (!p) return DSM_ERR_INVALID;
  p->min_grad_hist_cut = 0.5f, p->min_grad_hist_add = 7.0f, p->grad_downweight_per_level = 0.75f;
  p->select_direction_distribution = 1, p->th_factor = 1.0f, p->recursions = 1, p->pattern_padding = 2;
  p->outlier_th = 144.0f, p->outlier_th_sum_component = 2500.0f, p->overall_energy_th_weight = 1.0f;
  return DSM_OK;
}

namespace {
struct HostSelector {
  int w, h, w32, h32;
  const float *I0, *I1, *I2, *b_inv;
  const unsigned char *rp;
  const dsm_select_params *S;
  std::vector<float> ths_smoothed;
  std::vector<unsigned char> map;

  void make_hists() { // P2, P3
    std::vector<float> ths((size_t)w32 * h32);
    for (int y = 0; y < h32; y++)
      for (int x = 0; x < w32; x++) {
        int hist[50] = {};
        for (int j = 0; j < 32; j++)
          for (int i = 0; i < 32; i++) {
            const int it = i + 32 * x, jt = j + 32 * y;
            if (!dsm::sel::in_histogram(it, jt, w, h)) continue;
            hist[dsm::sel::hist_bin(dsm::sel::abs_grad(I0, w, h, it, jt, b_inv))]++;
            hist[0]++;
          }
        ths[x + y * w32] = (float)dsm::sel::hist_quantile(hist, S->min_grad_hist_cut) + S->min_grad_hist_add;
      }
    ths_smoothed.resize(ths.size());
    for (int y = 0; y < h32; y++)
      for (int x = 0; x < w32; x++) ths_smoothed[x + y * w32] = dsm::sel::smoothed_threshold(ths.data(), w32, h32, x, y);
  }

  // PixelSelector::select: P5-P9 in upstream's sequential form
  void select(int pot, int n[3]) {
    using namespace dsm::sel;
    std::fill(map.begin(), map.end(), 0);
    int n2 = 0, n3 = 0, n4 = 0;
    for (int y4 = 0; y4 < h; y4 += 4 * pot)
      for (int x4 = 0; x4 < w; x4 += 4 * pot) {
        const int my3 = std::min(4 * pot, h - y4), mx3 = std::min(4 * pot, w - x4);
        long long bestIdx4 = -1;
        float bestVal4 = 0;
        const int dir4 = rp[n2] & 15;
        for (int y3 = 0; y3 < my3; y3 += 2 * pot)
          for (int x3 = 0; x3 < mx3; x3 += 2 * pot) {
            const int x34 = x3 + x4, y34 = y3 + y4;
            const int my2 = std::min(2 * pot, h - y34), mx2 = std::min(2 * pot, w - x34);
            long long bestIdx3 = -1;
            float bestVal3 = 0;
            const int dir3 = rp[n2] & 15;
            for (int y2 = 0; y2 < my2; y2 += pot)
              for (int x2 = 0; x2 < mx2; x2 += pot) {
                const int x234 = x2 + x34, y234 = y2 + y34;
                const int my1 = std::min(pot, h - y234), mx1 = std::min(pot, w - x234);
                long long bestIdx2 = -1;
                float bestVal2 = 0;
                const int dir2 = rp[n2] & 15;
                for (int y1 = 0; y1 < my1; y1++)
                  for (int x1 = 0; x1 < mx1; x1++) {
                    const int xf = x1 + x234, yf = y1 + y234;
                    const long long idx = xf + (long long)w * yf;
                    if (!in_scan_window(xf, yf, w, h)) continue;
                    const float t0 = ths_smoothed[threshold_index(xf, yf, w32, h32)];
                    float gx, gy;
                    const float ag0 = abs_grad(I0, w, h, xf, yf, b_inv, gx, gy);
                    if (ag0 > level_threshold(t0, 0, *S)) {
                      const float dirNorm = rank_value(gx, gy, ag0, dir2, *S);
                      if (dirNorm > bestVal2) bestVal2 = dirNorm, bestIdx2 = idx, bestIdx3 = -2, bestIdx4 = -2;
                    }
                    if (bestIdx3 == -2) continue;
                    const float ag1 = coarse_abs_grad(I1, w, h, 1, xf, yf, b_inv);
                    if (ag1 > level_threshold(t0, 1, *S)) {
                      const float dirNorm = rank_value(gx, gy, ag1, dir3, *S);
                      if (dirNorm > bestVal3) bestVal3 = dirNorm, bestIdx3 = idx, bestIdx4 = -2;
                    }
                    if (bestIdx4 == -2) continue;
                    const float ag2 = coarse_abs_grad(I2, w, h, 2, xf, yf, b_inv);
                    if (ag2 > level_threshold(t0, 2, *S)) {
                      const float dirNorm = rank_value(gx, gy, ag2, dir4, *S);
                      if (dirNorm > bestVal4) bestVal4 = dirNorm, bestIdx4 = idx;
                    }
                  }
                if (bestIdx2 > 0) map[bestIdx2] = 1, bestVal3 = 1e10f, n2++;
              }
            if (bestIdx3 > 0) map[bestIdx3] = 2, bestVal4 = 1e10f, n3++;
          }
        if (bestIdx4 > 0) map[bestIdx4] = 4, n4++;
      }
    n[0] = n2, n[1] = n3, n[2] = n4;
  }
};
} // namespace

extern "C" int dsm_select_pixels_host(int w, int h, const float *I0, const float *I1, const float *I2, const unsigned char *random_pattern,
                                      const dsm_select_job *job, const dsm_select_params *params) {
  using namespace dsm::sel;
  auto fail = [](const char *msg) { return refuse("dsm_select_pixels_host", msg); };
  if (!I0 || !I1 || !I2 || !random_pattern || !job) return fail("bad argument");
  if (const char *e = dsm::select_params_error(params)) return fail(e);
  if (const char *e = dsm::select_geometry_error(w, h)) return fail(e);
  if (const char *e = dsm::select_job_error(*job)) return fail(e);
  const dsm_select_job &J = *job;
  const dsm_select_params &S = *params;
  HostSelector P{w, h, w / 32, h / 32, I0, I1, I2, J.b_inv, random_pattern, params, {}, {}};
  P.map.resize((size_t)w * h);
  P.make_hists();
  int pot = *J.potential_io, passes = 0, n[3];
  Adapt A;
  for (int left = S.recursions;; left--) { // P10
    P.select(pot, n);
    passes++;
    A = adapt(n[0], n[1], n[2], J.density, pot, left);
    if (!A.next_pot) break;
    pot = A.next_pot;
  }
  int num_total = n[0] + n[1] + n[2];
  unsigned char char_th;
  if (thinning(A.quot, char_th)) { // P11
    size_t rn = 0;
    for (size_t i = 0; i < P.map.size(); i++)
      if (P.map[i]) {
        if (random_pattern[rn] > char_th) P.map[i] = 0, num_total--;
        rn++;
      }
  }
  *J.potential_io = A.ideal; // P12
  int n_pts = 0;
  for (int y = 0; y < h; y++) // P13
    for (int x = 0; x < w; x++) {
      const unsigned char m = P.map[x + (size_t)w * y];
      NewPoint Q;
      if (!m || !in_point_window(x, y, w, h, S.pattern_padding) || !construct(I0, w, h, x, y, S, Q)) continue;
      const int i = n_pts++;
      if (i >= J.max_pts) continue;
      J.u[i] = (float)x, J.v[i] = (float)y, J.energy_th[i] = Q.energy_th;
      memcpy(J.grad_h + 4 * (size_t)i, Q.grad_h, 16), memcpy(J.color + 8 * (size_t)i, Q.color, 32), memcpy(J.weights + 8 * (size_t)i, Q.weights, 32);
      J.status[i] = DSM_IPS_UNINITIALIZED, J.idepth_min[i] = 0.f, J.idepth_max[i] = NAN, J.quality[i] = 10000.f, J.type[i] = (float)m;
    }
  *J.n_pts_out = n_pts, *J.num_total_out = num_total;
  if (J.counts_out) memcpy(J.counts_out, n, sizeof n);
  if (J.passes_out) *J.passes_out = passes;
  if (J.map_out) memcpy(J.map_out, P.map.data(), P.map.size());
  return DSM_OK;
}

// ---------------------------------------------------------------------------------------------
// FrontEnd::linearizeAll (dso_helpers/FrontEndOptimize.cpp:121-179) as the reference runs it on one thread: PointFrameResidual::linearize
// per active residual in residual order, then the energy sum, setNewFrameEnergyTH and, with fixLinearization, the keep verdict and the
// relative baseline.  L1-L8, B1-B4: DESIGN.md section 16.  The per-residual expressions are linearize_math.hpp, shared with the device
// kernel; the twelve sums are plain loops in pattern order.
// ---------------------------------------------------------------------------------------------
extern "C" int dsm_linearize_params_default(dsm_linearize_params *p) {
  if (!p) return DSM_ERR_INVALID;
  p->huber_th = DSM_LINEARIZE_HUBER_TH, p->outlier_th_sum_component = DSM_LINEARIZE_OUTLIER_TH_SUM_COMPONENT;
  p->scale_idepth = DSM_LINEARIZE_SCALE_IDEPTH, p->scale_f = DSM_LINEARIZE_SCALE_F, p->scale_c = DSM_LINEARIZE_SCALE_C;
  p->thn = DSM_LINEARIZE_FRAME_ENERGY_TH_N, p->fac_median = DSM_LINEARIZE_FRAME_ENERGY_TH_FAC_MEDIAN;
  p->cw = DSM_LINEARIZE_FRAME_ENERGY_TH_CONST_WEIGHT, p->ow = DSM_LINEARIZE_OVERALL_ENERGY_TH_WEIGHT;
  p->zero_jab_a = 0, p->zero_jab_b = 0;
  return DSM_OK;
}

extern "C" int dsm_linearize_residuals_host(int w, int h, const dsm_linearize_job *job, const float *const *frame_I,
                                            const dsm_linearize_params *params) {
  using namespace dsm::lin;
  auto fail = [](const char *msg) { return refuse("dsm_linearize_residuals_host", msg); };
  if (w < 8 || h < 8 || !job || !frame_I) return fail("bad argument");
  if (const char *e = dsm::linearize_params_error(params)) return fail(e);
  if (const char *e = dsm::linearize_job_error(*job)) return fail(e);
  const dsm_linearize_job &J = *job;
  for (int f = 0; f < J.n_frames; f++)
    if (!frame_I[f]) return fail("NULL frame");
  const Cam C{J.cam[0], J.cam[1], J.cam[2], J.cam[3], J.cam_inv[0], J.cam_inv[1], w, h};
  const Settings S{params->huber_th, params->outlier_th_sum_component, params->scale_idepth, params->scale_f, params->scale_c};
  const int nf = J.n_frames;
  for (int r = 0; r < J.n_res; r++) {
    const int p = J.point[r], tgt = J.target[r], hst = J.host[p], pair = hst * nf + tgt;
    const float *M = J.pre_KRKiTll + 9 * pair, *Kt = J.pre_KtTll + 3 * pair;
    int state = RES_OOB; // L1
    float E = J.energy_in[r], with_outlier = -1.0f;
    float row[J_FLOATS], proj[16];
    Centre c;
    if (J.state_in[r] != DSM_RES_OOB && centre(C, J.pre_RTll_0 + 9 * pair, J.pre_tTll_0 + 3 * pair, J.u[p], J.v[p], J.idepth_zero_scaled[p], c)) {
      geometric(C, J.pre_RTll_0 + 9 * pair, J.pre_tTll_0 + 3 * pair, c, S, row + J_PDXI);
      float sum[N_SUMS];
      for (int k = 0; k < N_SUMS; k++) sum[k] = 0.0f;
      int idx = 0;
      for (; idx < 8; idx++) { // L4-L6
        int dx, dy;
        dsm::pt::pattern(idx, dx, dy);
        Pixel P;
        if (!pixel(C, frame_I[tgt], M, Kt, J.pre_aff_mode + 2 * pair, J.pre_b0_mode[pair], J.u[p], J.v[p], dx, dy, J.idepth_scaled[p],
                   J.color[8 * p + idx], J.weights[8 * p + idx], S, P))
          break;
        proj[2 * idx] = P.Ku, proj[2 * idx + 1] = P.Kv;
        row[J_RESF + idx] = P.resF, row[J_IDX + idx] = P.gx, row[J_IDX + 8 + idx] = P.gy;
        row[J_ABF + idx] = params->zero_jab_a ? 0.0f : P.ja, row[J_ABF + 8 + idx] = params->zero_jab_b ? 0.0f : P.jb;
        for (int k = 0; k < N_SUMS; k++) sum[k] += P.T[k];
      }
      if (idx == 8) {
        row[J_IDX2] = sum[S_XX], row[J_IDX2 + 1] = row[J_IDX2 + 2] = sum[S_XY], row[J_IDX2 + 3] = sum[S_YY];
        row[J_ABJIDX] = sum[S_AX], row[J_ABJIDX + 1] = sum[S_AY], row[J_ABJIDX + 2] = sum[S_BX], row[J_ABJIDX + 3] = sum[S_BY];
        row[J_AB2] = sum[S_AA], row[J_AB2 + 1] = row[J_AB2 + 2] = sum[S_AB], row[J_AB2 + 3] = sum[S_BB];
        with_outlier = E = sum[S_E];
        state = verdict(E, sum[S_WJI2], J.frame_energy_th[hst], J.frame_energy_th[tgt]); // L7
      }
    }
    J.new_state[r] = (unsigned char)state, J.new_energy[r] = E, J.new_energy_with_outlier[r] = with_outlier;
    if (state != RES_OOB) { // L8
      if (J.J_out) memcpy(J.J_out + (size_t)J_FLOATS * r, row, sizeof row);
      if (J.projected_to) memcpy(J.projected_to + (size_t)16 * r, proj, sizeof proj);
      if (J.center_projected_to) {
        float *q = J.center_projected_to + (size_t)3 * r;
        q[0] = c.Ku, q[1] = c.Kv, q[2] = c.new_idepth;
      }
    }
    if (J.fix_linearization) { // B3
      const bool keep = J.state_in[r] != DSM_RES_OOB && state == RES_IN;
      if (J.keep) J.keep[r] = keep;
      if (J.rel_bs) J.rel_bs[r] = keep && J.is_new[r] ? rel_baseline(M, Kt, J.u[p], J.v[p], J.idepth_scaled[p]) : 0.0f;
    }
  }
  dsm::linearize_job_summary(J, *params); // B1, B2
  return DSM_OK;
}

// ---------------------------------------------------------------------------------------------
// accumulateAF_MT / accumulateSCF_MT of FrontEnd::optimize (dso_helpers/FrontEndOptimize.cpp:332-486) after linearizeAll, as one thread
// runs them: the linearisation above, then per active residual its record (A1, A2), the pair accumulators in residual order (A3, P1),
// the points' sums (S1, S2), the Schur accumulators in point order (S3) and the stitch (T1).  DESIGN.md section 17; the expressions
// are hessian_math.hpp, shared with the device kernels.
// ---------------------------------------------------------------------------------------------
extern "C" int dsm_window_hessian_host(int w, int h, const dsm_hessian_job *job, const float *const *frame_I, const dsm_linearize_params *params) {
  return dsm::hessian_host_run(w, h, job, frame_I, params, nullptr, nullptr);
}

// the host form above; after_lin (or null) sees the linearisation's result and may rewrite the rows before anything accumulates
// (dsm_window_marginalize_host: X1 of section 21)
int dsm::hessian_host_run(int w, int h, const dsm_hessian_job *job, const float *const *frame_I, const dsm_linearize_params *params,
                          void (*after_lin)(void *user, const dsm_linearize_job &L, float *rows), void *user) {
  using namespace dsm::hes;
  auto fail = [](const char *msg) { return refuse("dsm_window_hessian_host", msg); };
  if (w < 8 || h < 8 || !job || !frame_I) return fail("bad argument");
  if (const char *e = dsm::linearize_params_error(params)) return fail(e);
  if (const char *e = dsm::linearize_job_error(job->lin)) return fail(e);
  if (const char *e = dsm::hessian_job_error(*job)) return fail(e);
  const dsm_hessian_job &J = *job;
  for (int f = 0; f < J.lin.n_frames; f++)
    if (!frame_I[f]) return fail("NULL frame");
  const int nf = J.lin.n_frames, np = J.lin.n_pts, nr = J.lin.n_res;
  dsm_linearize_job L = J.lin;
  std::vector<float> rows;
  if (!L.J_out) rows.resize((size_t)nr * dsm::lin::J_FLOATS), L.J_out = rows.data();
  const int rc = dsm_linearize_residuals_host(w, h, &L, frame_I, params);
  if (rc) return rc;
  if (after_lin) after_lin(user, L, L.J_out);
  const size_t n2 = (size_t)nf * nf;
  std::vector<double> top(n2 * 169, 0.0), D(n2 * nf * 64, 0.0), E(n2 * 32, 0.0), EB(n2 * 8, 0.0), Hcc(16, 0.0), bc(4, 0.0);
  std::vector<float> rec((size_t)nr * R_FLOATS), prec((size_t)np * P_FLOATS, 0.0f);
  std::vector<unsigned char> act((size_t)nr);
  std::vector<int> start((size_t)np + 1, 0), list((size_t)nr), n_act((size_t)np, 0);
  for (int r = 0; r < nr; r++) start[L.point[r] + 1]++;
  for (int p = 0; p < np; p++) start[p + 1] += start[p];
  {
    std::vector<int> at(start.begin(), start.end() - 1);
    for (int r = 0; r < nr; r++) list[at[L.point[r]]++] = r; // ascending within a point
  }
  for (int r = 0; r < nr; r++) { // A0-A3, P1
    act[r] = L.state_in[r] != DSM_RES_OOB && L.new_state[r] == DSM_RES_IN;
    if (J.active) J.active[r] = act[r];
    if (!act[r]) continue;
    float *q = rec.data() + (size_t)r * R_FLOATS;
    residual_record(L.J_out + (size_t)r * dsm::lin::J_FLOATS, q);
    if (J.JpJdF) memcpy(J.JpJdF + (size_t)8 * r, q + R_JP, 32);
    double *T = top.data() + (size_t)(L.host[L.point[r]] * nf + L.target[r]) * 169;
    for (int a = 0; a < kTop; a++)
      for (int b = a; b < kTop; b++) T[a * kTop + b] += (double)top_term(q, a, b);
  }
  for (size_t pair = 0; pair < n2; pair++)
    for (int a = 0; a < kTop; a++)
      for (int b = a + 1; b < kTop; b++) top[pair * 169 + b * kTop + a] = top[pair * 169 + a * kTop + b];
  for (int p = 0; p < np; p++) { // S1, S2
    float *P = prec.data() + (size_t)p * P_FLOATS;
    for (int k = start[p]; k < start[p + 1]; k++)
      if (act[list[k]]) point_add(rec.data() + (size_t)list[k] * R_FLOATS, P[P_BD], P[P_HDD], P[P_HCD], P[P_HCD + 1], P[P_HCD + 2], P[P_HCD + 3]), n_act[p]++;
    point_finish(P, n_act[p], J.prior ? J.prior[p] : 0.0f, J.delta ? J.delta[p] : 0.0f, J.hdd_lin ? J.hdd_lin[p] : 0.0f,
                 J.bd_lin ? J.bd_lin[p] : 0.0f, J.hcd_lin ? J.hcd_lin + 4 * p : nullptr, J.shift_prior_to_zero != 0);
    if (J.hdd_acc) J.hdd_acc[p] = P[P_HDD];
    if (J.bd_acc) J.bd_acc[p] = P[P_BD];
    if (J.hcd_acc) memcpy(J.hcd_acc + 4 * p, P + P_HCD, 16);
    if (J.hdi) J.hdi[p] = P[P_HDI];
    if (J.bd_sum) J.bd_sum[p] = P[P_BDSUM];
    if (J.idepth_hessian) J.idepth_hessian[p] = P[P_IDH];
  }
  for (int p = 0; p < np; p++) { // S3
    if (!n_act[p]) continue;
    const float *P = prec.data() + (size_t)p * P_FLOATS;
    const int hst = L.host[p];
    for (int c = 0; c < 4; c++) {
      for (int d = 0; d < 4; d++) Hcc[4 * c + d] += (double)term_Hcc(P, c, d);
      bc[c] += (double)term_bc(P, c);
    }
    for (int k1 = start[p]; k1 < start[p + 1]; k1++) {
      const int r1 = list[k1];
      if (!act[r1]) continue;
      const float *j1 = rec.data() + (size_t)r1 * R_FLOATS + R_JP;
      const size_t p1 = (size_t)(hst * nf + L.target[r1]);
      for (int a = 0; a < 8; a++) {
        for (int c = 0; c < 4; c++) E[p1 * 32 + 4 * a + c] += (double)term_E(P, j1, a, c);
        EB[p1 * 8 + a] += (double)term_EB(P, j1, a);
      }
      for (int k2 = start[p]; k2 < start[p + 1]; k2++) {
        const int r2 = list[k2];
        if (!act[r2]) continue;
        const float *j2 = rec.data() + (size_t)r2 * R_FLOATS + R_JP;
        double *Dk = D.data() + (p1 * nf + L.target[r2]) * 64;
        for (int a = 0; a < 8; a++)
          for (int b = 0; b < 8; b++) Dk[8 * a + b] += (double)term_D(P, j1, j2, a, b);
      }
    }
  }
  dsm::hessian_stitch(J, top.data(), D.data(), E.data(), EB.data(), Hcc.data(), bc.data());
  return DSM_OK;
}
