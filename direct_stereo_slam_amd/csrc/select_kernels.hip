// select_kernels.hip -- FrontEnd::makeNewTraces (FrontEnd.cpp:936-962) on the device: PixelSelector::makeMaps and the ImmaturePoint
// constructor for the new keyframes of many sequences, in one call.  Semantics: P1-P14 of DESIGN.md section 15.
//
// Upstream's select() is one loop in which every cell reads its random direction through the count n2 of the level-1 hits before it.
// Here it is restated free of the scan order, and only the count itself is a chain:
//   select_hist_kernel     one workgroup per 32 x 32 block: the gradient histogram in LDS (integer atomics), the quantile (P2)
//   select_smooth_kernel   one lane per block: the smoothed squared thresholds (P3); sets the job's state
//   per pass (recursions + 1 of them are always enqueued; a job that no longer recurses leaves each kernel at once):
//   select_mask_kernel     one lane per pixel: bit d of its cell's mask is set if the pixel would make the cell a level-1 hit under
//                          direction d (an integer OR, so its order does not matter); clears the map
//   select_chain_kernel    ONE wave per job walks the cells in upstream's nested order, 64 at a time.  A group whose masks are all
//                          0 or 0xFFFF does not depend on the directions: n2 advances by a popcount.  Any other group takes 64 steps
//                          on scalars: the masks sit one per lane, rp[n2 .. n2 + 63] is loaded once (n2 moves by at most 64), both
//                          are read with v_readlane, and no memory access sits on the dependent chain.  Out: the direction of every cell.
//   select_key_kernel      one lane per pixel: with the directions known, "the first pixel in scan order with the largest dirNorm"
//                          (P7-P9) is the maximum of the 64-bit key (dirNorm's bits, ~scan rank) per cell, per 2 pot block and per
//                          4 pot block: three integer atomic maxima
//   select_resolve_kernel  one lane per 4 pot block: the hits of the three levels from the keys, with the rule that a block holding a
//                          finer hit gets none; n3 and n4 are integer counts
//   select_decide_kernel   one lane per job: P10, in device memory
//   after the last pass:
//   select_rows_kernel     one wave per row: map entries per row
//   select_thin_kernel     one wave per row: the raster rank of every entry (rows before + ballot prefix), the thinning (P11), and
//                          which entries are points (P13, and P14's finite test)
//   select_points_kernel   one wave per row: the rank of every point, the constructor (P14), the compacted point arrays
// No float atomics, no kernel waits for another workgroup, every loop is bounded by the geometry.  Potentials far above those
// makeMaps settles on (one cell of thousands of pixels) cost no more than any other: no lane ever walks a cell.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "call_arena.hpp"
#include "select_math.hpp"

using namespace dsm;

namespace {

typedef unsigned long long u64;

struct SelState { // per job, in its scratch
  int pot, done, passes, n2, n3, n4, thin, char_th, ideal;
};

struct SelLayout { // byte offsets into a job's scratch, and the sizes behind them
  size_t ths, ths_smoothed, dirs, map, rowcnt, rowkept, rowpts, stride;
  size_t masks, best1, best2, best3, atom_stride; // into a job's block of the buffer that is zeroed before every pass
  int ncell;                                      // cells at potential 1, in the padded nested order: 16 per 4 x 4 block
};

struct SelJob {
  const float *I0, *I1, *I2, *b_inv;
  unsigned char *scratch, *atoms, *map_out;
  unsigned *out; // kHeaderWords, then u, v, energy_th, grad_h, color, weights, type over max_pts points
  float density;
  int pot0, max_pts;
};

constexpr int kHeaderWords = 8;      // n_pts, num_total, n2, n3, n4, passes, potential, spare
constexpr int kPointWords = 24;      // u, v, energy_th, grad_h (4), color (8), weights (8), type
constexpr int kMaxJobs = 4096;

struct Cells { // the nested enumeration of P5 at one potential, padded: a 4 pot block always has 16 cells, those cut away stay empty
  int pot, nbx4, nby4;
  __host__ __device__ Cells(int w, int h, int p) : pot(p), nbx4((w + 4 * p - 1) / (4 * p)), nby4((h + 4 * p - 1) / (4 * p)) {}
  __host__ __device__ int blocks() const { return nbx4 * nby4; }
  __host__ __device__ int cells() const { return 16 * nbx4 * nby4; }
};
struct CellOf { // where a pixel sits
  int b4, l, r1; // 4 pot block; cell in the block, in scan order; raster rank in the cell
  __device__ CellOf(const Cells &C, int x, int y) {
    const int cx = x / C.pot, cy = y / C.pot;
    b4 = (cy >> 2) * C.nbx4 + (cx >> 2);
    l = ((cy >> 1) & 1) * 8 + ((cx >> 1) & 1) * 4 + (cy & 1) * 2 + (cx & 1);
    r1 = (y - cy * C.pot) * C.pot + (x - cx * C.pot);
  }
};
// the pixel of cell l of block b4 with raster rank r1
__device__ __forceinline__ int pixel_of(const Cells &C, int w, int b4, int l, int r1) {
  const int cx = (b4 % C.nbx4) * 4 + ((l >> 2) & 1) * 2 + (l & 1), cy = (b4 / C.nbx4) * 4 + ((l >> 3) & 1) * 2 + ((l >> 1) & 1);
  return (cy * C.pot + r1 / C.pot) * w + cx * C.pot + r1 % C.pot;
}
// larger value first, then the smaller scan rank; v > 0, so its bits order as the floats do
__device__ __forceinline__ u64 make_key(float v, int rank) { return ((u64)__float_as_uint(v) << 32) | (u64)(0xffffffffu - (unsigned)rank); }
// The maximum of a slot only grows, so a key that does not beat what the slot is seen to hold (however stale the sight) cannot be the
// maximum and needs no atomic: at large potentials thousands of pixels share a slot, and most of them stop here.
__device__ __forceinline__ void key_max(u64 *slot, u64 key) {
  if (key > __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(slot, key);
}
__device__ __forceinline__ int key_rank(u64 k) { return (int)(0xffffffffu - (unsigned)(k & 0xffffffffu)); }

template <typename T> __device__ __forceinline__ T *at(unsigned char *base, size_t off) { return reinterpret_cast<T *>(base + off); }
__device__ __forceinline__ SelState *state_of(const SelJob &J) { return reinterpret_cast<SelState *>(J.scratch); }

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}
__device__ __forceinline__ int rows_before(const int *cnt, int y, int lane) { // integer sums: any order
  int s = 0;
  for (int i = lane; i < y; i += 64) s += cnt[i];
  return wave_sum(s);
}

__global__ __launch_bounds__(256) void select_hist_kernel(const SelJob *jobs, SelLayout L, int w, int h, dsm_select_params S) {
  __shared__ int hist[50];
  const SelJob &J = jobs[blockIdx.y];
  const int w32 = w / 32, bx = (int)blockIdx.x % w32, by = (int)blockIdx.x / w32, tid = threadIdx.x;
  if (tid < 50) hist[tid] = 0;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int p = tid + 256 * k, it = (p & 31) + 32 * bx, jt = (p >> 5) + 32 * by;
    if (sel::in_histogram(it, jt, w, h)) atomicAdd(&hist[sel::hist_bin(sel::abs_grad(J.I0, w, h, it, jt, J.b_inv))], 1);
  }
  __syncthreads();
  if (tid == 0) {
    int all = 0;
    for (int i = 1; i < 50; i++) all += hist[i];
    hist[0] = all;
    at<float>(J.scratch, L.ths)[blockIdx.x] = (float)sel::hist_quantile(hist, S.min_grad_hist_cut) + S.min_grad_hist_add;
  }
}

__global__ __launch_bounds__(64) void select_smooth_kernel(const SelJob *jobs, SelLayout L, int w, int h) {
  const SelJob &J = jobs[blockIdx.y];
  const int w32 = w / 32, h32 = h / 32, b = (int)(blockIdx.x * 64 + threadIdx.x);
  if (b == 0) *state_of(J) = SelState{J.pot0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (b < w32 * h32) at<float>(J.scratch, L.ths_smoothed)[b] = sel::smoothed_threshold(at<const float>(J.scratch, L.ths), w32, h32, b % w32, b / w32);
}

__global__ __launch_bounds__(256) void select_mask_kernel(const SelJob *jobs, SelLayout L, int w, int h, dsm_select_params S) {
  const SelJob &J = jobs[blockIdx.y];
  const SelState *St = state_of(J);
  if (St->done) return;
  const int p = (int)(blockIdx.x * 256 + threadIdx.x);
  if (p >= w * h) return;
  const int x = p % w, y = p / w;
  at<unsigned char>(J.scratch, L.map)[p] = 0;
  if (!sel::in_scan_window(x, y, w, h)) return;
  const float t0 = at<const float>(J.scratch, L.ths_smoothed)[sel::threshold_index(x, y, w / 32, h / 32)];
  float gx, gy;
  const float ag0 = sel::abs_grad(J.I0, w, h, x, y, J.b_inv, gx, gy);
  if (!(ag0 > sel::level_threshold(t0, 0, S))) return;
  unsigned bits = 0;
#pragma unroll
  for (int d = 0; d < 16; d++)
    if (sel::rank_value(gx, gy, ag0, d, S) > 0.f) bits |= 1u << d;
  if (!bits) return;
  const Cells C(w, h, St->pot);
  const CellOf c(C, x, y);
  atomicOr(at<unsigned>(J.atoms, L.masks) + (c.b4 * 16 + c.l), bits);
}

__global__ __launch_bounds__(64) void select_chain_kernel(const SelJob *jobs, SelLayout L, int w, int h, const unsigned char *rp) {
  const SelJob &J = jobs[blockIdx.x];
  SelState *St = state_of(J);
  if (St->done) return;
  const int lane = threadIdx.x, last = w * h - 1;
  const int ncell = Cells(w, h, St->pot).cells();
  const unsigned *masks = at<const unsigned>(J.atoms, L.masks);
  unsigned char *dirs = at<unsigned char>(J.scratch, L.dirs);
  int n2 = 0;
  for (int g0 = 0; g0 < ncell; g0 += 64) {
    const int c = g0 + lane;
    const unsigned m = c < ncell ? masks[c] : 0u;
    unsigned byte = 0;
    if (__ballot(m != 0u && m != 0xffffu) == 0ull) { // no cell of the group depends on its direction
      const u64 full = __ballot(m == 0xffffu);
      byte = rp[min(n2 + (int)__popcll(full & ((1ull << lane) - 1ull)), last)];
      n2 += (int)__popcll(full);
    } else {
      const unsigned window = rp[min(n2 + lane, last)];
      const int base = n2;
#pragma unroll
      for (int i = 0; i < 64; i++) {
        const unsigned mi = __builtin_amdgcn_readlane(m, i);
        const unsigned bi = __builtin_amdgcn_readlane(window, __builtin_amdgcn_readfirstlane(n2 - base)); // n2 - base <= i
        if (lane == i) byte = bi;
        n2 += (int)((mi >> (bi & 15u)) & 1u);
      }
    }
    if (c < ncell) dirs[c] = (unsigned char)(byte & 15u);
  }
  if (lane == 0) St->n2 = n2, St->n3 = 0, St->n4 = 0;
}

__global__ __launch_bounds__(256) void select_key_kernel(const SelJob *jobs, SelLayout L, int w, int h, dsm_select_params S) {
  const SelJob &J = jobs[blockIdx.y];
  const SelState *St = state_of(J);
  if (St->done) return;
  const int p = (int)(blockIdx.x * 256 + threadIdx.x);
  if (p >= w * h) return;
  const int x = p % w, y = p / w;
  if (!sel::in_scan_window(x, y, w, h)) return;
  const float t0 = at<const float>(J.scratch, L.ths_smoothed)[sel::threshold_index(x, y, w / 32, h / 32)];
  const sel::Pixel P = sel::pixel(J.I0, J.I1, J.I2, w, h, x, y, J.b_inv, t0, S);
  if (!P.above[0] && !P.above[1] && !P.above[2]) return;
  const Cells C(w, h, St->pot);
  const CellOf c(C, x, y);
  const int pot2 = C.pot * C.pot;
  const unsigned char *dirs = at<const unsigned char>(J.scratch, L.dirs) + c.b4 * 16; // a block's direction is its first cell's
  if (P.above[0]) {
    const float v = sel::rank_value(P.gx, P.gy, P.ag[0], dirs[c.l], S);
    if (v > 0.f) key_max(at<u64>(J.atoms, L.best1) + (c.b4 * 16 + c.l), make_key(v, c.r1));
  }
  if (P.above[1]) {
    const float v = sel::rank_value(P.gx, P.gy, P.ag[1], dirs[c.l & 12], S);
    if (v > 0.f) key_max(at<u64>(J.atoms, L.best2) + (c.b4 * 4 + (c.l >> 2)), make_key(v, (c.l & 3) * pot2 + c.r1));
  }
  if (P.above[2]) {
    const float v = sel::rank_value(P.gx, P.gy, P.ag[2], dirs[0], S);
    if (v > 0.f) key_max(at<u64>(J.atoms, L.best3) + c.b4, make_key(v, c.l * pot2 + c.r1));
  }
}

__global__ __launch_bounds__(256) void select_resolve_kernel(const SelJob *jobs, SelLayout L, int w, int h) {
  const SelJob &J = jobs[blockIdx.y];
  SelState *St = state_of(J);
  if (St->done) return;
  const Cells C(w, h, St->pot);
  const int b4 = (int)(blockIdx.x * 256 + threadIdx.x);
  if (b4 >= C.blocks()) return;
  const int pot2 = C.pot * C.pot;
  unsigned char *map = at<unsigned char>(J.scratch, L.map);
  const u64 *best1 = at<const u64>(J.atoms, L.best1) + b4 * 16, *best2 = at<const u64>(J.atoms, L.best2) + b4 * 4;
  unsigned finer = 0; // the 2 pot blocks that hold a level-1 hit (P8)
  for (int l = 0; l < 16; l++) {
    const u64 k = best1[l];
    if (k) map[pixel_of(C, w, b4, l, key_rank(k))] = 1, finer |= 1u << (l >> 2);
  }
  int n3 = 0, n4 = 0;
  for (int q = 0; q < 4; q++) {
    const u64 k = (finer >> q) & 1u ? 0ull : best2[q];
    if (k) {
      const int r = key_rank(k);
      map[pixel_of(C, w, b4, q * 4 + r / pot2, r % pot2)] = 2, n3++;
    }
  }
  if (!finer && !n3) { // P9
    const u64 k = at<const u64>(J.atoms, L.best3)[b4];
    if (k) {
      const int r = key_rank(k);
      map[pixel_of(C, w, b4, r / pot2, r % pot2)] = 4, n4++;
    }
  }
  if (n3) atomicAdd(&St->n3, n3);
  if (n4) atomicAdd(&St->n4, n4);
}

__global__ __launch_bounds__(64) void select_decide_kernel(const SelJob *jobs, int n_jobs, dsm_select_params S) {
  const int j = (int)(blockIdx.x * 64 + threadIdx.x);
  if (j >= n_jobs) return;
  SelState *St = state_of(jobs[j]);
  if (St->done) return;
  const sel::Adapt A = sel::adapt(St->n2, St->n3, St->n4, jobs[j].density, St->pot, S.recursions - St->passes);
  St->passes++;
  if (A.next_pot) {
    St->pot = A.next_pot;
    return;
  }
  unsigned char char_th = 0;
  St->thin = sel::thinning(A.quot, char_th) ? 1 : 0;
  St->char_th = char_th, St->ideal = A.ideal, St->done = 1;
}

__global__ __launch_bounds__(64) void select_rows_kernel(const SelJob *jobs, SelLayout L, int w, int h) {
  const SelJob &J = jobs[blockIdx.y];
  const int y = blockIdx.x, lane = threadIdx.x;
  const unsigned char *row = at<const unsigned char>(J.scratch, L.map) + (size_t)y * w;
  int n = 0;
  for (int x = lane; x < w; x += 64) n += row[x] != 0;
  n = wave_sum(n);
  if (lane == 0) at<int>(J.scratch, L.rowcnt)[y] = n;
}

__global__ __launch_bounds__(64) void select_thin_kernel(const SelJob *jobs, SelLayout L, int w, int h, dsm_select_params S, const unsigned char *rp) {
  const SelJob &J = jobs[blockIdx.y];
  const SelState *St = state_of(J);
  const int y = blockIdx.x, lane = threadIdx.x;
  unsigned char *row = at<unsigned char>(J.scratch, L.map) + (size_t)y * w;
  int rn = rows_before(at<const int>(J.scratch, L.rowcnt), y, lane), kept = 0, pts = 0;
  for (int x0 = 0; x0 < w; x0 += 64) {
    const int x = x0 + lane;
    unsigned char m = x < w ? row[x] : 0;
    const u64 entries = __ballot(m != 0);
    if (m && St->thin && (int)rp[rn + (int)__popcll(entries & ((1ull << lane) - 1ull))] > St->char_th) m = 0; // P11
    sel::NewPoint Q;
    const bool point = m && sel::in_point_window(x, y, w, h, S.pattern_padding) && sel::construct(J.I0, w, h, x, y, S, Q);
    if (x < w) {
      row[x] = (unsigned char)(m | (point ? 0x80 : 0)); // bit 7: the entry is a point (P13)
      if (J.map_out) J.map_out[(size_t)y * w + x] = m;
    }
    rn += (int)__popcll(entries), kept += (int)__popcll(__ballot(m != 0)), pts += (int)__popcll(__ballot(point));
  }
  if (lane == 0) at<int>(J.scratch, L.rowkept)[y] = kept, at<int>(J.scratch, L.rowpts)[y] = pts;
}

__global__ __launch_bounds__(64) void select_points_kernel(const SelJob *jobs, SelLayout L, int w, int h, dsm_select_params S) {
  const SelJob &J = jobs[blockIdx.y];
  const SelState *St = state_of(J);
  const int y = blockIdx.x, lane = threadIdx.x;
  const int *rowpts = at<const int>(J.scratch, L.rowpts);
  int at_pt = rows_before(rowpts, y, lane);
  if (y == h - 1) { // the last row's wave also writes the header
    const int kept = rows_before(at<const int>(J.scratch, L.rowkept), h, lane);
    if (lane == 0) {
      int *hd = reinterpret_cast<int *>(J.out);
      hd[0] = at_pt + rowpts[y], hd[1] = kept, hd[2] = St->n2, hd[3] = St->n3, hd[4] = St->n4, hd[5] = St->passes, hd[6] = St->ideal, hd[7] = 0;
    }
  }
  const unsigned char *row = at<const unsigned char>(J.scratch, L.map) + (size_t)y * w;
  float *out = reinterpret_cast<float *>(J.out + kHeaderWords);
  const size_t n = (size_t)J.max_pts;
  for (int x0 = 0; x0 < w; x0 += 64) {
    const int x = x0 + lane;
    const unsigned char m = x < w ? row[x] : 0;
    const u64 points = __ballot((m & 0x80) != 0);
    const size_t i = (size_t)(at_pt + (int)__popcll(points & ((1ull << lane) - 1ull)));
    sel::NewPoint Q;
    if ((m & 0x80) && i < n && sel::construct(J.I0, w, h, x, y, S, Q)) { // P14
      out[i] = (float)x, out[n + i] = (float)y, out[2 * n + i] = Q.energy_th;
#pragma unroll
      for (int k = 0; k < 4; k++) out[3 * n + 4 * i + k] = Q.grad_h[k];
#pragma unroll
      for (int k = 0; k < 8; k++) out[7 * n + 8 * i + k] = Q.color[k], out[15 * n + 8 * i + k] = Q.weights[k];
      out[23 * n + i] = (float)(m & 0x7f);
    }
    at_pt += (int)__popcll(points);
  }
}

size_t round256(size_t b) { return (b + 255) & ~(size_t)255; }

} // namespace

struct dsm_pixel_selector {
  dsm_context *ctx = nullptr;
  int w = 0, h = 0, max_jobs = 0;
  SelLayout L{};
  unsigned char *d_rp = nullptr, *d_scratch = nullptr, *d_atoms = nullptr;
  std::vector<size_t> o_binv, o_out, o_map; // a call's arena offsets per job, sized once
};

extern "C" int dsm_pixel_selector_create(dsm_context *ctx, int w, int h, int max_jobs, const unsigned char *random_pattern, dsm_pixel_selector **sel_out) {
  auto bad = [](const char *msg) { return invalid((std::string("dsm_pixel_selector_create: ") + msg).c_str()); };
  if (!ctx || !random_pattern || !sel_out || max_jobs < 1 || max_jobs > kMaxJobs) return bad("bad argument");
  if (const char *e = select_geometry_error(w, h)) return bad(e);
  DSM_HIP(hipSetDevice(ctx->device));
  dsm_pixel_selector *s = new dsm_pixel_selector;
  s->ctx = ctx, s->w = w, s->h = h, s->max_jobs = max_jobs;
  s->o_binv.resize(max_jobs), s->o_out.resize(max_jobs), s->o_map.resize(max_jobs);
  const size_t wh = (size_t)w * h, nb = (size_t)(w / 32) * (h / 32);
  SelLayout &L = s->L;
  L.ncell = Cells(w, h, 1).cells();
  const size_t ncell = round256((size_t)L.ncell);
  size_t o = round256(sizeof(SelState));
  L.ths = o, o += round256(4 * nb);
  L.ths_smoothed = o, o += round256(4 * nb);
  L.dirs = o, o += ncell;
  L.map = o, o += round256(wh);
  L.rowcnt = o, o += round256(4 * (size_t)h);
  L.rowkept = o, o += round256(4 * (size_t)h);
  L.rowpts = o, o += round256(4 * (size_t)h);
  L.stride = o;
  o = 0;
  L.masks = o, o += 4 * ncell;
  L.best1 = o, o += 8 * ncell;
  L.best2 = o, o += 2 * ncell;
  L.best3 = o, o += round256(ncell / 2);
  L.atom_stride = o;
  hipError_t e = hipMalloc(&s->d_rp, wh);
  if (e == hipSuccess) e = hipMalloc(&s->d_scratch, L.stride * max_jobs);
  if (e == hipSuccess) e = hipMalloc(&s->d_atoms, L.atom_stride * max_jobs);
  if (e == hipSuccess) e = hipMemcpyAsync(s->d_rp, random_pattern, wh, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) {
    dsm_pixel_selector_destroy(s);
    DSM_HIP(e);
  }
  *sel_out = s;
  return DSM_OK;
}

extern "C" int dsm_pixel_selector_destroy(dsm_pixel_selector *s) {
  if (!s) return DSM_OK;
  (void)hipSetDevice(s->ctx->device);
  if (s->d_rp) (void)hipFree(s->d_rp);
  if (s->d_scratch) (void)hipFree(s->d_scratch);
  if (s->d_atoms) (void)hipFree(s->d_atoms);
  delete s;
  return DSM_OK;
}

namespace {
// all-or-nothing validation of a batch: nothing is enqueued before every job has passed
int check_jobs(const dsm_pixel_selector *sel, int n_jobs, const dsm_select_job *jobs, const dsm_select_params *params) {
  auto bad = [](const char *msg) { return invalid((std::string("dsm_select_pixels_batch: ") + msg).c_str()); };
  if (!sel || !jobs || n_jobs < 1) return bad("bad argument");
  if (n_jobs > sel->max_jobs) return bad("more jobs than the selector was created for");
  if (const char *e = select_params_error(params)) return bad(e);
  for (int j = 0; j < n_jobs; j++) {
    const dsm_select_job &J = jobs[j];
    if (const char *e = select_job_error(J)) return bad(e);
    const dsm_tracker *t = J.tracker;
    if (!t) return bad("a job without a tracker");
    if (t->ctx != sel->ctx) return bad("the tracker belongs to another context");
    if (t->nlevels < 3) return bad("the tracker has fewer than 3 levels");
    if (t->w != sel->w || t->h != sel->h) return bad("the tracker's geometry is not the selector's");
    if (J.slot < 0 || J.slot > 1 || !t->have_frame[J.slot]) return bad("no frame in this tracker slot");
  }
  return DSM_OK;
}
} // namespace

extern "C" int dsm_select_pixels_batch(dsm_pixel_selector *sel, int n_jobs, const dsm_select_job *jobs, const dsm_select_params *params) {
  int rc = check_jobs(sel, n_jobs, jobs, params);
  if (rc) return rc;
  dsm_context *ctx = sel->ctx;
  const int w = sel->w, h = sel->h;
  const size_t wh = (size_t)w * h;
  const SelLayout &L = sel->L;
  const dsm_select_params S = *params;
  // staged [job table | the jobs' inverse responses], read back per job [header | point arrays | map if asked for]
  CallArena A;
  const size_t o_jobs = A.in.take(sizeof(SelJob) * n_jobs);
  std::vector<size_t> &o_binv = sel->o_binv, &o_out = sel->o_out, &o_map = sel->o_map;
  for (int j = 0; j < n_jobs; j++) {
    o_binv[j] = jobs[j].b_inv ? A.in.take(4 * 256) : 0;
    o_out[j] = A.out.take(4 * (kHeaderWords + (size_t)kPointWords * jobs[j].max_pts));
    o_map[j] = jobs[j].map_out ? A.out.take(wh) : 0;
  }
  if ((rc = A.bind(ctx))) return rc;
  SelJob *hj = A.host_in<SelJob>(o_jobs);
  for (int j = 0; j < n_jobs; j++) {
    const dsm_select_job &J = jobs[j];
    SelJob &D = hj[j];
    memset(&D, 0, sizeof D);
    float *const *img = J.tracker->d_img[J.slot];
    D.I0 = img[0], D.I1 = img[1], D.I2 = img[2];
    if (J.b_inv) memcpy(A.host_in<float>(o_binv[j]), J.b_inv, 4 * 256), D.b_inv = A.dev_in<const float>(o_binv[j]);
    D.scratch = sel->d_scratch + L.stride * j, D.atoms = sel->d_atoms + L.atom_stride * j;
    D.map_out = J.map_out ? A.dev_out<unsigned char>(o_map[j]) : nullptr;
    D.out = A.dev_out<unsigned>(o_out[j]);
    D.density = J.density, D.pot0 = *J.potential_io, D.max_pts = J.max_pts;
  }
  if ((rc = A.upload())) return rc;
  const SelJob *dj = A.dev_in<const SelJob>(o_jobs);
  hipStream_t st = ctx->stream;
  const unsigned nj = (unsigned)n_jobs, nb = (unsigned)((w / 32) * (h / 32)), px_blocks = (unsigned)((wh + 255) / 256);
  hipLaunchKernelGGL(select_hist_kernel, dim3(nb, nj), dim3(256), 0, st, dj, L, w, h, S);
  hipLaunchKernelGGL(select_smooth_kernel, dim3((nb + 63) / 64, nj), dim3(64), 0, st, dj, L, w, h);
  for (int pass = 0; pass <= S.recursions; pass++) { // P10 is decided on the device: a job that is done leaves every kernel at once
    DSM_HIP(hipMemsetAsync(sel->d_atoms, 0, L.atom_stride * n_jobs, st));
    hipLaunchKernelGGL(select_mask_kernel, dim3(px_blocks, nj), dim3(256), 0, st, dj, L, w, h, S);
    hipLaunchKernelGGL(select_chain_kernel, dim3(nj), dim3(64), 0, st, dj, L, w, h, (const unsigned char *)sel->d_rp);
    hipLaunchKernelGGL(select_key_kernel, dim3(px_blocks, nj), dim3(256), 0, st, dj, L, w, h, S);
    hipLaunchKernelGGL(select_resolve_kernel, dim3((unsigned)(L.ncell / 16 + 255) / 256, nj), dim3(256), 0, st, dj, L, w, h);
    hipLaunchKernelGGL(select_decide_kernel, dim3((nj + 63) / 64), dim3(64), 0, st, dj, n_jobs, S);
  }
  hipLaunchKernelGGL(select_rows_kernel, dim3((unsigned)h, nj), dim3(64), 0, st, dj, L, w, h);
  hipLaunchKernelGGL(select_thin_kernel, dim3((unsigned)h, nj), dim3(64), 0, st, dj, L, w, h, S, (const unsigned char *)sel->d_rp);
  hipLaunchKernelGGL(select_points_kernel, dim3((unsigned)h, nj), dim3(64), 0, st, dj, L, w, h, S);
  DSM_HIP(hipGetLastError());
  if ((rc = A.fetch(A.out.used))) return rc;
  for (int j = 0; j < n_jobs; j++) {
    const dsm_select_job &J = jobs[j];
    const int *hd = A.host_out<int>(o_out[j]);
    const float *q = A.host_out<float>(o_out[j]) + kHeaderWords;
    const size_t cap = (size_t)J.max_pts, n = std::min((size_t)hd[0], cap);
    if (n) {
      memcpy(J.u, q, 4 * n), memcpy(J.v, q + cap, 4 * n), memcpy(J.energy_th, q + 2 * cap, 4 * n), memcpy(J.grad_h, q + 3 * cap, 16 * n);
      memcpy(J.color, q + 7 * cap, 32 * n), memcpy(J.weights, q + 15 * cap, 32 * n), memcpy(J.type, q + 23 * cap, 4 * n);
    }
    for (size_t i = 0; i < n; i++) J.status[i] = DSM_IPS_UNINITIALIZED, J.idepth_min[i] = 0.f, J.idepth_max[i] = NAN, J.quality[i] = 10000.f;
    *J.n_pts_out = hd[0], *J.num_total_out = hd[1], *J.potential_io = hd[6];
    if (J.counts_out) memcpy(J.counts_out, hd + 2, 12);
    if (J.passes_out) *J.passes_out = hd[5];
    if (J.map_out) memcpy(J.map_out, A.host_out<unsigned char>(o_map[j]), wh);
  }
  return DSM_OK;
}
