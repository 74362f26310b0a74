// template_kernels.hip -- row A4 / N3 on the device: TrackerAndScaler::makeCoarseDepthL0
// (TrackerAndScaler.cpp:143-315) from flat arrays of the window's active points straight into the
// tracker's float4 template, without the per-keyframe host loops and the host->device upload of the
// template lists.  Every float operation is the reference's, in the reference's order:
//   * points that splat onto the same pixel are summed in point order (:149-164) -- per-pixel lists
//     are linked with an atomic exchange (order irrelevant) and then walked in ascending point index;
//   * 2x2 sums (:166-187) and the 4-neighbour dilation (:190-275) are element-wise; the dilation reads
//     the pre-dilation weights (the reference's _bak copy) and only pre-dilation depths of pixels it
//     never writes, so a two-buffer form is identical to the in-place loop;
//   * the emit loop (:278-314) is an ordered stream compaction over the interior pixels in row-major
//     order (block counts -> exclusive scan -> ordered writes), so the template order -- and with it
//     the chunking and every reduction of the eval kernels -- equals the reference's emit order.
// The idepth_/weight_sums_ side products (only read by debugPlotIDepthMap) are not kept.
// At the end: the template helpers of dsm_tracker_set_ref / _get_template (interleave, de-interleave) and scaleCoarseDepthL0.
#include "dsm_kernels.hpp"

namespace dsm {

// One job = one keyframe's template (dsm_set_refs_from_points builds the templates of every sequence that made a keyframe in the same
// advance with ONE launch sequence: blockIdx.y = job; a per-job launch sequence was 26 launches x the jobs of a call, 1.1 of the 1.9 ms a
// node serving 128 sequences spent between two advances).  All jobs of a call share w, h and the level count.
struct TplView { // the pieces of a job's workspace (TplJob::ws), as launch_make_coarse_depth lays them out
  const float *pu, *pv, *pid, *pw;
  int *next, *head;
  float *idA, *wsA, *idB, *wsB;
  int *block_count;
};
__device__ __forceinline__ TplView tpl_view(const TplJob &J, int w, int h, int px_total) {
  TplView V;
  V.pu = J.pt, V.pv = V.pu + J.npts, V.pid = V.pv + J.npts, V.pw = V.pid + J.npts;
  V.next = (int *)J.ws;
  V.head = V.next + J.npts;
  V.idA = (float *)(V.head + (size_t)w * h);
  V.wsA = V.idA + px_total, V.idB = V.wsA + px_total, V.wsB = V.idB + px_total;
  V.block_count = (int *)(V.wsB + px_total);
  return V;
}

__global__ void tpl_init_kernel(const TplJob *__restrict__ jobs, int w, int h, int nlevels, int px_total) {
  const TplJob J = jobs[blockIdx.y];
  const TplView V = tpl_view(J, w, h, px_total);
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p < w * h) V.head[p] = -1;
  if (p <= nlevels) J.d_n[p] = 0;
}

__global__ void tpl_splat_link_kernel(const TplJob *__restrict__ jobs, int w, int h, int nlevels, int px_total) {
  const TplJob J = jobs[blockIdx.y];
  const TplView V = tpl_view(J, w, h, px_total);
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= J.npts) return;
  const float fu = V.pu[k] + 0.5f, fv = V.pv[k] + 0.5f; // :151-152
  // accepted: fu and fv finite and truncating (toward zero) into [0, w) x [0, h), i.e. -1 < f < size.  Tested on the floats, every
  // comparison false for a NaN: the float -> int conversion of a NaN or of a value outside int is not defined (here it gave 0 for NaN).
  if (!(fu > -1.0f && fu < (float)w && fv > -1.0f && fv < (float)h)) { // the reference would write out of bounds
    atomicOr(J.d_n + nlevels, 1);
    V.next[k] = -2;
    return;
  }
  const int u = (int)fu, v = (int)fv;
  V.next[k] = atomicExch(&V.head[u + w * v], k);
}

// one thread per level-0 pixel: sum this pixel's points in ascending point index (:160-161)
__global__ void tpl_splat_sum_kernel(const TplJob *__restrict__ jobs, int w, int h, int px_total) {
  const TplJob J = jobs[blockIdx.y];
  const TplView V = tpl_view(J, w, h, px_total);
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= w * h) return;
  float sid = 0.f, sw = 0.f;
  const int hd = V.head[p];
  int last = -1;
  while (hd >= 0) {
    int best = 0x7FFFFFFF;
    for (int j = hd; j >= 0; j = V.next[j])
      if (j > last && j < best) best = j;
    if (best == 0x7FFFFFFF) break;
    sid += V.pid[best] * V.pw[best];
    sw += V.pw[best];
    last = best;
  }
  V.idA[p] = sid;
  V.wsA[p] = sw;
}

__global__ void tpl_pyr_sum_kernel(const TplJob *__restrict__ jobs, int w, int h, int px_total, int wl, int hl, int wlm1, int prev, int off) {
  const TplView V = tpl_view(jobs[blockIdx.y], w, h, px_total);
  const float *idm = V.idA + prev, *wsm = V.wsA + prev;
  float *idl = V.idA + off, *wsl = V.wsA + off;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= wl * hl) return;
  const int x = i % wl, y = i / wl;
  const int b = 2 * x + 2 * y * wlm1;
  idl[i] = idm[b] + idm[b + 1] + idm[b + wlm1] + idm[b + wlm1 + 1];
  wsl[i] = wsm[b] + wsm[b + 1] + wsm[b + wlm1] + wsm[b + wlm1 + 1];
}

// :190-233 (levels 0-1, diagonal neighbours) / :236-275 (levels >= 2, axis neighbours)
__global__ void tpl_dilate_kernel(const TplJob *__restrict__ jobs, int w, int h, int px_total, int wl, int hl, int diagonal, int off) {
  const TplView V = tpl_view(jobs[blockIdx.y], w, h, px_total);
  const float *idl_in = V.idA + off, *bak = V.wsA + off;
  float *idl_out = V.idB + off, *ws_out = V.wsB + off;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int npix = wl * hl;
  if (i >= npix) return;
  float id = idl_in[i], ws = bak[i];
  if (i >= wl && i < npix - wl && ws <= 0) {
    const int o0 = diagonal ? 1 + wl : 1, o1 = diagonal ? -1 - wl : -1, o2 = diagonal ? wl - 1 : wl, o3 = diagonal ? -wl + 1 : -wl;
    const int offs[4] = {o0, o1, o2, o3};
    float sum = 0, num = 0, numn = 0;
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (bak[i + offs[k]] > 0) {
        sum += idl_in[i + offs[k]];
        num += bak[i + offs[k]];
        numn++;
      }
    if (numn > 0) {
      id = sum / numn;
      ws = num / numn;
    }
  }
  idl_out[i] = id;
  ws_out[i] = ws;
}

constexpr int kEmitThreads = 256, kEmitItems = 4, kEmitBlock = kEmitThreads * kEmitItems;

// the emit test of one interior item (:291-307); returns the template entry in `e`
__device__ __forceinline__ bool tpl_emit_item(int item, int wi, int wl, const float *idl, const float *ws, const float *ref,
                                              int texel_floats, float4 &e) {
  const int x = 2 + item % wi, y = 2 + item / wi;
  const int i = x + y * wl;
  const float wsum = ws[i];
  if (!(wsum > 0)) return false;
  const float id = idl[i] / wsum;
  const float color = ref[(size_t)texel_floats * i];
  e = make_float4((float)x, (float)y, id, color);
  return __builtin_isfinite(color) && id > 0;
}

__global__ __launch_bounds__(kEmitThreads) void tpl_emit_count_kernel(const TplJob *__restrict__ jobs, int w, int h, int px_total, int lvl,
                                                                      int nitems, int wi, int wl, int off, int texel_floats) {
  const TplJob J = jobs[blockIdx.y];
  const TplView V = tpl_view(J, w, h, px_total);
  const float *idl = V.idB + off, *ws = V.wsB + off, *ref = J.ref[lvl];
  __shared__ int wave_cnt[kEmitThreads / 64];
  const int base = blockIdx.x * kEmitBlock;
  int c = 0;
  for (int j = 0; j < kEmitItems; j++) {
    const int item = base + j * kEmitThreads + threadIdx.x;
    float4 e;
    const bool v = item < nitems && tpl_emit_item(item, wi, wl, idl, ws, ref, texel_floats, e);
    c += __builtin_popcountll(__ballot(v));
  }
  if ((threadIdx.x & 63) == 0) wave_cnt[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) V.block_count[blockIdx.x] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
}

// exclusive scan of the block counts by one workgroup per job (<= 1024 counts per pass, carried), total -> d_n[lvl]
__global__ __launch_bounds__(1024) void tpl_emit_scan_kernel(const TplJob *__restrict__ jobs, int w, int h, int px_total, int lvl, int nblocks) {
  const TplJob J = jobs[blockIdx.y];
  int *block_count = tpl_view(J, w, h, px_total).block_count;
  __shared__ int s[1024];
  __shared__ int carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (int b0 = 0; b0 < nblocks; b0 += 1024) {
    const int i = b0 + threadIdx.x;
    const int v = i < nblocks ? block_count[i] : 0;
    s[threadIdx.x] = v;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) { // Hillis-Steele inclusive scan (integers: order is immaterial)
      const int t = threadIdx.x >= d ? s[threadIdx.x - d] : 0;
      __syncthreads();
      s[threadIdx.x] += t;
      __syncthreads();
    }
    if (i < nblocks) block_count[i] = carry + s[threadIdx.x] - v;
    __syncthreads();
    if (threadIdx.x == 1023) carry += s[1023];
    __syncthreads();
  }
  if (threadIdx.x == 0) J.d_n[lvl] = carry;
}

// The template fact (eval_facts.hpp) of the entries a thread writes, kept where the entry is in registers: note() per written entry,
// commit() once at the end of the kernel by EVERY thread of the workgroup (full waves, at most 1024 threads: it exchanges across the
// wave, then across the waves through LDS behind a barrier).  The flag is stored as 0 on failure into the armed word; the bounds tighten
// by integer atomics on order-preserving keys: exact, whatever the order of arrival.  One thread per workgroup issues them, and only
// where its value would move the bound it reads (a bound only ever tightens, so a value that does not beat what is read -- however
// stale -- cannot beat the final one either): without both, a level-0 list's 7 k waves queued 37 k atomics on one cache line, 95 us
// for a 4 us kernel.  F null (workgroup-uniform): nothing is kept.
struct EntryFacts {
  bool ok = true;
  int x0 = kKeyMinInit, x1 = kKeyMaxInit, y0 = kKeyMinInit, y1 = kKeyMaxInit, id1 = kKeyMaxInit;
  __device__ __forceinline__ void note(float x, float y, float id) {
    ok = ok && entry_plain(x, y, id);
    const int kx = ordered_key(x), ky = ordered_key(y), ki = ordered_key(id);
    x0 = kx < x0 ? kx : x0, x1 = kx > x1 ? kx : x1, y0 = ky < y0 ? ky : y0, y1 = ky > y1 ? ky : y1, id1 = ki > id1 ? ki : id1;
  }
  __device__ __forceinline__ void commit(LevelFacts *F) {
    if (!F) return;
    __shared__ int part[16][6]; // per wave: {failed, x0, x1, y0, y1, id1}
    const int bad = __any(!ok) ? 1 : 0;
    for (int d = 32; d >= 1; d >>= 1) {
      const int a0 = __shfl_xor(x0, d), a1 = __shfl_xor(x1, d), b0 = __shfl_xor(y0, d), b1 = __shfl_xor(y1, d), c1 = __shfl_xor(id1, d);
      x0 = a0 < x0 ? a0 : x0, x1 = a1 > x1 ? a1 : x1, y0 = b0 < y0 ? b0 : y0, y1 = b1 > y1 ? b1 : y1, id1 = c1 > id1 ? c1 : id1;
    }
    const int wave = threadIdx.x >> 6, nwaves = (blockDim.x + 63) >> 6;
    if ((threadIdx.x & 63) == 0) part[wave][0] = bad, part[wave][1] = x0, part[wave][2] = x1, part[wave][3] = y0, part[wave][4] = y1, part[wave][5] = id1;
    __syncthreads();
    if (threadIdx.x != 0) return;
    int any_bad = 0;
    for (int w = 0; w < nwaves; w++) {
      any_bad |= part[w][0];
      x0 = part[w][1] < x0 ? part[w][1] : x0, x1 = part[w][2] > x1 ? part[w][2] : x1;
      y0 = part[w][3] < y0 ? part[w][3] : y0, y1 = part[w][4] > y1 ? part[w][4] : y1, id1 = part[w][5] > id1 ? part[w][5] : id1;
    }
    if (any_bad) F->tpl_plain = 0;
    if (x0 <= x1) { // the workgroup wrote an entry
      const volatile LevelFacts *R = F;
      if (x0 < R->xmin) atomicMin(&F->xmin, x0);
      if (x1 > R->xmax) atomicMax(&F->xmax, x1);
      if (y0 < R->ymin) atomicMin(&F->ymin, y0);
      if (y1 > R->ymax) atomicMax(&F->ymax, y1);
      if (id1 > R->idmax) atomicMax(&F->idmax, id1);
    }
  }
};

__global__ __launch_bounds__(kEmitThreads) void tpl_emit_write_kernel(const TplJob *__restrict__ jobs, int w, int h, int px_total, int lvl,
                                                                      int nitems, int wi, int wl, int off, int texel_floats) {
  const TplJob J = jobs[blockIdx.y];
  const TplView V = tpl_view(J, w, h, px_total);
  const float *idl = V.idB + off, *ws = V.wsB + off, *ref = J.ref[lvl];
  const int *block_offset = V.block_count;
  float4 *pts = J.pts[lvl];
  __shared__ int wave_cnt[kEmitItems][kEmitThreads / 64];
  const int base = blockIdx.x * kEmitBlock;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float4 e[kEmitItems];
  bool v[kEmitItems];
  int before[kEmitItems]; // valid items before this lane inside its wave, for pass j
#pragma unroll
  for (int j = 0; j < kEmitItems; j++) {
    const int item = base + j * kEmitThreads + threadIdx.x;
    v[j] = item < nitems && tpl_emit_item(item, wi, wl, idl, ws, ref, texel_floats, e[j]);
    const unsigned long long m = __ballot(v[j]);
    before[j] = __builtin_popcountll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wave_cnt[j][wave] = __builtin_popcountll(m);
  }
  __syncthreads();
  int pos = block_offset[blockIdx.x];
  EntryFacts ef;
#pragma unroll
  for (int j = 0; j < kEmitItems; j++) {
    int off2 = pos;
    for (int w2 = 0; w2 < wave; w2++) off2 += wave_cnt[j][w2];
    if (v[j]) pts[off2 + before[j]] = e[j], ef.note(e[j].x, e[j].y, e[j].z);
    pos += wave_cnt[j][0] + wave_cnt[j][1] + wave_cnt[j][2] + wave_cnt[j][3];
  }
  ef.commit(J.facts ? J.facts + lvl : nullptr);
}

// floats of a job's workspace (everything but its points, which live in the call's point region)
size_t make_coarse_depth_workspace_floats(int w, int h, int nlevels, int npts) {
  size_t px = 0;
  for (int l = 0; l < nlevels; l++) px += (size_t)(w >> l) * (h >> l);
  const size_t blocks = ((size_t)w * h + kEmitBlock - 1) / kEmitBlock + 1;
  return 4 * px + (size_t)w * h + (size_t)npts + blocks + 64;
}

// jobs: device table of njobs entries (ws = make_coarse_depth_workspace_floats() floats each; pt = [pu | pv | pidepth | pweight], npts
// each, on the device; ref[l] = the keyframe's pyramid level l (texel_floats = kTexel: the intensity plane); pts[l] = the float4
// template buffers; d_n = nlevels + 1 ints: n per level, then the out-of-bounds flag).  max_npts = the largest npts of the table.
void launch_make_coarse_depth(hipStream_t s, int w, int h, int nlevels, const TplJob *jobs, int njobs, int max_npts, int texel_floats) {
  if (njobs <= 0) return;
  int px = 0;
  for (int l = 0; l < nlevels; l++) px += (w >> l) * (h >> l);
  const unsigned J = (unsigned)njobs;
  hipLaunchKernelGGL(tpl_init_kernel, dim3((w * h + 255) / 256, J), dim3(256), 0, s, jobs, w, h, nlevels, px);
  if (max_npts > 0) hipLaunchKernelGGL(tpl_splat_link_kernel, dim3((max_npts + 255) / 256, J), dim3(256), 0, s, jobs, w, h, nlevels, px);
  hipLaunchKernelGGL(tpl_splat_sum_kernel, dim3((w * h + 255) / 256, J), dim3(256), 0, s, jobs, w, h, px);
  int off = 0;
  for (int l = 1; l < nlevels; l++) {
    const int prev = off;
    off += (w >> (l - 1)) * (h >> (l - 1));
    const int wl = w >> l, hl = h >> l;
    hipLaunchKernelGGL(tpl_pyr_sum_kernel, dim3((wl * hl + 255) / 256, J), dim3(256), 0, s, jobs, w, h, px, wl, hl, w >> (l - 1), prev, off);
  }
  off = 0;
  for (int l = 0; l < nlevels; l++) {
    const int wl = w >> l, hl = h >> l;
    hipLaunchKernelGGL(tpl_dilate_kernel, dim3((wl * hl + 255) / 256, J), dim3(256), 0, s, jobs, w, h, px, wl, hl, l < 2 ? 1 : 0, off);
    const int wi = wl - 4, hi = hl - 4;
    const int nitems = wi > 0 && hi > 0 ? wi * hi : 0;
    if (nitems > 0) {
      const int nblocks = (nitems + kEmitBlock - 1) / kEmitBlock;
      hipLaunchKernelGGL(tpl_emit_count_kernel, dim3(nblocks, J), dim3(kEmitThreads), 0, s, jobs, w, h, px, l, nitems, wi, wl, off, texel_floats);
      hipLaunchKernelGGL(tpl_emit_scan_kernel, dim3(1, J), dim3(1024), 0, s, jobs, w, h, px, l, nblocks);
      hipLaunchKernelGGL(tpl_emit_write_kernel, dim3(nblocks, J), dim3(kEmitThreads), 0, s, jobs, w, h, px, l, nitems, wi, wl, off, texel_floats);
    }
    off += wl * hl;
  }
}

// ------------------------------------------------------------------------------------------
// template helpers
// ------------------------------------------------------------------------------------------
__global__ void interleave_kernel(int n, const float *__restrict__ u, const float *__restrict__ v,
                                  const float *__restrict__ id, const float *__restrict__ c,
                                  float4 *__restrict__ out, LevelFacts *facts) {
  EntryFacts ef;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const float4 e = make_float4(u[i], v[i], id[i], c[i]);
    out[i] = e;
    ef.note(e.x, e.y, e.z);
  }
  ef.commit(facts);
}
// the words behind dsm_tracker::announce_template_write / announce_plane_write (one thread)
__global__ void facts_set_kernel(TrackerFacts *f, int tpl_levels, int img_set, int img_levels, int value) {
  for (int l = 0; l < kFactLevels; l++) {
    if (tpl_levels >> l & 1) {
      LevelFacts &L = f->lv[l];
      L.tpl_plain = value;
      L.xmin = L.ymin = kKeyMinInit, L.xmax = L.ymax = L.idmax = kKeyMaxInit;
    }
    if (img_set >= 0 && (img_levels >> l & 1)) f->img_plain[img_set][l] = value;
  }
}
void launch_facts_set(hipStream_t s, TrackerFacts *f, int tpl_levels, int img_set, int img_levels, int value) {
  if (f) hipLaunchKernelGGL(facts_set_kernel, dim3(1), dim3(1), 0, s, f, tpl_levels, img_set < kFactImageSets ? img_set : -1, img_levels, value);
}
__global__ void deinterleave_kernel(int n, const float4 *__restrict__ in, float *u, float *v, float *id,
                                    float *c) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const float4 p = in[i];
    u[i] = p.x;
    v[i] = p.y;
    id[i] = p.z;
    c[i] = p.w;
  }
}
// scaleCoarseDepthL0 (:329-336): lpc_idepth[p] /= scale
__global__ void scale_depth_kernel(int n, float4 *pts, float scale) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) pts[i].z = pts[i].z / scale;
}
static inline int grid_for(int n, int block = 256) {
  int g = (n + block - 1) / block;
  return g < 1 ? 1 : (g > 2048 ? 2048 : g);
}

void launch_interleave_template(hipStream_t s, int n, const float *u, const float *v, const float *id,
                                const float *c, float4 *out, LevelFacts *facts) {
  if (n > 0) hipLaunchKernelGGL(interleave_kernel, dim3(grid_for(n)), dim3(256), 0, s, n, u, v, id, c, out, facts);
}
void launch_deinterleave_template(hipStream_t s, int n, const float4 *in, float *u, float *v, float *id,
                                  float *c) {
  if (n > 0) hipLaunchKernelGGL(deinterleave_kernel, dim3(grid_for(n)), dim3(256), 0, s, n, in, u, v, id, c);
}
void launch_scale_depth(hipStream_t s, int n, float4 *pts, float scale) {
  if (n > 0) hipLaunchKernelGGL(scale_depth_kernel, dim3(grid_for(n)), dim3(256), 0, s, n, pts, scale);
}
__global__ void scale_depth_levels_kernel(ScaleDepthArgs a, float scale) {
  const int l = blockIdx.y, n = a.n[l];
  float4 *pts = a.pts[l];
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) pts[i].z = pts[i].z / scale; // (:333, as scale_depth_kernel)
}
void launch_scale_depth_levels(hipStream_t s, const ScaleDepthArgs &a, int max_n, float scale) {
  if (max_n > 0) hipLaunchKernelGGL(scale_depth_levels_kernel, dim3(grid_for(max_n), a.nlevels), dim3(256), 0, s, a, scale);
}

} // namespace dsm
