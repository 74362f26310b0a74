// frame_kernels.hip -- the frame helpers of the hand-over and of the single-frame calls: makeImages' pyramids, the reference's
// (I, dx, dy) texels out of / into / against an intensity plane, the copy of page-locked caller rows, undistortion fused with level 0.
#include "dsm_kernels.hpp"

namespace dsm {

static inline int grid_for(int n, int block = 256) {
  int g = (n + block - 1) / block;
  return g < 1 ? 1 : (g > 2048 ? 2048 : g);
}

// ------------------------------------------------------------------------------------------
// makeImages (upstream DSO FrameHessian::makeImages; call sites FrontEnd.cpp:605,680)
// The device keeps the INTENSITY plane of every level only; the reference's (I, dx, dy) texels are formed where they are
// consumed (taps_interp) or handed back (dip_export_kernel).
// ------------------------------------------------------------------------------------------
// One launch per pyramid level l: the intensities of level l+1 are the 2x2 means 0.25 * (a + b + c + d) of level l.
// Level 0 also converts the camera image (float or "mono8" bytes, exactly) into the level-0 plane.
// The image fact (eval_facts.hpp): every pixel of a plane passes through a register here on its way into the plane, so the thread
// that writes it also tests it; a thread that wrote a failing pixel stores 0 into the level's armed word (plain_l for out_l,
// plain_next for out_next; null: no word kept).  Stores of the one value 0: order-independent.
template <typename SRC>
__device__ __forceinline__ void pyr_level_body(int wl, int hl, const SRC *__restrict__ src, float *__restrict__ out_l,
                                               float *__restrict__ out_next, int first, int step, int *plain_l, int *plain_next) {
  const int wn = wl >> 1, hn = hl >> 1;
  const int npx = out_l ? wl * hl : wn * hn;
  bool ok_l = true, ok_next = true;
  for (int idx = first; idx < npx; idx += step) {
    if (out_l) {
      const float v = (float)src[idx];
      out_l[idx] = v;
      ok_l = ok_l && pixel_plain(v);
    }
    if (out_next && idx < wn * hn) {
      const int x = idx % wn, y = idx / wn;
      const int b = 2 * x + 2 * y * wl;
      const float v = 0.25f * ((float)src[b] + (float)src[b + 1] + (float)src[b + wl] + (float)src[b + 1 + wl]);
      out_next[idx] = v;
      ok_next = ok_next && pixel_plain(v);
    }
  }
  if (!ok_l && plain_l) *plain_l = 0;
  if (!ok_next && plain_next) *plain_next = 0;
}
// out_l != nullptr: level 0 (src = the camera image); else src = the plane of level l
__global__ void pyr_level_fused_kernel(int wl, int hl, const float *__restrict__ src, float *__restrict__ out_l,
                                       float *__restrict__ out_next, int *plain_l, int *plain_next) {
  pyr_level_body<float>(wl, hl, src, out_l, out_next, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x, plain_l, plain_next);
}
// the same for a batch of images (dsm_upload_images): blockIdx.y = image; U8: the level-0 source holds camera bytes
// (main.cpp:216-217 "mono8"), converted exactly
template <bool U8>
__global__ void pyr_level_batched_kernel(int l, int nlevels, int wl, int hl, const PyrJob *__restrict__ jobs) {
  const PyrJob &j = jobs[blockIdx.y];
  float *out_next = l + 1 < nlevels ? j.img[l + 1] : nullptr;
  const int first = blockIdx.x * blockDim.x + threadIdx.x, step = gridDim.x * blockDim.x;
  int *const plain_l = j.plain ? j.plain + l : nullptr, *const plain_next = j.plain ? j.plain + l + 1 : nullptr;
  if (l == 0) {
    if (U8)
      pyr_level_body<unsigned char>(wl, hl, (const unsigned char *)j.raw, j.img[0], out_next, first, step, plain_l, plain_next);
    else
      pyr_level_body<float>(wl, hl, (const float *)j.raw, j.img[0], out_next, first, step, plain_l, plain_next);
  } else {
    pyr_level_body<float>(wl, hl, j.img[l], nullptr, out_next, first, step, nullptr, plain_next);
  }
}
// the first launch of a batched build: every job's words read 1 until a pixel fails
__global__ void pyr_facts_arm_kernel(const PyrJob *__restrict__ jobs, int njobs, int nlevels) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= njobs * nlevels) return;
  int *const plain = jobs[i / nlevels].plain;
  if (plain) plain[i % nlevels] = 1;
}
void launch_pyr_facts_arm(hipStream_t s, const PyrJob *d_jobs, int njobs, int nlevels) {
  if (njobs > 0) hipLaunchKernelGGL(pyr_facts_arm_kernel, dim3(grid_for(njobs * nlevels)), dim3(256), 0, s, d_jobs, njobs, nlevels);
}
// The reference's texels from / against an intensity plane.  Gradients: central differences on the flat index for
// idx in [w, w (h - 1)), zero elsewhere and where the difference is not finite (upstream DSO makeImages).
__device__ __forceinline__ void dip_gradients(const float *__restrict__ I, int w, int h, int idx, float &dx, float &dy) {
  dx = 0.f, dy = 0.f;
  if (idx >= w && idx < w * (h - 1)) {
    dx = 0.5f * (I[idx + 1] - I[idx - 1]);
    dy = 0.5f * (I[idx + w] - I[idx - w]);
    if (!__builtin_isfinite(dx)) dx = 0;
    if (!__builtin_isfinite(dy)) dy = 0;
  }
}
// dsm_tracker_get_frame: plane -> (I, dx, dy)
__global__ void dip_export_kernel(int w, int h, const float *__restrict__ I, float *__restrict__ out3) {
  for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < w * h; idx += gridDim.x * blockDim.x) {
    float dx, dy;
    dip_gradients(I, w, h, idx, dx, dy);
    out3[3 * idx] = I[idx];
    out3[3 * idx + 1] = dx;
    out3[3 * idx + 2] = dy;
  }
}
// dsm_tracker_upload_frame, step 1: (I, dx, dy) -> plane
__global__ void dip_import_kernel(int npx, const float *__restrict__ in3, float *__restrict__ I) {
  for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < npx; idx += gridDim.x * blockDim.x) I[idx] = in3[3 * idx];
}
// step 2: the caller's gradient channels must be what makeImages derives from channel 0 (they are not stored): count
// the texels of the rows makeImages fills whose dx or dy differs (bitwise, or by more than tol * max(1, |g|)) and keep the
// first of them: bad = {count, smallest index}
__global__ void dip_verify_kernel(int w, int h, const float *__restrict__ in3, const float *__restrict__ I, int *__restrict__ bad, float tol) {
  int mine = 0, first = 0x7FFFFFFF;
  for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < w * h; idx += gridDim.x * blockDim.x) {
    if (idx < w || idx >= w * (h - 1)) continue; // rows makeImages leaves untouched are never read by the tracker
    float dx, dy;
    dip_gradients(I, w, h, idx, dx, dy);
    const float gx = in3[3 * idx + 1], gy = in3[3 * idx + 2];
    bool off;
    if (tol > 0.0f)
      off = !(__builtin_fabsf(gx - dx) <= tol * __builtin_fmaxf(1.0f, __builtin_fabsf(dx))) || !(__builtin_fabsf(gy - dy) <= tol * __builtin_fmaxf(1.0f, __builtin_fabsf(dy)));
    else
      off = (__float_as_uint(dx) != __float_as_uint(gx)) || (__float_as_uint(dy) != __float_as_uint(gy));
    if (off) {
      mine++;
      if (idx < first) first = idx;
    }
  }
  if (mine) {
    atomicAdd(bad, mine);
    atomicMin(bad + 1, first);
  }
}
void launch_dip_export(hipStream_t s, int w, int h, const float *plane, float *out3) {
  hipLaunchKernelGGL(dip_export_kernel, dim3(grid_for(w * h)), dim3(256), 0, s, w, h, plane, out3);
}
void launch_dip_import(hipStream_t s, int w, int h, const float *in3, float *plane, int *d_bad, float tol) {
  hipLaunchKernelGGL(dip_import_kernel, dim3(grid_for(w * h)), dim3(256), 0, s, w * h, in3, plane);
  if (d_bad) hipLaunchKernelGGL(dip_verify_kernel, dim3(grid_for(w * h)), dim3(256), 0, s, w, h, in3, plane, d_bad, tol);
}
// Pinned caller images are fetched by the GPU itself (one launch for the whole batch instead of one copy command per
// image): every thread moves UNIT bytes per access straight from host memory.
typedef unsigned copy_uvec4 __attribute__((ext_vector_type(4)));
template <typename UNIT>
__global__ void host_rows_copy_kernel(const PyrJob *__restrict__ jobs, int njobs, int row_units, int rows, size_t pitch_units) {
  // one grid-stride loop over all images: a small grid (asynchronous hand-over) keeps the slow host reads on a few CUs
  const long long per = (long long)row_units * rows, total = per * njobs;
  for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (long long)gridDim.x * blockDim.x) {
    const int job = (int)(g / per), idx = (int)(g - (long long)job * per);
    const int r = idx / row_units, c = idx - r * row_units;
    const PyrJob &j = jobs[job];
    ((UNIT *)j.raw)[idx] = __builtin_nontemporal_load((const UNIT *)j.src + (size_t)r * pitch_units + c);
  }
}
void launch_host_rows_copy(hipStream_t s, const PyrJob *d_jobs, int njobs, int row_bytes, int rows, size_t pitch, int unit, int max_blocks) {
  const int row_units = row_bytes / unit;
  long long blocks = ((long long)row_units * rows * njobs + 255) / 256;
  if (blocks > max_blocks) blocks = max_blocks;
  const dim3 grid((unsigned)blocks);
  if (unit == 16)
    hipLaunchKernelGGL(host_rows_copy_kernel<copy_uvec4>, grid, dim3(256), 0, s, d_jobs, njobs, row_units, rows, pitch / 16);
  else if (unit == 4)
    hipLaunchKernelGGL(host_rows_copy_kernel<unsigned>, grid, dim3(256), 0, s, d_jobs, njobs, row_units, rows, pitch / 4);
  else
    hipLaunchKernelGGL(host_rows_copy_kernel<unsigned char>, grid, dim3(256), 0, s, d_jobs, njobs, row_units, rows, pitch);
}
// raw: the level-0 float image; img[l]: the intensity planes of the pyramid levels
void launch_pyramid(hipStream_t s, int w, int h, int nlevels, const float *raw, float *const *img, int *plain) {
  for (int l = 0; l < nlevels; l++) {
    const int wl = w >> l, hl = h >> l;
    if (l > 0 && l + 1 >= nlevels) break; // the coarsest level has nothing to produce
    hipLaunchKernelGGL(pyr_level_fused_kernel, dim3(grid_for(l == 0 ? wl * hl : (wl >> 1) * (hl >> 1))), dim3(256), 0, s, wl, hl,
                       l == 0 ? raw : img[l], l == 0 ? img[0] : nullptr, l + 1 < nlevels ? img[l + 1] : nullptr,
                       plain && l == 0 ? plain : nullptr, plain && l + 1 < nlevels ? plain + l + 1 : nullptr);
  }
}
void launch_pyramid_batched(hipStream_t s, int w, int h, int nlevels, const PyrJob *d_jobs, int njobs, bool u8) {
  launch_pyr_facts_arm(s, d_jobs, njobs, nlevels);
  for (int l = 0; l < nlevels; l++) {
    const int wl = w >> l, hl = h >> l;
    if (l > 0 && l + 1 >= nlevels) break;
    const dim3 grid(grid_for(l == 0 ? wl * hl : (wl >> 1) * (hl >> 1)), njobs);
    if (u8)
      hipLaunchKernelGGL(pyr_level_batched_kernel<true>, grid, dim3(256), 0, s, l, nlevels, wl, hl, d_jobs);
    else
      hipLaunchKernelGGL(pyr_level_batched_kernel<false>, grid, dim3(256), 0, s, l, nlevels, wl, hl, d_jobs);
  }
}

// ------------------------------------------------------------------------------------------
// dsm_upload_images_undistorted: UPSTREAM-DSO Undistort::undistort<unsigned char>(img, 1, 0, 1.0f) (main.cpp:246-256) fused
// with makeImages' level 0 -> 1.  blockIdx.y = image; every thread produces one 2x2 quad of level 0 and, from those four
// values, its level-1 texel (0.25 ((a + b) + c) + d) as pyr_level_body forms it.  The 2x2 taps come from the staged camera
// bytes (neighbouring outputs share them: L2 / MALL); the remap entries are read as 8-byte (x, y) pairs.  dsm_undistorter_create
// checked every entry: x < 0, or the whole footprint inside the w_in x h_in source.
// ------------------------------------------------------------------------------------------
// PhotometricUndistorter::processFrame: G[byte] (setting_photometricCalibration >= 1) else factor * byte with factor 1;
// then times vignetteMapInv (== 2)
template <bool HAS_G, bool HAS_VIG>
__device__ __forceinline__ float photometric(const unsigned char *__restrict__ raw, const float *__restrict__ Gs,
                                             const float *__restrict__ vig, int i) {
  float p = HAS_G ? Gs[raw[i]] : (float)raw[i];
  if (HAS_VIG) p *= vig[i];
  return p;
}
template <bool HAS_G, bool HAS_VIG, bool REMAP>
__device__ __forceinline__ float undistort_px(const UndistortTables &u, const unsigned char *__restrict__ raw, const float *__restrict__ Gs,
                                              int idx) {
  if (!REMAP) return photometric<HAS_G, HAS_VIG>(raw, Gs, u.vig, idx); // passthrough: w_out == w_in
  const float2 r = u.remap[idx];
  if (r.x < 0) return 0.f;
  const int xi = (int)r.x, yi = (int)r.y;
  const float ax = r.x - xi, ay = r.y - yi, axy = ax * ay;
  const int b = xi + yi * u.w_in;
  const float s00 = photometric<HAS_G, HAS_VIG>(raw, Gs, u.vig, b), s10 = photometric<HAS_G, HAS_VIG>(raw, Gs, u.vig, b + 1);
  const float s01 = photometric<HAS_G, HAS_VIG>(raw, Gs, u.vig, b + u.w_in), s11 = photometric<HAS_G, HAS_VIG>(raw, Gs, u.vig, b + 1 + u.w_in);
  return axy * s11 + (ay - axy) * s01 + (ax - axy) * s10 + (1 - ax - ay + axy) * s00;
}
template <bool HAS_G, bool HAS_VIG, bool REMAP>
__global__ __launch_bounds__(256) void undistort_pyr_kernel(UndistortTables u, int nlevels, const PyrJob *__restrict__ jobs) {
  __shared__ float Gs[256];
  if (HAS_G) {
    Gs[threadIdx.x] = u.G[threadIdx.x]; // blockDim.x == 256
    __syncthreads();
  }
  const PyrJob &j = jobs[blockIdx.y];
  const unsigned char *raw = (const unsigned char *)j.raw;
  float *out0 = j.img[0], *out1 = nlevels > 1 ? j.img[1] : nullptr;
  const int w = u.w_out, h = u.h_out, wq = (w + 1) >> 1, hq = (h + 1) >> 1, wn = w >> 1, hn = h >> 1;
  bool ok0 = true, ok1 = true; // the image fact of levels 0 and 1, as pyr_level_body keeps it
  for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < wq * hq; q += gridDim.x * blockDim.x) {
    const int qx = q % wq, qy = q / wq, x = 2 * qx, y = 2 * qy, i = x + y * w;
    const bool right = x + 1 < w, below = y + 1 < h;
    const float a = undistort_px<HAS_G, HAS_VIG, REMAP>(u, raw, Gs, i);
    const float b = right ? undistort_px<HAS_G, HAS_VIG, REMAP>(u, raw, Gs, i + 1) : 0.f;
    const float c = below ? undistort_px<HAS_G, HAS_VIG, REMAP>(u, raw, Gs, i + w) : 0.f;
    const float d = right && below ? undistort_px<HAS_G, HAS_VIG, REMAP>(u, raw, Gs, i + w + 1) : 0.f;
    out0[i] = a;
    if (right) out0[i + 1] = b;
    if (below) out0[i + w] = c;
    if (right && below) out0[i + w + 1] = d;
    ok0 = ok0 && pixel_plain(a) && pixel_plain(b) && pixel_plain(c) && pixel_plain(d); // (an absent neighbour is 0)
    if (out1 && qx < wn && qy < hn) {
      const float v = 0.25f * (a + b + c + d);
      out1[qx + qy * wn] = v;
      ok1 = ok1 && pixel_plain(v);
    }
  }
  if (!ok0 && j.plain) j.plain[0] = 0;
  if (!ok1 && j.plain) j.plain[1] = 0;
}
template <bool HAS_G, bool HAS_VIG>
static void launch_undistort_l0(hipStream_t s, const UndistortTables &u, int nlevels, const PyrJob *d_jobs, const dim3 &grid) {
  if (u.remap)
    hipLaunchKernelGGL((undistort_pyr_kernel<HAS_G, HAS_VIG, true>), grid, dim3(256), 0, s, u, nlevels, d_jobs);
  else
    hipLaunchKernelGGL((undistort_pyr_kernel<HAS_G, HAS_VIG, false>), grid, dim3(256), 0, s, u, nlevels, d_jobs);
}
void launch_undistort_pyramid_batched(hipStream_t s, const UndistortTables &u, int nlevels, const PyrJob *d_jobs, int njobs) {
  launch_pyr_facts_arm(s, d_jobs, njobs, nlevels);
  const dim3 grid0(grid_for(((u.w_out + 1) >> 1) * ((u.h_out + 1) >> 1)), njobs);
  if (u.G && u.vig)
    launch_undistort_l0<true, true>(s, u, nlevels, d_jobs, grid0);
  else if (u.G)
    launch_undistort_l0<true, false>(s, u, nlevels, d_jobs, grid0);
  else if (u.vig)
    launch_undistort_l0<false, true>(s, u, nlevels, d_jobs, grid0);
  else
    launch_undistort_l0<false, false>(s, u, nlevels, d_jobs, grid0);
  // levels >= 1: launch_pyramid_batched's launches l = 1 .. nlevels - 2
  for (int l = 1; l + 1 < nlevels; l++) {
    const int wl = u.w_out >> l, hl = u.h_out >> l;
    const dim3 grid(grid_for((wl >> 1) * (hl >> 1)), njobs);
    hipLaunchKernelGGL(pyr_level_batched_kernel<false>, grid, dim3(256), 0, s, l, nlevels, wl, hl, d_jobs);
  }
}

} // namespace dsm
