// pose_batch_kernels.hip -- set-up kernels of dsm_pose_estimate_batch (row N2 batched: PoseEstimator::estimate of many ScanContext
// matches in one call).  Two streaming kernels, each one launch over every job of the call (or of a wave of it):
//   pose_pack_kernel   the jobs' double points and per-level float colours -> the float4 templates (x, y, z, refColor[lvl]) of every level
//   pose_import_kernel the jobs' (I, dx, dy) pyramids -> intensity planes, with the makeImages gradient check of dsm_tracker_upload_frame
// Neither does arithmetic beyond the narrowing `(float)` of PoseEstimator.cpp:183-185 and the central differences of the check, so
// the templates and planes hold the bits the single call's interleave_kernel / dip_import_kernel / dip_verify_kernel produce.
#include "dsm_kernels.hpp"

namespace dsm {

// blockIdx.y = job; a thread owns point i of the job on EVERY level: the three doubles are read once (24 B per lane, a wave's 1536 B
// contiguous), each level's colour is one coalesced 4-byte load and each level's template entry one coalesced 16-byte store.
// Entries [n, n + kTemplatePad) are the zeroed slack the evaluation's prefetch may touch.
__global__ __launch_bounds__(256) void pose_pack_kernel(const PosePackJob *__restrict__ jobs, int nlevels) {
  const PosePackJob &J = jobs[blockIdx.y];
  const int n = J.n, total = n + kTemplatePad;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    float x = 0.f, y = 0.f, z = 0.f;
    const bool live = i < n;
    if (live) { // `float x = pts_[i].first(0)` ..., PoseEstimator.cpp:183-185
      x = (float)J.xyz[3 * (size_t)i];
      y = (float)J.xyz[3 * (size_t)i + 1];
      z = (float)J.xyz[3 * (size_t)i + 2];
    }
#pragma unroll
    for (int l = 0; l < DSM_MAX_LEVELS; l++)
      if (l < nlevels) J.pts[l][i] = make_float4(x, y, z, live ? J.col[l][i] : 0.f);
  }
}

void launch_pose_pack(hipStream_t s, const PosePackJob *d_jobs, int njobs, int nlevels, int max_n) {
  if (njobs <= 0) return;
  int gx = (max_n + kTemplatePad + 255) / 256;
  if (gx > 256) gx = 256;
  hipLaunchKernelGGL(pose_pack_kernel, dim3(gx, njobs), dim3(256), 0, s, d_jobs, nlevels);
}

// One texel of the check of dip_verify_kernel against the staged texels themselves (channel 0 of in3 IS the plane being written):
// dx, dy as dip_gradients forms them.
__device__ __forceinline__ bool pose_texel_off(const float *__restrict__ in3, int w, int idx, float left, float right, float gx, float gy, float tol) {
  float dx = 0.5f * (right - left);
  float dy = 0.5f * (in3[3 * (size_t)(idx + w)] - in3[3 * (size_t)(idx - w)]);
  if (!__builtin_isfinite(dx)) dx = 0;
  if (!__builtin_isfinite(dy)) dy = 0;
  if (tol > 0.0f)
    return !(__builtin_fabsf(gx - dx) <= tol * __builtin_fmaxf(1.0f, __builtin_fabsf(dx))) ||
           !(__builtin_fabsf(gy - dy) <= tol * __builtin_fmaxf(1.0f, __builtin_fabsf(dy)));
  return (__float_as_uint(dx) != __float_as_uint(gx)) || (__float_as_uint(dy) != __float_as_uint(gy));
}

// blockIdx.z = job of the wave, blockIdx.y = level.  A thread owns FOUR consecutive texels: three 16-byte loads of the staged
// (I, dx, dy) texels, one 16-byte store of the plane.  The check's horizontal neighbours come from the registers (the two outer
// ones and the rows above and below: 4-byte loads of lines other threads stream anyway).  bad = [level]{count, smallest index}.
__global__ __launch_bounds__(256) void pose_import_kernel(const PoseImportJob *__restrict__ jobs, int w0, int h0, int check, float tol) {
  const PoseImportJob &J = jobs[blockIdx.z];
  const int l = blockIdx.y, w = w0 >> l, h = h0 >> l, npx = w * h;
  const float *__restrict__ in3 = J.in3[l];
  float *__restrict__ plane = J.plane[l];
  int mine = 0, first = 0x7FFFFFFF;
  const int groups = (npx + 3) >> 2;
  for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += gridDim.x * blockDim.x) {
    const int idx = 4 * g;
    float I[4], gx[4], gy[4];
    const int cnt = npx - idx < 4 ? npx - idx : 4;
    if (cnt == 4) {
      const float4 a = ((const float4 *)in3)[3 * (size_t)g], b = ((const float4 *)in3)[3 * (size_t)g + 1], c = ((const float4 *)in3)[3 * (size_t)g + 2];
      I[0] = a.x, gx[0] = a.y, gy[0] = a.z;
      I[1] = a.w, gx[1] = b.x, gy[1] = b.y;
      I[2] = b.z, gx[2] = b.w, gy[2] = c.x;
      I[3] = c.y, gx[3] = c.z, gy[3] = c.w;
      ((float4 *)plane)[g] = make_float4(I[0], I[1], I[2], I[3]);
    } else {
      for (int k = 0; k < 4; k++) {
        const bool in = k < cnt;
        I[k] = in ? in3[3 * (size_t)(idx + k)] : 0.f;
        gx[k] = in ? in3[3 * (size_t)(idx + k) + 1] : 0.f;
        gy[k] = in ? in3[3 * (size_t)(idx + k) + 2] : 0.f;
        if (in) plane[idx + k] = I[k];
      }
    }
    if (!check) continue;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int t = idx + k;
      if (k >= cnt || t < w || t >= w * (h - 1)) continue; // rows makeImages leaves untouched are never read by the tracker
      const float left = k > 0 ? I[k - 1] : in3[3 * (size_t)(t - 1)];
      const float right = (k < 3 && k + 1 < cnt) ? I[k + 1] : in3[3 * (size_t)(t + 1)];
      if (pose_texel_off(in3, w, t, left, right, gx[k], gy[k], tol)) {
        mine++;
        if (t < first) first = t;
      }
    }
  }
  if (mine) {
    atomicAdd(J.bad + 2 * l, mine);
    atomicMin(J.bad + 2 * l + 1, first);
  }
}

void launch_pose_import(hipStream_t s, const PoseImportJob *d_jobs, int njobs, int w, int h, int nlevels, bool check, float tol) {
  if (njobs <= 0) return;
  int gx = ((w * h + 3) / 4 + 255) / 256;
  if (gx > 128) gx = 128;
  hipLaunchKernelGGL(pose_import_kernel, dim3(gx, nlevels, njobs), dim3(256), 0, s, d_jobs, w, h, check ? 1 : 0, tol);
}

} // namespace dsm
