// delta_math.hpp -- one entry of EnergyFunctional::setDeltaF's adHTdeltaF as DESIGN.md section 21 states it, for everyone who forms it:
// MarginalizeRequest::setDeltaF (host/WindowMarginalize.hpp), the finish of optimize on the device (finish_kernels.hip) and its host
// form (finish_host.cpp).  Plain C++ that needs no other header of the library; float products and sums over ascending k from 0, the
// host's part and the target's part added last, no contraction.
#pragma once

#if defined(__HIPCC__)
#define DSM_DELTA_HD __host__ __device__ __forceinline__
#else
#define DSM_DELTA_HD inline
#endif

namespace dsm {

// entry c of pair (h, t), h != t: ad_host, ad_target the pair's 8 x 8 (row-major doubles), state_h - zero_h and state_t - zero_t the
// frames' delta_f in double
DSM_DELTA_HD float ad_ht_delta_entry(const double *ad_host, const double *ad_target, const double *state_h, const double *zero_h,
                                     const double *state_t, const double *zero_t, int c) {
  float a = 0.f, b = 0.f;
  for (int k = 0; k < 8; k++) a += (float)(state_h[k] - zero_h[k]) * (float)ad_host[8 * k + c];
  for (int k = 0; k < 8; k++) b += (float)(state_t[k] - zero_t[k]) * (float)ad_target[8 * k + c];
  return a + b;
}

} // namespace dsm
