// Device functions of the second-moment plane (option "moments"; dr_accum_error): per pixel the sum of the squared luma of every frame folded into
// the accumulator, the noise estimate formed from it and the accumulated sums, its carry across a reprojection and the temporal variance the
// denoiser may take from it.  Written once and included by the gfx950 kernels (kernels_moments.hip, kernels_reproject.hip, kernels_denoise.hip)
// and the host build (tools/host_kernel.cpp hk_moments_add / hk_error / hk_reproject_m2 / hk_denoise_m2), so both run the same arithmetic;
// tests/moments_checks.py restates it in numpy int64 / uint64 / float64.  Integer arithmetic is exact; the estimate is double, only + - * /,
// sqrt, floor and comparisons in the order written here (-ffp-contract=off): include/dogeray_amd.h has the definition this file implements,
// operation by operation.
#pragma once
#ifdef DR_HOST_BUILD
#include "host_stubs.hpp"
#else
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

#include "device_layout.h"

namespace dr {

// Rec.709 luma x 256 of an int32 triple: the weights sum to 256, |y| < 2^39
__device__ __forceinline__ long long mo_luma(int32_t r, int32_t g, int32_t b) { return (54ll * (long long)r + 183ll * (long long)g) + 19ll * (long long)b; }

// what one frame adds to M2: the capped luma, squared (<= 2^52)
__device__ __forceinline__ unsigned long long mo_square(int32_t r, int32_t g, int32_t b) {
  const long long y = mo_luma(r, g, b);
  const long long yc = y < -MO_CAP ? -MO_CAP : (y > MO_CAP ? MO_CAP : y);
  return (unsigned long long)(yc * yc);
}

// M2 + sq, saturating at 2^64 - 1
__device__ __forceinline__ unsigned long long mo_add(unsigned long long m2, unsigned long long sq) {
  const unsigned long long s = m2 + sq;
  return s < m2 ? ~0ull : s;
}

// What a valid pixel of a reprojection carries: M2 as it is while cnt <= max_history, beyond that floor(M2 * max_history / cnt) exactly
// (M2 = a cnt + b, b < cnt: a max_history + floor(b max_history / cnt), and b max_history < 2^32 x 2^16) -- the factor the sums are scaled by
__device__ __forceinline__ unsigned long long mo_carry(unsigned long long m2, long long cnt, int max_history) {
  if (cnt <= (long long)max_history) return m2;
  const unsigned long long c = (unsigned long long)cnt, mh = (unsigned long long)max_history;
  return (m2 / c) * mh + ((m2 % c) * mh) / c;
}

// var_p: the variance of the displayed mean luma of a pixel with n samples, in (0..255 units)^2.  false for n < 2 (not estimated).
__device__ __forceinline__ bool mo_variance(int32_t r, int32_t g, int32_t b, unsigned long long m2, long long n, double& var) {
  if (n < 2) return false;
  const double S1d = (double)mo_luma(r, g, b), M2d = (double)m2;
  double ss = M2d - (S1d * S1d) / (double)n;
  ss = ss > 0.0 ? ss : 0.0;
  var = (ss / ((double)(n - 1) * (double)n)) / 65536.0;
  return true;
}

__device__ __forceinline__ float mo_sigma(double var) { return (float)__builtin_sqrt(var); }

// bin 0: sigma < 2^-6; bin k: 2^(k-7) <= sigma < 2^(k-6), k = 1 .. 14; bin 15: sigma >= 2^8
__device__ __forceinline__ int mo_bin(float sigma) {
  int k = 0;
  float t = 0.015625f;
#pragma unroll
  for (int i = 0; i < MO_BINS - 1; i++) {
    if (sigma >= t) k = i + 1;
    t = t * 2.0f;
  }
  return k;
}

// min(floor(var * 65536), 2^40)
__device__ __forceinline__ unsigned long long mo_var_q16(double var) {
  const double q = var * 65536.0;
  return q < 1099511627776.0 ? (unsigned long long)__builtin_floor(q) : (1ull << 40);
}

// The denoiser's temporal variance (option "denoise_variance"): var_p over the squared luma of the demodulating albedo a' (the moments are of the
// luma BEFORE demodulation: a stated approximation), for pixels with n >= 4 samples and la != 0; false: the spatial estimate stands.
__device__ __forceinline__ bool mo_denoise_variance(int32_t r, int32_t g, int32_t b, unsigned long long m2, long long n, float ar, float ag, float ab, float& var) {
  if (n < 4) return false;
  const float la = (0.2126f * ar + 0.7152f * ag) + 0.0722f * ab;
  if (la == 0.0f) return false;
  double vp = 0.0;
  mo_variance(r, g, b, m2, n, vp);
  var = (float)(vp / ((double)la * (double)la));
  return true;
}

}  // namespace dr
