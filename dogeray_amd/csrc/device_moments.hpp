// Device functions of the second-moment plane (option "moments"; dr_accum_error): per pixel the sum of the squared luma of every frame folded into
// the accumulator, the noise estimate formed from it and the accumulated sums, its carry across a reprojection and the temporal variance the
// denoiser may take from it.  Everything a pixel does is written once, here: mo_add_pixel is one pixel of the fused add, mo_error_pixel (of the
// launch struct MoLaunch, device_launch.h, and the pixel) the noise estimate; the carry and the temporal variance are called by the bodies of
// device_reproject.hpp and device_denoise.hpp.  The gfx950 kernels (kernels_moments.hip) map threads to pixels, call them and reduce the counts
// per wave; the host build (tools/host_kernel.cpp hk_moments_add / hk_error) loops over the pixels, calls them and counts;
// tests/moments_checks.py restates it in numpy int64 / uint64 / float64, independently.  Integer arithmetic is exact; the estimate is double, only + - * /,
// sqrt, floor and comparisons in the order written here (-ffp-contract=off): include/dogeray_amd.h has the definition this file implements,
// operation by operation.
#pragma once
#include "device_prims.hpp"      // the device or the host build's runtime (the one switch between them)
#include <stdint.h>

#include "device_launch.h"

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

// One pixel of the fused add: acc += frame (the sums wrap as two's complement) and M2 += yc^2, in place; acc / frame 3 words per pixel
__device__ __forceinline__ void mo_add_pixel(int32_t* acc, const int32_t* frame, unsigned long long* m2, size_t p) {
  const int32_t r = frame[3 * p], g = frame[3 * p + 1], b = frame[3 * p + 2];
  acc[3 * p] = (int32_t)((uint32_t)acc[3 * p] + (uint32_t)r);
  acc[3 * p + 1] = (int32_t)((uint32_t)acc[3 * p + 1] + (uint32_t)g);
  acc[3 * p + 2] = (int32_t)((uint32_t)acc[3 * p + 2] + (uint32_t)b);
  m2[p] = mo_add(m2[p], mo_square(r, g, b));
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

// The noise estimate of grid pixel (x, y): n = its history + divide_by samples; false for a pixel that is not estimated (sigma 0), otherwise var
// and sigma.  sigma goes into the row-major W x H plane when there is one; the accumulator, its history plane and M2 are column-major (x * H + y).
__device__ __forceinline__ bool mo_error_pixel(const MoLaunch& L, int x, int y, double& var, float& sigma) {
  const size_t p = (size_t)x * (size_t)L.H + (size_t)y;
  const int32_t* a = L.acc + p * 3;
  const long long n = (long long)(L.hist ? L.hist[p] : 0) + (long long)L.divide_by;
  var = 0.0;
  const bool est = mo_variance(a[0], a[1], a[2], L.m2[p], n, var);
  sigma = est ? mo_sigma(var) : 0.0f;
  if (L.out_sigma) L.out_sigma[(size_t)y * (size_t)L.W + (size_t)x] = sigma;
  return est;
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
