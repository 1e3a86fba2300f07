// Device functions of the AOV-guided a-trous denoiser (dr_accum_denoise): the spatial part of SVGF (Schied et al. 2017), an edge-avoiding
// a-trous wavelet filter (Dammertz et al. 2010) over the demodulated running mean, with luminance-variance, normal, depth and material stops.
// Written once and included by the gfx950 kernels (kernels_denoise.hip) and the host build (tools/host_kernel.cpp hk_denoise), so both run
// the same arithmetic; tests/denoise_checks.py restates it in numpy float32.  Only + - * /, sqrtf, fminf / fmaxf and comparisons, in the order
// written here (-ffp-contract=off): include/dogeray_amd.h has the definition this file implements, operation by operation.
#pragma once
#ifdef DR_HOST_BUILD
#include "host_stubs.hpp"
#else
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

#include "device_layout.h"

namespace dr {

// What a tap needs of a pixel: its colour plane (e.r, e.g, e.b, w), its packed guide (n.x, n.y, n.z, z) and its material (DN_OUTSIDE: no tap)
struct DnTap {
  float4 c;
  float4 g;
  int m;
};

// phi(x) = 1 / q(x) with q(x) = (1 + x) + (0.5 x) x  (phi(inf) = 0): the rational stand-in for the papers' exp(-x)
__device__ __forceinline__ float dn_q(float x) { return (1.0f + x) + (0.5f * x) * x; }

__device__ __forceinline__ float dn_lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// c of one channel: the sum over the pixel's divisor -- divide_by, plus the pixel's entry of the history plane when the accumulator has one
// (dr_accum_reproject); a divisor of 0 gives 0
__device__ __forceinline__ int dn_divisor(const int32_t* hist, size_t pixel, int divide_by) { return hist ? hist[pixel] + divide_by : divide_by; }
__device__ __forceinline__ float dn_colour(int32_t sum, int divisor) { return divisor == 0 ? 0.0f : (float)sum / (float)divisor; }

// a' of one channel: 1 for a miss, an albedo <= 1e-3, or demodulation off
__device__ __forceinline__ float dn_albedo(float a, int m, int demodulate) { return (!demodulate || m == DN_MISS || a <= 1e-3f) ? 1.0f : a; }

// Depth gradient of pixel p from its four neighbours' depth and material (DN_MISS / DN_OUTSIDE count as +inf in the fminf; an axis with no
// usable neighbour gives 0).  A miss has gradient 0 (it is never read).
__device__ __forceinline__ float dn_gradient(float zp, int mp, float zl, int ml, float zr, int mr, float zu, int mu, float zd, int md) {
  if (mp == DN_MISS) return 0.0f;
  const float inf = __builtin_inff();
  const float ar = (mr == DN_MISS || mr == DN_OUTSIDE) ? inf : __builtin_fabsf(zr - zp);
  const float al = (ml == DN_MISS || ml == DN_OUTSIDE) ? inf : __builtin_fabsf(zp - zl);
  const float ad = (md == DN_MISS || md == DN_OUTSIDE) ? inf : __builtin_fabsf(zd - zp);
  const float au = (mu == DN_MISS || mu == DN_OUTSIDE) ? inf : __builtin_fabsf(zp - zu);
  float gx = __builtin_fminf(ar, al), gy = __builtin_fminf(ad, au);
  if (gx == inf) gx = 0.0f;
  if (gy == inf) gy = 0.0f;
  return __builtin_fmaxf(gx, gy);
}

// The per-pixel constants of the depth stop: rz[k] = 1 / ((sigma_depth * gz_p) * (float)(step * k) + 1e-3f * z_p), k = |dx| + |dy| = 1 .. 4
struct DnDepthStop {
  float rz[5];
};
__device__ __forceinline__ DnDepthStop dn_depth_stop(const DnParams& D, float zp, float gzp, int step) {
  DnDepthStop s;
  s.rz[0] = 0.0f;
  const float a = D.sigma_depth * gzp, b = 1e-3f * zp;
#pragma unroll
  for (int k = 1; k <= 4; k++) s.rz[k] = 1.0f / (a * (float)(step * k) + b);
  return s;
}

// The pair weight without colour, as a fraction num / den (den >= 1):
//   q outside the grid, or exactly one of p, q a miss, or (material_stop) another material: num = 0 (the tap is skipped)
//   both miss, or q = p: 1 / 1
//   otherwise num = wn = fmaxf((n_p.x n_q.x + n_p.y n_q.y) + n_p.z n_q.z, 0) squared normal_power_log2 times,
//             den = q(xz), xz = dz > 0 ? dz * rz[k] : 0, dz = |z_p - z_q|, k = |dx| + |dy|
// Returns false when the tap is skipped (dn_stop).
__device__ __forceinline__ bool dn_stop(const DnParams& D, int mp, int mq) {
  return mq != DN_OUTSIDE && (mp == DN_MISS) == (mq == DN_MISS) && !(D.material_stop && mp != mq);
}
__device__ __forceinline__ bool dn_pair(const DnParams& D, const DnDepthStop& S, const float4& gp, int mp, const DnTap& q, int k, float& num, float& den) {
  if (!dn_stop(D, mp, q.m)) return false;
  num = 1.0f; den = 1.0f;
  if (k == 0 || mp == DN_MISS) return true;
  float wn = __builtin_fmaxf((gp.x * q.g.x + gp.y * q.g.y) + gp.z * q.g.z, 0.0f);
  for (int i = 0; i < D.normal_power_log2; i++) wn = wn * wn;
  const float dz = __builtin_fabsf(gp.w - q.g.w);
  const float xz = dz > 0.0f ? dz * S.rz[k] : 0.0f;
  num = wn;
  den = dn_q(xz);
  return true;
}

// Variance pre-pass at pixel p: var = fmaxf(mu2 - mu1 * mu1, 0), mu1 = s1 / sw, mu2 = s2 / sw over the 5x5 taps at step 1 inside the grid,
// dy = -2 .. 2 outer, dx = -2 .. 2 inner, w = num / den, sw += w, s1 += w * l_q, s2 += w * (l_q * l_q).  tap(dx, dy) returns the tap with
// c.w = l_q.  Returns var.
template <class Tap>
__device__ __forceinline__ float dn_variance(const DnParams& D, const float4& gp, int mp, float gzp, const Tap& tap) {
  const DnDepthStop S = dn_depth_stop(D, gp.w, gzp, 1);
  float sw = 0.0f, s1 = 0.0f, s2 = 0.0f;
#pragma unroll
  for (int dy = -2; dy <= 2; dy++)
#pragma unroll
    for (int dx = -2; dx <= 2; dx++) {
      const DnTap q = tap(dx, dy);
      const int k = (dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy);
      float num, den;
      if (dn_pair(D, S, gp, mp, q, k, num, den)) {
        const float w = num / den;
        sw = sw + w;
        s1 = s1 + w * q.c.w;
        s2 = s2 + w * (q.c.w * q.c.w);
      }
    }
  const float mu1 = s1 / sw, mu2 = s2 / sw;
  return __builtin_fmaxf(mu2 - mu1 * mu1, 0.0f);
}

// One a-trous iteration at pixel p with step `step`; tap(dx, dy) returns the tap at p + step (dx, dy) with c = (e, var), l_q = dn_lum(e_q).
//   gv  = sum kk var_q / sum kk over the 3x3 taps at the same step that dn_stop lets through (dy outer, dx inner), kk = k[dx] * k[dy],
//         k = (1/4, 1/2, 1/4): the variance, like the colour, never crosses an edge stop
//   rl  = 1 / (sigma_luminance * sqrtf(gv) + 1e-4f)
//   w   = (h[dx] * h[dy] * num) / (den * q(xl)), xl = |l_p - l_q| * rl, h = (1/16, 1/4, 3/8, 1/4, 1/16)
//   e'  = (sum w e_q) / sw, var' = (sum (w * w) var_q) / (sw * sw), over the 5x5 taps (dy outer, dx inner)
template <class Tap>
__device__ __forceinline__ float4 dn_atrous(const DnParams& D, int step, const float4& gp, int mp, float gzp, const Tap& tap) {
  const float kw[3] = {0.25f, 0.5f, 0.25f};
  const float hw[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
  float gs = 0.0f, gv = 0.0f;
#pragma unroll
  for (int dy = -1; dy <= 1; dy++)
#pragma unroll
    for (int dx = -1; dx <= 1; dx++) {
      const DnTap q = tap(dx, dy);
      if (dn_stop(D, mp, q.m)) {
        const float kk = kw[dx + 1] * kw[dy + 1];
        gs = gs + kk;
        gv = gv + kk * q.c.w;
      }
    }
  gv = gv / gs;
  const float rl = 1.0f / (D.sigma_luminance * __builtin_sqrtf(gv) + 1e-4f);
  const DnDepthStop S = dn_depth_stop(D, gp.w, gzp, step);
  const DnTap c0 = tap(0, 0);
  const float lp = dn_lum(c0.c.x, c0.c.y, c0.c.z);
  float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sv = 0.0f;
#pragma unroll
  for (int dy = -2; dy <= 2; dy++)
#pragma unroll
    for (int dx = -2; dx <= 2; dx++) {
      const DnTap q = tap(dx, dy);
      const int k = (dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy);
      float num, den;
      if (dn_pair(D, S, gp, mp, q, k, num, den)) {
        const float xl = __builtin_fabsf(lp - dn_lum(q.c.x, q.c.y, q.c.z)) * rl;
        const float w = (hw[dx + 2] * hw[dy + 2] * num) / (den * dn_q(xl));
        sw = sw + w;
        sr = sr + w * q.c.x;
        sg = sg + w * q.c.y;
        sb = sb + w * q.c.z;
        sv = sv + (w * w) * q.c.w;
      }
    }
  return make_float4(sr / sw, sg / sw, sb / sw, sv / (sw * sw));
}

// Output of one channel: f = e * a' (f32), (uint8)(int)fminf(fmaxf(f, 0), 255) (RGB8)
__device__ __forceinline__ uint8_t dn_rgb8(float f) { return (uint8_t)(int)__builtin_fminf(__builtin_fmaxf(f, 0.0f), 255.0f); }

}  // namespace dr
