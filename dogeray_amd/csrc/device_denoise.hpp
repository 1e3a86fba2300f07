// Device functions of the AOV-guided a-trous denoiser (dr_accum_denoise): the spatial part of SVGF (Schied et al. 2017), an edge-avoiding
// a-trous wavelet filter (Dammertz et al. 2010) over the demodulated running mean, with luminance-variance, normal, depth and material stops.
// Everything a pixel of a stage does is written once, here: the small functions, and one body per stage (dn_*_pixel) that takes the launch
// struct (DnLaunch, device_launch.h) and the pixel -- which plane is row-major and which column-major, which albedo a pixel takes, the zero
// outside the grid.  The gfx950 kernels (kernels_denoise.hip) map a thread to a pixel and call the body; the host build (tools/host_kernel.cpp
// hk_denoise) loops over the pixels and calls the same body; tests/denoise_checks.py restates it in numpy float32, independently.  Only + - * /,
// sqrtf, fminf / fmaxf and comparisons, in the order written here (-ffp-contract=off): include/dogeray_amd.h has the definition this file
// implements, operation by operation.
#pragma once
#include "device_prims.hpp"      // the device or the host build's runtime (the one switch between them)
#include <stdint.h>

#include "device_launch.h"
#include "device_moments.hpp"

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
// (dn_stop, dn_wn and dn_xz take the values, not a struct: the upsampler has them too, device_upscale.hpp)
__device__ __forceinline__ bool dn_stop(int material_stop, int mp, int mq) {
  return mq != DN_OUTSIDE && (mp == DN_MISS) == (mq == DN_MISS) && !(material_stop && mp != mq);
}
__device__ __forceinline__ float dn_wn(const float4& gp, const float4& gq, int normal_power_log2) {
  float wn = __builtin_fmaxf((gp.x * gq.x + gp.y * gq.y) + gp.z * gq.z, 0.0f);
  for (int i = 0; i < normal_power_log2; i++) wn = wn * wn;
  return wn;
}
__device__ __forceinline__ float dn_xz(float zp, float zq, float rz) {
  const float dz = __builtin_fabsf(zp - zq);
  return dz > 0.0f ? dz * rz : 0.0f;
}
__device__ __forceinline__ bool dn_pair(const DnParams& D, const DnDepthStop& S, const float4& gp, int mp, const DnTap& q, int k, float& num, float& den) {
  if (!dn_stop(D.material_stop, mp, q.m)) return false;
  num = 1.0f; den = 1.0f;
  if (k == 0 || mp == DN_MISS) return true;
  num = dn_wn(gp, q.g, D.normal_power_log2);
  den = dn_q(dn_xz(gp.w, q.g.w, S.rz[k]));
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
      if (dn_stop(D.material_stop, mp, q.m)) {
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

// ---- one body per stage.  Planes are row-major over the grid (pixel (x, y) at y * gw + x), as dr_render_aov writes them; the accumulator, its
// history plane and the second-moment plane are column-major (x * H + y).

// The tap at (x, y) from the colour plane src, the packed guides and the materials; outside the grid: DN_OUTSIDE and zeros
__device__ __forceinline__ DnTap dn_tap_global(const DnLaunch& L, int x, int y) {
  DnTap q;
  if (x < 0 || y < 0 || x >= L.gw || y >= L.gh) {
    q.m = DN_OUTSIDE; q.c = make_float4(0, 0, 0, 0); q.g = q.c;
    return q;
  }
  const size_t j = (size_t)y * L.gw + x;
  q.c = reinterpret_cast<const float4*>(L.src)[j]; q.g = reinterpret_cast<const float4*>(L.guide)[j]; q.m = L.mat[j];
  return q;
}

// guide prepare: (n, z) packed into the guide plane, the depth gradient into gz (normal, depth, mat -> guide, gz)
__device__ __forceinline__ void dn_guide_pixel(const DnLaunch& L, int x, int y) {
  const size_t i = (size_t)y * L.gw + x;
  auto zm = [&](int xx, int yy, float& z) {
    if (xx < 0 || yy < 0 || xx >= L.gw || yy >= L.gh) { z = 0.0f; return DN_OUTSIDE; }
    const size_t j = (size_t)yy * L.gw + xx;
    z = L.depth[j];
    return (int)L.mat[j];
  };
  float zp, zl, zr, zu, zd;
  const int mp = zm(x, y, zp), ml = zm(x - 1, y, zl), mr = zm(x + 1, y, zr), mu = zm(x, y - 1, zu), md = zm(x, y + 1, zd);
  L.gz[i] = dn_gradient(zp, mp, zl, ml, zr, mr, zu, mu, zd, md);
  reinterpret_cast<float4*>(L.guide)[i] = make_float4(L.normal[3 * i], L.normal[3 * i + 1], L.normal[3 * i + 2], zp);
}

// colour prepare, stage 0: acc -> c -> e = c / a' -> (e, l) in dst
__device__ __forceinline__ void dn_colour_pixel(const DnLaunch& L, int x, int y) {
  const size_t i = (size_t)y * L.gw + x;
  const size_t px = (size_t)x * (size_t)L.H + (size_t)y;
  const int32_t* a = L.acc + px * 3;
  const int n = dn_divisor(L.hist, px, L.divide_by);
  const int m = L.mat[i];
  const float er = dn_colour(a[0], n) / dn_albedo(L.albedo[3 * i], m, L.D.demodulate);
  const float eg = dn_colour(a[1], n) / dn_albedo(L.albedo[3 * i + 1], m, L.D.demodulate);
  const float eb = dn_colour(a[2], n) / dn_albedo(L.albedo[3 * i + 2], m, L.D.demodulate);
  reinterpret_cast<float4*>(L.dst)[i] = make_float4(er, eg, eb, dn_lum(er, eg, eb));
}

// colour prepare, stage 1: src (e, l) -> (e, var) in dst
__device__ __forceinline__ void dn_variance_pixel(const DnLaunch& L, int x, int y) {
  const size_t i = (size_t)y * L.gw + x;
  const float4 gp = reinterpret_cast<const float4*>(L.guide)[i];
  const int m = L.mat[i];
  float var = 0.0f;
  bool temporal = false;
  if (L.m2) {                                // option "denoise_variance": SVGF's rule, the temporal second moment once the pixel has four samples
    const size_t px = (size_t)x * (size_t)L.H + (size_t)y;
    const int32_t* acc = L.acc + px * 3;
    temporal = mo_denoise_variance(acc[0], acc[1], acc[2], L.m2[px], (long long)dn_divisor(L.hist, px, L.divide_by), dn_albedo(L.albedo[3 * i], m, L.D.demodulate),
                                   dn_albedo(L.albedo[3 * i + 1], m, L.D.demodulate), dn_albedo(L.albedo[3 * i + 2], m, L.D.demodulate), var);
  }
  if (!temporal) var = dn_variance(L.D, gp, m, L.gz[i], [&](int dx, int dy) { return dn_tap_global(L, x + dx, y + dy); });
  const float4 c = reinterpret_cast<const float4*>(L.src)[i];
  reinterpret_cast<float4*>(L.dst)[i] = make_float4(c.x, c.y, c.z, var);
}

// one a-trous iteration, every tap from the planes: src -> dst
__device__ __forceinline__ void dn_pass_pixel(const DnLaunch& L, int step, int x, int y) {
  const size_t i = (size_t)y * L.gw + x;
  reinterpret_cast<float4*>(L.dst)[i] = dn_atrous(L.D, step, reinterpret_cast<const float4*>(L.guide)[i], (int)L.mat[i], L.gz[i], [&](int dx, int dy) { return dn_tap_global(L, x + step * dx, y + step * dy); });
}

// finish, pixel (X, Y) of the W x H output: e' * a' as f32 and / or RGB8 in dr_accum_present's layout (row-major, 0 outside the grid)
__device__ __forceinline__ void dn_finish_pixel(const DnLaunch& L, int X, int Y) {
  float f[3] = {0.0f, 0.0f, 0.0f};
  if (X < L.gw && Y < L.gh) {
    const size_t i = (size_t)Y * L.gw + X;
    if (L.D.iterations == 0) {               // no filter, no demodulation: c itself
      const size_t px = (size_t)X * (size_t)L.H + (size_t)Y;
      const int32_t* a = L.acc + px * 3;
      const int n = dn_divisor(L.hist, px, L.divide_by);
      f[0] = dn_colour(a[0], n); f[1] = dn_colour(a[1], n); f[2] = dn_colour(a[2], n);
    } else {
      const float4 e = reinterpret_cast<const float4*>(L.src)[i];
      const int m = L.mat[i];
      f[0] = e.x * dn_albedo(L.albedo[3 * i], m, L.D.demodulate);
      f[1] = e.y * dn_albedo(L.albedo[3 * i + 1], m, L.D.demodulate);
      f[2] = e.z * dn_albedo(L.albedo[3 * i + 2], m, L.D.demodulate);
    }
  }
  const size_t o = ((size_t)Y * (size_t)L.W + (size_t)X) * 3;
  if (L.out_f32) { L.out_f32[o] = f[0]; L.out_f32[o + 1] = f[1]; L.out_f32[o + 2] = f[2]; }
  if (L.out_rgb8) { L.out_rgb8[o] = dn_rgb8(f[0]); L.out_rgb8[o + 1] = dn_rgb8(f[1]); L.out_rgb8[o + 2] = dn_rgb8(f[2]); }
}

}  // namespace dr
