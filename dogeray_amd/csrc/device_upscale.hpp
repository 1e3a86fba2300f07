// Device functions of the AOV-guided upsampler (dr_accum_upscale): a joint-bilateral upsample (Kopf et al. 2007) of the demodulated
// low-resolution accumulator, guided by the first-hit AOVs of the same view at full resolution, with the denoiser's normal, depth and material
// stops (device_denoise.hpp: dn_stop, dn_wn, dn_xz) and the full-resolution albedo multiplied back.  Everything an output pixel does is written
// once, here: up_pixel takes the launch struct (UpLaunch, device_launch.h) and the pixel and covers both modes, the fallback of a pixel without a
// tap and both outputs.  The gfx950 kernel (kernels_upscale.hip) maps a thread to a pixel and calls it, the host build (tools/host_kernel.cpp
// hk_upscale) loops over the pixels and calls it; tests/upscale_checks.py restates it in numpy float32, independently.  Only + - * /, fminf /
// fmaxf and comparisons, in the order written here (-ffp-contract=off): include/dogeray_amd.h has the definition this file implements, operation
// by operation.
#pragma once
#include "device_denoise.hpp"

namespace dr {

// Where output coordinate X falls between the low pixel centres: the left tap x0 (-1 on the left edge) and the weight f of the right tap,
// in integers first -- t = 2 X + 1 - div, x0 = floor(t / (2 div)), r = t - 2 div x0, f = (float)r / (float)(2 div)
__device__ __forceinline__ void up_position(int X, int div, int& x0, float& f) {
  const int t = 2 * X + 1 - div;
  x0 = t < 0 ? -1 : t / (2 * div);               // t > -2 div: the floor of a negative quotient is -1
  const int r = t - 2 * div * x0;
  f = (float)r / (float)(2 * div);
}

// c of low pixel (qx, qy), per channel: the block value
__device__ __forceinline__ void up_block_colour(const int32_t* acc, const int32_t* hist, int H, int qx, int qy, int divide_by, float c[3]) {
  const size_t px = (size_t)qx * (size_t)H + (size_t)qy;
  const int n = dn_divisor(hist, px, divide_by);
  c[0] = dn_colour(acc[3 * px], n); c[1] = dn_colour(acc[3 * px + 1], n); c[2] = dn_colour(acc[3 * px + 2], n);
}

// One channel of dr_accum_present's integer image: clamp(sum / divisor, 0, 255), the division towards zero, a divisor of 0 giving 0
__device__ __forceinline__ uint8_t up_present8(int32_t sum, int divisor) {
  if (divisor == 0) return 0;
  const int v = sum / divisor;
  return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// The guided value of output pixel P = (X, Y): gp = (N_P, Z_P), mp = M_P, gzp the depth gradient and ap = A'_P of the full-resolution guides;
// tap(qx, qy) returns low pixel q with c = (e_q, *), g = (n_q, z_q), m = m_q, or m = DN_OUTSIDE for a q outside the low grid.  Taps j = 0, 1
// outer, i = 0, 1 inner, q = (x0 + i, y0 + j):
//   b = bx_i * by_j, bx = (1 - fx, fx); no tap for q outside, b == 0, exactly one of M_P, m_q a miss, or (material_stop) M_P != m_q
//   both miss: w = b; otherwise w = (b * wn) / q(xz) with the denoiser's wn and xz, rz = 1 / ((sigma_depth * gz_P) * (float)div + 1e-3f * Z_P)
//   sw += w, s += w * e_q per channel
// sw > 0: f = (s / sw) * A'_P and true; otherwise false (no usable tap: the caller writes the block value) and f is untouched.
template <class Tap>
__device__ __forceinline__ bool up_guided(const UpParams& U, int div, int X, int Y, const float4& gp, int mp, float gzp, const float ap[3], const Tap& tap,
                                          float f[3]) {
  int x0, y0;
  float fx, fy;
  up_position(X, div, x0, fx);
  up_position(Y, div, y0, fy);
  const float bx[2] = {1.0f - fx, fx}, by[2] = {1.0f - fy, fy};
  const float rz = 1.0f / ((U.sigma_depth * gzp) * (float)div + 1e-3f * gp.w);
  float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f;
#pragma unroll
  for (int j = 0; j < 2; j++)
#pragma unroll
    for (int i = 0; i < 2; i++) {
      const float b = bx[i] * by[j];
      if (b == 0.0f) continue;
      const DnTap q = tap(x0 + i, y0 + j);
      if (!dn_stop(U.material_stop, mp, q.m)) continue;
      float w = b;
      if (mp != DN_MISS) w = (b * dn_wn(gp, q.g, U.normal_power_log2)) / dn_q(dn_xz(gp.w, q.g.w, rz));
      sw = sw + w;
      sr = sr + w * q.c.x;
      sg = sg + w * q.c.y;
      sb = sb + w * q.c.z;
    }
  if (!(sw > 0.0f)) return false;
  f[0] = (sr / sw) * ap[0]; f[1] = (sg / sw) * ap[1]; f[2] = (sb / sw) * ap[2];
  return true;
}

// Output pixel (X, Y) of the W x H image, row-major; the output grid is gw div x gh div, pixels outside it are 0.
//   block   the low pixel (X / div, Y / div): c as f32, dr_accum_present's integer divide as RGB8 (the reference's display, K:2287-2300)
//   guided  the four low taps around P, loaded straight from the low planes, weighted against P's full-resolution guides; a pixel without a
//           usable tap takes the block value (*notap = true when notap is given: the host build's plane of such pixels; the kernel passes null)
// Low planes are row-major over the low grid (pixel (x, y) at y * gw + x), full planes over the full grid (Y * FW + X), as launch_aov and
// launch_denoise_guides write them; the accumulator is column-major ((x * H + y) * 3).
__device__ __forceinline__ void up_pixel(const UpLaunch& L, int X, int Y, bool* notap) {
  const size_t o = ((size_t)Y * (size_t)L.W + (size_t)X) * 3;
  float f[3] = {0.0f, 0.0f, 0.0f};
  const bool inside = X < L.gw * L.div && Y < L.gh * L.div;
  if (inside && L.U.mode == UP_BLOCK) {        // the integer present of the low pixel
    const int qx = X / L.div, qy = Y / L.div;
    up_block_colour(L.acc, L.hist, L.H, qx, qy, L.divide_by, f);
    if (L.out_rgb8) {
      const size_t px = (size_t)qx * (size_t)L.H + (size_t)qy;
      const int n = dn_divisor(L.hist, px, L.divide_by);
      L.out_rgb8[o] = up_present8(L.acc[3 * px], n); L.out_rgb8[o + 1] = up_present8(L.acc[3 * px + 1], n); L.out_rgb8[o + 2] = up_present8(L.acc[3 * px + 2], n);
    }
    if (L.out_f32) { L.out_f32[o] = f[0]; L.out_f32[o + 1] = f[1]; L.out_f32[o + 2] = f[2]; }
    return;
  }
  if (inside) {
    const size_t p = (size_t)Y * L.FW + X;
    const int mp = L.Fmat[p];
    const float ap[3] = {dn_albedo(L.Falbedo[3 * p], mp, L.U.demodulate), dn_albedo(L.Falbedo[3 * p + 1], mp, L.U.demodulate),
                         dn_albedo(L.Falbedo[3 * p + 2], mp, L.U.demodulate)};
    const bool found = up_guided(L.U, L.div, X, Y, reinterpret_cast<const float4*>(L.Fguide)[p], mp, L.Fgz[p], ap,
                                 [&](int qx, int qy) {
      DnTap q;
      if (qx < 0 || qy < 0 || qx >= L.gw || qy >= L.gh) {
        q.m = DN_OUTSIDE; q.c = make_float4(0, 0, 0, 0); q.g = q.c;
        return q;
      }
      const size_t j = (size_t)qy * L.gw + qx;
      q.c = reinterpret_cast<const float4*>(L.e)[j]; q.g = reinterpret_cast<const float4*>(L.guide)[j]; q.m = L.mat[j];
      return q;
    }, f);
    if (!found) {
      up_block_colour(L.acc, L.hist, L.H, X / L.div, Y / L.div, L.divide_by, f);
      if (notap) *notap = true;
    }
  }
  if (L.out_f32) { L.out_f32[o] = f[0]; L.out_f32[o + 1] = f[1]; L.out_f32[o + 2] = f[2]; }
  if (L.out_rgb8) { L.out_rgb8[o] = dn_rgb8(f[0]); L.out_rgb8[o + 1] = dn_rgb8(f[1]); L.out_rgb8[o + 2] = dn_rgb8(f[2]); }
}

}  // namespace dr
