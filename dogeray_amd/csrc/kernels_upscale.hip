// The AOV-guided upsampler (dr_accum_upscale): one kernel, one thread per pixel of the W x H output, each pixel's arithmetic the device functions
// of device_upscale.hpp.  The output grid is gw div x gh div; pixels outside it are 0.
//   block   the low pixel (X / div, Y / div): c as f32, dr_accum_present's integer divide as RGB8 (the reference's display, K:2287-2300)
//   guided  the four low taps around P, loaded straight from the low planes (a low tap is shared by the 4 div^2 threads around it: neighbouring
//           lanes of a wave, served by the vector L1), weighted against P's full-resolution guides
// Low planes are row-major over the low grid (pixel (x, y) at y * gw + x), full planes over the full grid (Y * FW + X), as launch_aov and
// launch_denoise_guides write them; the accumulator is column-major ((x * H + y) * 3).
#include <hip/hip_runtime.h>

#include "device_upscale.hpp"
#include "kernels.hpp"

namespace dr {

namespace {

// consecutive threads walk a row of the output (coalesced writes, coalesced reads of the full guides)
__global__ __launch_bounds__(256) void up_kernel(UpLaunch L) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)L.W * L.H) return;
  const int Y = (int)(idx / L.W), X = (int)(idx - (long long)Y * L.W);
  const size_t o = (size_t)idx * 3;
  float f[3] = {0.0f, 0.0f, 0.0f};
  bool inside = X < L.gw * L.div && Y < L.gh * L.div;
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
    const bool found = up_guided(L.U, L.div, X, Y, reinterpret_cast<const float4*>(L.Fguide)[p], mp, L.Fgz[p], ap, [&](int qx, int qy) {
      DnTap q;
      if (qx < 0 || qy < 0 || qx >= L.gw || qy >= L.gh) {
        q.m = DN_OUTSIDE; q.c = make_float4(0, 0, 0, 0); q.g = q.c;
        return q;
      }
      const size_t j = (size_t)qy * L.gw + qx;
      q.c = reinterpret_cast<const float4*>(L.e)[j]; q.g = reinterpret_cast<const float4*>(L.guide)[j]; q.m = L.mat[j];
      return q;
    }, f);
    if (!found) up_block_colour(L.acc, L.hist, L.H, X / L.div, Y / L.div, L.divide_by, f);
  }
  if (L.out_f32) { L.out_f32[o] = f[0]; L.out_f32[o + 1] = f[1]; L.out_f32[o + 2] = f[2]; }
  if (L.out_rgb8) { L.out_rgb8[o] = dn_rgb8(f[0]); L.out_rgb8[o + 1] = dn_rgb8(f[1]); L.out_rgb8[o + 2] = dn_rgb8(f[2]); }
}

}  // namespace

void launch_upscale(hipStream_t stream, const UpLaunch& L) {
  const long long n = (long long)L.W * L.H;
  if (n <= 0) return;
  hipLaunchKernelGGL(up_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, L);
}

}  // namespace dr
