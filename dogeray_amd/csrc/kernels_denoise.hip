// The AOV-guided a-trous denoiser (dr_accum_denoise): four kernels over the pixel grid, each pixel's arithmetic one device function of
// device_denoise.hpp.
//   guide prepare   (n, z) packed into a float4 plane, the material plane completed, the depth gradient gz
//   colour prepare  stage 0: the column-major accumulator -> c = acc / divide_by -> e = c / a' -> (e, l) plane
//                   stage 1: (e, l) -> the variance pre-pass -> (e, var) plane (option "denoise_variance": the temporal variance of the second-moment
//                            plane for pixels with four samples or more)
//   a-trous pass    (e, var) -> (e', var') at step 2^i, ping-pong between two planes; two shapes (option denoise_tiles):
//                   1: one workgroup per 16x16 LATTICE tile -- at step s it filters the pixels (x0 + s i, y0 + s j), whose taps lie on the same
//                      lattice, so one 20x20-point LDS tile of colour, guides and materials serves every step (the apron does not grow with s)
//                   0: one thread per pixel, every tap loaded from the planes
//   finish          e' * a' as f32 and / or RGB8 in dr_accum_present's layout (row-major W x H, 0 outside the grid)
// Planes are row-major over the grid (pixel (x, y) at y * gw + x), as dr_render_aov writes them.
#include <hip/hip_runtime.h>

#include "device_denoise.hpp"
#include "device_moments.hpp"
#include "kernels.hpp"

namespace dr {

namespace {

__global__ __launch_bounds__(256) void dn_guide_kernel(DnLaunch L) {
  const int x = (int)(blockIdx.x * 16 + (threadIdx.x & 15)), y = (int)(blockIdx.y * 16 + (threadIdx.x >> 4));
  if (x >= L.gw || y >= L.gh) return;
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

// consecutive threads walk a column of the accumulator (coalesced reads, as present_kernel)
__global__ __launch_bounds__(256) void dn_colour_kernel(DnLaunch L) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)L.gw * L.gh) return;
  const int x = (int)(idx / L.gh), y = (int)(idx - (long long)x * L.gh);
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

__global__ __launch_bounds__(256) void dn_variance_kernel(DnLaunch L) {
  const int x = (int)(blockIdx.x * 16 + (threadIdx.x & 15)), y = (int)(blockIdx.y * 16 + (threadIdx.x >> 4));
  if (x >= L.gw || y >= L.gh) return;
  const size_t i = (size_t)y * L.gw + x;
  const float4 gp = reinterpret_cast<const float4*>(L.guide)[i];
  const int m = L.mat[i];
  float var = 0.0f;
  bool temporal = false;
  if (L.m2) {                                // option "denoise_variance": SVGF's rule, the temporal second moment once the pixel has four samples
    const size_t px = (size_t)x * (size_t)L.H + (size_t)y;
    const int32_t* a = L.acc + px * 3;
    temporal = mo_denoise_variance(a[0], a[1], a[2], L.m2[px], (long long)dn_divisor(L.hist, px, L.divide_by), dn_albedo(L.albedo[3 * i], m, L.D.demodulate),
                                   dn_albedo(L.albedo[3 * i + 1], m, L.D.demodulate), dn_albedo(L.albedo[3 * i + 2], m, L.D.demodulate), var);
  }
  if (!temporal) var = dn_variance(L.D, gp, m, L.gz[i], [&](int dx, int dy) { return dn_tap_global(L, x + dx, y + dy); });
  const float4 c = reinterpret_cast<const float4*>(L.src)[i];
  reinterpret_cast<float4*>(L.dst)[i] = make_float4(c.x, c.y, c.z, var);
}

// plain shape: one thread per pixel of a 16x16 block, every tap from the planes
__global__ __launch_bounds__(256) void dn_pass_global_kernel(DnLaunch L, int step) {
  const int x = (int)(blockIdx.x * 16 + (threadIdx.x & 15)), y = (int)(blockIdx.y * 16 + (threadIdx.x >> 4));
  if (x >= L.gw || y >= L.gh) return;
  const size_t i = (size_t)y * L.gw + x;
  reinterpret_cast<float4*>(L.dst)[i] = dn_atrous(L.D, step, reinterpret_cast<const float4*>(L.guide)[i], (int)L.mat[i], L.gz[i], [&](int dx, int dy) { return dn_tap_global(L, x + step * dx, y + step * dy); });
}

// lattice shape: workgroup (blockIdx.x, blockIdx.y) = residue class (rx, ry) = (bx % step, by % step) and lattice tile (tx, ty) = (bx / step, by / step);
// thread (i, j) filters pixel (rx + step (16 tx + i), ry + step (16 ty + j)); LDS point (u, v) is lattice index (16 tx + u - 2, 16 ty + v - 2)
constexpr int DN_T = 16, DN_A = 2, DN_P = DN_T + 2 * DN_A;
__global__ __launch_bounds__(256) void dn_pass_lattice_kernel(DnLaunch L, int step) {
  __shared__ float4 s_c[DN_P * DN_P];
  __shared__ float4 s_g[DN_P * DN_P];
  __shared__ int s_m[DN_P * DN_P];
  const int rx = (int)blockIdx.x % step, tx = (int)blockIdx.x / step, ry = (int)blockIdx.y % step, ty = (int)blockIdx.y / step;
  const int t = (int)threadIdx.x;
  for (int k = t; k < DN_P * DN_P; k += 256) {
    const int u = k % DN_P, v = k / DN_P;
    const int px = rx + step * (DN_T * tx + u - DN_A), py = ry + step * (DN_T * ty + v - DN_A);
    const DnTap q = dn_tap_global(L, px, py);
    s_c[k] = q.c; s_g[k] = q.g; s_m[k] = q.m;
  }
  __syncthreads();
  const int i = t & (DN_T - 1), j = t >> 4;
  const int x = rx + step * (DN_T * tx + i), y = ry + step * (DN_T * ty + j);
  if (x >= L.gw || y >= L.gh) return;
  const int c0 = (j + DN_A) * DN_P + (i + DN_A);
  const size_t p = (size_t)y * L.gw + x;
  reinterpret_cast<float4*>(L.dst)[p] = dn_atrous(L.D, step, s_g[c0], s_m[c0], L.gz[p], [&](int dx, int dy) {
    const int k = c0 + dy * DN_P + dx;
    DnTap q;
    q.c = s_c[k]; q.g = s_g[k]; q.m = s_m[k];
    return q;
  });
}

// one thread per pixel of the W x H output, row-major (coalesced writes)
__global__ __launch_bounds__(256) void dn_finish_kernel(DnLaunch L) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)L.W * L.H) return;
  const int y = (int)(idx / L.W), x = (int)(idx - (long long)y * L.W);
  float f[3] = {0.0f, 0.0f, 0.0f};
  if (x < L.gw && y < L.gh) {
    const size_t i = (size_t)y * L.gw + x;
    if (L.D.iterations == 0) {               // no filter, no demodulation: c itself
      const size_t px = (size_t)x * (size_t)L.H + (size_t)y;
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
  const size_t o = (size_t)idx * 3;
  if (L.out_f32) { L.out_f32[o] = f[0]; L.out_f32[o + 1] = f[1]; L.out_f32[o + 2] = f[2]; }
  if (L.out_rgb8) { L.out_rgb8[o] = dn_rgb8(f[0]); L.out_rgb8[o + 1] = dn_rgb8(f[1]); L.out_rgb8[o + 2] = dn_rgb8(f[2]); }
}

dim3 grid16(int w, int h) { return dim3((unsigned)((w + 15) / 16), (unsigned)((h + 15) / 16)); }

}  // namespace

void launch_denoise_guides(hipStream_t stream, const DnLaunch& L) {
  if (L.gw <= 0 || L.gh <= 0) return;
  hipLaunchKernelGGL(dn_guide_kernel, grid16(L.gw, L.gh), dim3(256), 0, stream, L);
}

void launch_denoise_colour(hipStream_t stream, const DnLaunch& L, int stage) {
  if (L.gw <= 0 || L.gh <= 0) return;
  if (stage == 0) {
    const long long n = (long long)L.gw * L.gh;
    hipLaunchKernelGGL(dn_colour_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, L);
  } else {
    hipLaunchKernelGGL(dn_variance_kernel, grid16(L.gw, L.gh), dim3(256), 0, stream, L);
  }
}

void launch_denoise_pass(hipStream_t stream, const DnLaunch& L, int step, int lattice) {
  if (L.gw <= 0 || L.gh <= 0) return;
  if (lattice) {
    // lattice points per residue class, at most ceil(g / step) along each axis
    const int lx = (L.gw + step - 1) / step, ly = (L.gh + step - 1) / step;
    const dim3 grid((unsigned)(((lx + DN_T - 1) / DN_T) * step), (unsigned)(((ly + DN_T - 1) / DN_T) * step));
    hipLaunchKernelGGL(dn_pass_lattice_kernel, grid, dim3(256), 0, stream, L, step);
  } else {
    hipLaunchKernelGGL(dn_pass_global_kernel, grid16(L.gw, L.gh), dim3(256), 0, stream, L, step);
  }
}

void launch_denoise_finish(hipStream_t stream, const DnLaunch& L) {
  const long long n = (long long)L.W * L.H;
  if (n <= 0) return;
  hipLaunchKernelGGL(dn_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, L);
}

}  // namespace dr
