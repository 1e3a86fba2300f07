// The AOV-guided a-trous denoiser (dr_accum_denoise): the kernels over the pixel grid.  A kernel is its thread-to-pixel mapping and a call of
// the stage's body in device_denoise.hpp (dn_*_pixel), which holds every pixel's arithmetic and indexing and runs unchanged in the host build.
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
#include "kernels.hpp"

namespace dr {

namespace {

__global__ __launch_bounds__(256) void dn_guide_kernel(DnLaunch L) {
  const int x = (int)(blockIdx.x * 16 + (threadIdx.x & 15)), y = (int)(blockIdx.y * 16 + (threadIdx.x >> 4));
  if (x >= L.gw || y >= L.gh) return;
  dn_guide_pixel(L, x, y);
}

// consecutive threads walk a column of the accumulator (coalesced reads, as present_kernel)
__global__ __launch_bounds__(256) void dn_colour_kernel(DnLaunch L) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)L.gw * L.gh) return;
  const int x = (int)(idx / L.gh), y = (int)(idx - (long long)x * L.gh);
  dn_colour_pixel(L, x, y);
}

__global__ __launch_bounds__(256) void dn_variance_kernel(DnLaunch L) {
  const int x = (int)(blockIdx.x * 16 + (threadIdx.x & 15)), y = (int)(blockIdx.y * 16 + (threadIdx.x >> 4));
  if (x >= L.gw || y >= L.gh) return;
  dn_variance_pixel(L, x, y);
}

// plain shape: one thread per pixel of a 16x16 block, every tap from the planes
__global__ __launch_bounds__(256) void dn_pass_global_kernel(DnLaunch L, int step) {
  const int x = (int)(blockIdx.x * 16 + (threadIdx.x & 15)), y = (int)(blockIdx.y * 16 + (threadIdx.x >> 4));
  if (x >= L.gw || y >= L.gh) return;
  dn_pass_pixel(L, step, x, y);
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
  dn_finish_pixel(L, x, y);
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
