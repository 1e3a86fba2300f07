// The second-moment plane (option "moments"; dr_accum_error): two kernels.  A pixel's arithmetic and indexing are the bodies of device_moments.hpp
// (mo_add_pixel, mo_error_pixel), which run unchanged in the host build; here are the thread-to-pixel mappings, the four-pixel vector shape of the
// add and the wave reductions of the counts.
//   fused add   acc += frame and M2 += yc^2 in one pass over the column-major accumulator, in place of frame_add_kernel while a plane exists.
//               A stream bound by memory: 52 bytes per pixel (12 of frame, 12 + 12 of acc, 8 + 8 of M2) against the plain add's 36.  A lane
//               takes FOUR pixels, so that every access is a 16-byte vector access: 3 x 16 B of frame, 3 x 16 B of acc, 2 x 16 B of M2; the
//               pixels left over (W * H % 4, or all of them when a frame buffer is not 16-byte aligned) go one by one.
//   error       sigma_p of every pixel of the grid and the counts of dr_error_result.  A wave takes one 8x8 tile as reproject_kernel does: the
//               eight lanes of a column read 96-byte runs of the accumulator and 64-byte runs of M2, eight neighbouring lanes write eight
//               neighbouring floats of a row of the row-major sigma plane.  Every field is an integer, reduced per wave by ballot (the counts)
//               or shuffles (the fixed-point sum) and added with one vector atomic per wave and field: any order gives the same bits.
#include <hip/hip_runtime.h>

#include "device_moments.hpp"
#include "kernels.hpp"

namespace dr {

namespace {

__global__ __launch_bounds__(256) void moments_add_kernel(int4* __restrict__ acc, const int4* __restrict__ frame, ulonglong2* __restrict__ m2, size_t n4,
                                                          size_t npix) {
  const size_t stride = (size_t)gridDim.x * blockDim.x, first = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (size_t i = first; i < n4; i += stride) {
    // pixels 4 i .. 4 i + 3: (f0.x f0.y f0.z) (f0.w f1.x f1.y) (f1.z f1.w f2.x) (f2.y f2.z f2.w)
    const int4 f0 = frame[3 * i], f1 = frame[3 * i + 1], f2 = frame[3 * i + 2];
    int4 a0 = acc[3 * i], a1 = acc[3 * i + 1], a2 = acc[3 * i + 2];
    ulonglong2 ma = m2[2 * i], mb = m2[2 * i + 1];
    a0.x += f0.x; a0.y += f0.y; a0.z += f0.z; a0.w += f0.w;
    a1.x += f1.x; a1.y += f1.y; a1.z += f1.z; a1.w += f1.w;
    a2.x += f2.x; a2.y += f2.y; a2.z += f2.z; a2.w += f2.w;
    ma.x = mo_add(ma.x, mo_square(f0.x, f0.y, f0.z));
    ma.y = mo_add(ma.y, mo_square(f0.w, f1.x, f1.y));
    mb.x = mo_add(mb.x, mo_square(f1.z, f1.w, f2.x));
    mb.y = mo_add(mb.y, mo_square(f2.y, f2.z, f2.w));
    acc[3 * i] = a0; acc[3 * i + 1] = a1; acc[3 * i + 2] = a2;
    m2[2 * i] = ma; m2[2 * i + 1] = mb;
  }
  int32_t* as = reinterpret_cast<int32_t*>(acc);
  const int32_t* fs = reinterpret_cast<const int32_t*>(frame);
  unsigned long long* ms = reinterpret_cast<unsigned long long*>(m2);
  for (size_t p = n4 * 4 + first; p < npix; p += stride) mo_add_pixel(as, fs, ms, p);
}

// lane l of a tile is pixel (l & 7, l >> 3); the grid is whole tiles, so every lane of a launched tile has a pixel
__global__ __launch_bounds__(256) void moments_error_kernel(MoLaunch L) {
  const int wave = (int)(blockIdx.x * 4 + (threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63);
  const int tiles_x = L.gw >> 3;
  if (wave >= tiles_x * (L.gh >> 3)) return;
  const int x = (wave % tiles_x) * 8 + (lane & 7), y = (wave / tiles_x) * 8 + (lane >> 3);
  double var;
  float sigma;
  const bool est = mo_error_pixel(L, x, y, var, sigma);
  if (!L.counts) return;
  const int bin = est ? mo_bin(sigma) : -1;
  unsigned long long q = est ? mo_var_q16(var) : 0ull;
  for (int off = 32; off > 0; off >>= 1) q += __shfl_xor(q, off, 64);
  const unsigned long long be = __ballot(est), ba = __ballot(est && sigma > L.tolerance);
  if (lane == 0) {
    if (be) atomicAdd(L.counts + MO_ESTIMATED, (unsigned long long)__popcll(be));
    if (ba) atomicAdd(L.counts + MO_ABOVE, (unsigned long long)__popcll(ba));
    if (q) atomicAdd(L.counts + MO_SUM_VAR, q);
  }
#pragma unroll
  for (int k = 0; k < MO_BINS; k++) {
    const unsigned long long b = __ballot(bin == k);
    if (lane == 0 && b) atomicAdd(L.counts + MO_BIN0 + k, (unsigned long long)__popcll(b));
  }
}

}  // namespace

void launch_moments_add(hipStream_t stream, int32_t* acc, const int32_t* frame, unsigned long long* m2, size_t npix) {
  if (npix == 0) return;
  // (hipMalloc aligns acc and M2; frame f of a group starts f * W * H * 12 bytes into its slot)
  const bool aligned = ((reinterpret_cast<uintptr_t>(acc) | reinterpret_cast<uintptr_t>(frame) | reinterpret_cast<uintptr_t>(m2)) & 15u) == 0;
  const size_t n4 = aligned ? npix / 4 : 0, work = n4 > 0 ? n4 : npix;
  size_t blocks = (work + 255) / 256; if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(moments_add_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, reinterpret_cast<int4*>(acc), reinterpret_cast<const int4*>(frame),
                     reinterpret_cast<ulonglong2*>(m2), n4, npix);
}

void launch_moments_error(hipStream_t stream, const MoLaunch& L) {
  const long long tiles = (long long)(L.gw >> 3) * (long long)(L.gh >> 3);
  if (tiles <= 0) return;
  hipLaunchKernelGGL(moments_error_kernel, dim3((unsigned)((tiles + 3) / 4)), dim3(256), 0, stream, L);
}

}  // namespace dr
