// Temporal reprojection of the accumulator (dr_accum_reproject): one kernel over the pixel grid of the `to` view.  The kernel is the lane-to-pixel
// mapping, a call of rp_pixel (device_reproject.hpp), which holds the pixel's arithmetic and indexing and runs unchanged in the host build, and the
// count of the classes.  A gather bound by memory: per pixel it reads the guides of p (t, normal, material), the guides of the pixel q it projects
// to, q's sums and sample count (and, while the accumulator has a second-moment plane, q's M2), and writes p's.  The guide planes are row-major and
// the accumulator is column-major, so a wave takes one 8x8 tile as kernels_aov.hip does: eight neighbouring lanes read eight neighbouring words of a
// plane's row, and the eight lanes of one column write a 96-byte run of the accumulator; neighbouring p project to neighbouring q, so the gathers
// come in runs as well.  The ray direction is recomputed from the pixel, not read from a plane.  The four classes are counted by wave ballot and one
// vector atomic per wave and class.
#include <hip/hip_runtime.h>

#include "device_reproject.hpp"
#include "kernels.hpp"

namespace dr {

namespace {

// lane l of a tile is pixel (l & 7, l >> 3); the grid is whole tiles (gw, gh are multiples of 8), so every lane of a launched tile has a pixel
__global__ __launch_bounds__(256) void reproject_kernel(RpLaunch L) {
  const int wave = (int)(blockIdx.x * 4 + (threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63);
  const int tiles_x = L.gw >> 3;
  if (wave >= tiles_x * (L.gh >> 3)) return;
  const int x = (wave % tiles_x) * 8 + (lane & 7), y = (wave / tiles_x) * 8 + (lane >> 3);
  const int cls = rp_pixel(L, x, y);
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const unsigned long long b = __ballot(cls == k);
    if (lane == 0 && b) atomicAdd(L.counts + k, (unsigned long long)__popcll(b));
  }
}

}  // namespace

void launch_reproject(hipStream_t stream, const RpLaunch& L) {
  const long long tiles = (long long)(L.gw >> 3) * (long long)(L.gh >> 3);
  if (tiles <= 0) return;
  hipLaunchKernelGGL(reproject_kernel, dim3((unsigned)((tiles + 3) / 4)), dim3(256), 0, stream, L);
}

}  // namespace dr
