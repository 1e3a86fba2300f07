// Temporal reprojection of the accumulator (dr_accum_reproject): one kernel over the pixel grid of the `to` view, each pixel's arithmetic the
// device functions of device_reproject.hpp.  A gather bound by memory: per pixel it reads the guides of p (t, normal, material), the guides of the
// pixel q it projects to, q's sums and sample count (and, while the accumulator has a second-moment plane, q's M2), and writes p's.  The guide planes are row-major and the accumulator is column-major, so a
// wave takes one 8x8 tile as kernels_aov.hip does: eight neighbouring lanes read eight neighbouring words of a plane's row, and the eight lanes
// of one column write a 96-byte run of the accumulator; neighbouring p project to neighbouring q, so the gathers come in runs as well.  The ray
// direction is recomputed from the pixel, not read from a plane.  The four classes are counted by wave ballot and one vector atomic per wave
// and class.
#include <hip/hip_runtime.h>

#include "device_moments.hpp"
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
  RpGuides Gt, Gf;
  Gt.t = L.t_to; Gt.normal = L.normal_to; Gt.mat = L.mat_to;
  Gf.t = L.t_from; Gf.normal = L.normal_from; Gf.mat = L.mat_from;
  int qx = 0, qy = 0;
  const int cls = rp_classify(L.R, L.to, L.from, L.J, L.gw, L.gh, x, y, Gt, Gf, qx, qy);
  int32_t sums[3] = {0, 0, 0}, hist = 0;
  unsigned long long m2 = 0;
  if (cls == RP_VALID) {
    const size_t q = (size_t)qx * (size_t)L.H + (size_t)qy;
    const int32_t* aq = L.acc_from + q * 3;
    const int32_t from_sums[3] = {aq[0], aq[1], aq[2]};
    const int32_t hist_q = L.hist_from ? L.hist_from[q] : 0;
    rp_carry(L.R, L.frames, from_sums, hist_q, sums, hist);
    if (L.m2_to) m2 = mo_carry(L.m2_from[q], (long long)hist_q + (long long)L.frames, L.R.max_history);      // (option "moments": the plane goes with the sums)
  }
  const size_t p = (size_t)x * (size_t)L.H + (size_t)y;
  int32_t* ap = L.acc_to + p * 3;
  ap[0] = sums[0]; ap[1] = sums[1]; ap[2] = sums[2];
  L.hist_to[p] = hist;
  if (L.m2_to) L.m2_to[p] = m2;
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
