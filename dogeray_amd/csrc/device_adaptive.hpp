// Device functions of adaptive sampling (dr_render_adaptive): which pixels of the accumulator still ask for samples, which 8x8 tiles
// are therefore rendered, the launch's tile order without the others, and the fold of the new frames into the planes of the rendered tiles only.
// Everything a pixel or a tile does is written once, here, over the launch struct AdLaunch (device_launch.h): ad_asks is one pixel of the selection,
// ad_tile_active a tile's verdict, ad_fold_pixel one pixel of the fold, FlagKeep the predicate of the split (device_split.hpp order_split_plain is
// the split as plain C++, kernels_aux.hip order_split_kernel the one workgroup that computes it).  The gfx950 kernels (kernels_adaptive.hip) map a
// wave to a tile and its lanes to the pixels, ballot and count; the host build (tools/host_kernel/hk_accum.hpp hk_adaptive_select /
// hk_subset_split / hk_adaptive_add) loops and counts; tests/adaptive_checks.py and tests/split_cases.py restate it in numpy, independently.  The noise
// estimate is device_moments.hpp's, the comparison dr_error_result.above's: include/dogeray_amd.h has the definition, operation by operation.
#pragma once
#include "device_moments.hpp"
#include "launch_plan.hpp"

namespace dr {

// pixel `lane` of tile `tile` in the planes: (8 col + (lane >> 3), 8 by + (lane & 7)) at x * H + y
__device__ __forceinline__ size_t ad_pixel(const AdLaunch& L, int tile, int lane) {
  const int col = tile / L.gy, by = tile - col * L.gy;
  return (size_t)(col * 8 + (lane >> 3)) * (size_t)L.H + (size_t)(by * 8 + (lane & 7));
}

// The selection's pixel: n = hist + divide_by samples so far; it asks below min_samples, and -- below max_samples, if there is one -- when its
// noise is estimated and above the tolerance
__device__ __forceinline__ bool ad_asks(const AdLaunch& L, int tile, int lane) {
  const size_t p = ad_pixel(L, tile, lane);
  const long long n = (long long)(L.hist ? L.hist[p] : 0) + (long long)L.divide_by;
  if (n < (long long)L.A.min_samples) return true;
  if (L.A.max_samples != 0 && n >= (long long)L.A.max_samples) return false;
  const int32_t* a = L.acc + p * 3;
  double var = 0.0;
  return mo_variance(a[0], a[1], a[2], L.m2[p], n, var) && mo_sigma(var) > L.A.tolerance;
}

// a tile with `asking` of its 64 pixels asking is rendered
__device__ __forceinline__ bool ad_tile_active(const AdLaunch& L, int asking) { return asking >= L.A.tile_pixels; }

// The fold's pixel: every frame's triple into the sums and its capped luma squared into M2, the frames counted in the history plane.  The sums wrap
// and M2 is a saturating sum of non-negatives: any order of the frames gives the same bits, so the pixel keeps both in registers across the frames
// and writes once.
__device__ __forceinline__ void ad_fold_pixel(const AdLaunch& L, int tile, int lane) {
  const size_t p = ad_pixel(L, tile, lane);
  int32_t* a = L.acc + p * 3;
  uint32_t r = (uint32_t)a[0], g = (uint32_t)a[1], b = (uint32_t)a[2];
  unsigned long long m2 = L.m2[p];
  for (int f = 0; f < L.nframes; f++) {
    const int32_t* fr = L.frames + (size_t)f * L.frame_stride + p * 3;
    const int32_t fr0 = fr[0], fr1 = fr[1], fr2 = fr[2];
    r += (uint32_t)fr0; g += (uint32_t)fr1; b += (uint32_t)fr2;
    m2 = mo_add(m2, mo_square(fr0, fr1, fr2));
  }
  a[0] = (int32_t)r; a[1] = (int32_t)g; a[2] = (int32_t)b;
  L.m2[p] = m2;
  L.hist[p] = (int32_t)((uint32_t)L.hist[p] + (uint32_t)L.nframes);
}

// The split's predicate over the selection's flags: a tile is kept when its flag is set (load and test apart, as device_sky.hpp SkyKeep)
struct FlagKeep {
  typedef uint8_t Value;
  const uint8_t* flag;
  __host__ __device__ __forceinline__ Value load(int t) const { return flag[t]; }
  __host__ __device__ __forceinline__ static bool keep(Value v) { return v != 0; }
  __host__ __device__ __forceinline__ bool operator()(int t) const { return keep(load(t)); }
};

}  // namespace dr
