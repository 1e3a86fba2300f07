// Tiles that see nothing of the scene (entry code ENTRY_NONE in the view's entry table): every path of their pixels misses, so a frame
// of such a pixel is spp camera rays and spp backgrounds -- no walk, no path pool.  sky_pixel is that frame, written with the functions the render
// kernels run (render_pixel with a `closest` that always misses); SkyKeep is the predicate by which a launch's tile order is split into the geometry
// tiles the persistent kernel keeps and the sky tiles (device_split.hpp order_split_plain says what the split writes; kernels_aux.hip
// order_split_kernel computes it with one workgroup; the host build exports the plain one, tests/test_sky_tiles_host.py).
#pragma once
#include "device_shade.hpp"
#include "launch_plan.hpp"

namespace dr {

// a tile's word (entry code << ENTRY_SHIFT | grade, RenderParams cert_level) says that no leaf can be seen from the tile
__host__ __device__ __forceinline__ bool sky_word(uint32_t word) { return ((int)word >> ENTRY_SHIFT) == ENTRY_NONE; }
// the split's predicate over the tiles' words: a tile is kept unless it is a sky tile (load and test apart: the kernel issues a round trip's loads
// before it uses any of them)
struct SkyKeep {
  typedef uint32_t Value;
  const uint32_t* word;
  __host__ __device__ __forceinline__ Value load(int t) const { return word[t]; }
  __host__ __device__ __forceinline__ static bool keep(Value v) { return !sky_word(v); }
  __host__ __device__ __forceinline__ bool operator()(int t) const { return keep(load(t)); }
};

// What store_pixel adds for pixel (x, y) and frame `frame` of the launch when every sample's path misses (max_depth > 0: the first ray of a path
// is always shaded)
__device__ __forceinline__ void sky_pixel(const RenderParams& P, int x, int y, int frame, int& r, int& g, int& b) {
  V3 color = mk(0, 0, 0);
  Ctr c = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int s = 0; (float)s < P.spp_f; ++s) {
    Xorwow rng;
    rng.init(sample_seed(P, x, y, s, frame));
    Path path; path.atten = splat(1.0f);
    camera_ray(P, x, y, rng, path.rayo, path.raydir);
    color = color + shade_miss<false>(P, path, c);
  }
  r = f2i(color.x * 255 * P.scale); g = f2i(color.y * 255 * P.scale); b = f2i(color.z * 255 * P.scale);
}

// `count` frames from frame `first` of the launch for lane `lane` of sky tile `tile` -- pixel (lane >> 3, lane & 7) of it, as in the render kernels --
// summed in registers and written once per channel as P.accumulate says (several units of one tile: the atomic add); the cost the persistent kernel
// records for such a pixel, 0 node steps, is stored by the unit that starts at frame 0.  The one body of sky_tiles_kernel (kernels_aux.hip: the whole
// batch) and of the lean build's retiring waves (kernels_render.hip: a unit of launch_plan.hpp sky_unit); which wave runs it enters no arithmetic.
__device__ __forceinline__ void sky_tile_frames(const RenderParams& P, int tile, int lane, int first, int count, unsigned* pixel_cost) {
  const int col = tile / P.gy, by = tile - col * P.gy;
  const int x = (P.stripe_rem + col * P.stripe_mod) * 8 + (lane >> 3), y = by * 8 + (lane & 7);
  int r = 0, g = 0, b = 0;
  for (int frame = first; frame < first + count; frame++) {
    int fr, fg, fb;
    sky_pixel(P, x, y, frame, fr, fg, fb);
    r += fr; g += fg; b += fb;
  }
  int32_t* px = P.out + ((size_t)x * (size_t)P.H + (size_t)y) * 3;
  if (P.accumulate == 2) { atomicAdd(px + 0, r); atomicAdd(px + 1, g); atomicAdd(px + 2, b); }
  else if (P.accumulate) { px[0] += r; px[1] += g; px[2] += b; }
  else { px[0] = r; px[1] = g; px[2] = b; }
  if (pixel_cost && first == 0) pixel_cost[(size_t)tile * 64 + lane] = 0u;
}

}  // namespace dr
