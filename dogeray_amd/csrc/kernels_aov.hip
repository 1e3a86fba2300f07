// First-hit AOV buffers (dr_render_aov): one wave per 8x8 tile of the requested window, one pinhole ray per lane through the pixel centre,
// its closest hit and what shade_prepare forms there (device_aov.hpp aov_first_hit).  Camera rays of one tile are coherent, so the
// wave walks the tree nearly in lockstep; there is no path, no random draw and no counter.  The traversal stacks live in LDS with the layout
// of kat_hit_kernel (word k of lane l at stack[k * 64 + l]).
#include <hip/hip_runtime.h>

#include "device_wide.hpp"
#include "device_aov.hpp"
#include "kernels.hpp"
#include "../../include/dogeray_amd.h"

namespace dr {

// lane l of a tile is pixel (l & 7, l >> 3): eight neighbouring lanes write eight neighbouring words of a row of the row-major planes
template <int MODE>
__global__ __launch_bounds__(256) void aov_kernel(RenderParams P, AovLaunch A) {
  __shared__ int lds_stack[MODE == DR_TRAVERSAL_ORDERED ? ORDERED_STACK * 256 : (MODE == DR_TRAVERSAL_WIDE ? WIDE_STACK * 256 : 1)];
  const int wave = (int)(blockIdx.x * 4 + (threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63);
  const int tiles_x = (A.w + 7) >> 3;
  if (wave >= tiles_x * ((A.h + 7) >> 3)) return;
  const int wx = (wave % tiles_x) * 8 + (lane & 7), wy = (wave / tiles_x) * 8 + (lane >> 3);      // pixel inside the window
  if (wx >= A.w || wy >= A.h) return;
  AovHit a;
  if (MODE == DR_TRAVERSAL_ORDERED) {
    int* stack = lds_stack + (threadIdx.x >> 6) * (ORDERED_STACK * 64) + lane;
    auto closest = [&](V3 o, V3 d, Ctr& c) { return closest_hit_ordered<false>(P.pairs, P.prims, o, d, c, stack); };
    a = aov_first_hit(P, closest, A.focus, A.x0 + wx, A.y0 + wy);
  } else if (MODE == DR_TRAVERSAL_WIDE) {
    int* stack = lds_stack + (threadIdx.x >> 6) * (WIDE_STACK * 64) + lane;
    const WalkRsrc wide = wide_rsrc(P);
    auto closest = [&](V3 o, V3 d, Ctr& c) { return closest_hit_wide<false>(wide, P.wide_pmax, P.wide_mu.e, P.wide_mu.l, P.wide_mu.v, o, d, c, stack); };
    a = aov_first_hit(P, closest, A.focus, A.x0 + wx, A.y0 + wy);
  } else {
    const WalkRsrc walk = walk_rsrc(P);
    auto closest = [&](V3 o, V3 d, Ctr& c) { return closest_hit_threaded<false>(walk, o, d, c); };
    a = aov_first_hit(P, closest, A.focus, A.x0 + wx, A.y0 + wy);
  }
  const size_t i = (size_t)wy * (size_t)A.w + (size_t)wx;
  if (A.t) A.t[i] = a.t;
  if (A.distance) A.distance[i] = a.distance;
  if (A.depth) A.depth[i] = a.depth;
  if (A.object) A.object[i] = a.slot >= 0 ? A.slot_to_orig[a.slot] : -1;
  if (A.material) A.material[i] = a.mat;
  if (A.normal) { A.normal[3 * i] = a.normal.x; A.normal[3 * i + 1] = a.normal.y; A.normal[3 * i + 2] = a.normal.z; }
  if (A.uv) { A.uv[2 * i] = a.u; A.uv[2 * i + 1] = a.v; }
  if (A.albedo) { A.albedo[3 * i] = a.albedo.x; A.albedo[3 * i + 1] = a.albedo.y; A.albedo[3 * i + 2] = a.albedo.z; }
  if (A.dir) { A.dir[3 * i] = a.dir.x; A.dir[3 * i + 1] = a.dir.y; A.dir[3 * i + 2] = a.dir.z; }
}

void launch_aov(hipStream_t stream, const RenderParams& P, int traversal, const AovLaunch& A) {
  const long long tiles = (long long)((A.w + 7) >> 3) * (long long)((A.h + 7) >> 3);
  if (tiles <= 0) return;
  const dim3 grid((unsigned)((tiles + 3) / 4)), block(256);
  if (traversal == DR_TRAVERSAL_WIDE) hipLaunchKernelGGL((aov_kernel<DR_TRAVERSAL_WIDE>), grid, block, 0, stream, P, A);
  else if (traversal == DR_TRAVERSAL_ORDERED) hipLaunchKernelGGL((aov_kernel<DR_TRAVERSAL_ORDERED>), grid, block, 0, stream, P, A);
  else hipLaunchKernelGGL((aov_kernel<DR_TRAVERSAL_THREADED>), grid, block, 0, stream, P, A);
}

}  // namespace dr
