// First-hit AOV buffers (dr_render_aov): one wave per 8x8 tile of the requested window, one pinhole ray per lane through the pixel centre,
// its closest hit and what shade_prepare forms there (device_aov.hpp aov_first_hit).  Camera rays of one tile are coherent, so the
// wave walks the tree nearly in lockstep; there is no path, no random draw and no counter.  The traversal stacks live in LDS with the layout
// of kat_hit_kernel (word k of lane l at stack[k * 64 + l]).
#include <hip/hip_runtime.h>

#include "device_wide.hpp"
#include "device_aov.hpp"
#include "device_aov_lens.hpp"
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

// ------------------------------------------------------------------ lens-averaged AOVs (dr_render_aov_lens)
// The same tiles and stacks, N = nframes * spp camera rays per lane (device_aov_lens.hpp).  REFILL false: aov_lens_pixel's nested loop, every
// sample's walk run until all lanes are done -- the default: camera rays of a tile are coherent, and the wave runs the fold and the next sample's
// seed and camera ray ONCE per sample.  REFILL true (the wide and the threaded walk, which have a step to interleave; the ordered walk is always
// launched nested): ONE walk loop per wave; a lane whose walk has ended (LANE_DONE) folds its sample into its registers and starts its next one
// -- seed, camera_ray, wide_ray, entry at the root -- at the next turn of the loop, so no lane waits for the wave's slowest N times; but the fold
// and the seeding then run for a few lanes at a time, and that costs more than the waiting saves (12.5 ms against 9.2 ms).  A lane
// folds its own samples in order in both: the same bits.
template <int MODE, bool REFILL>
__global__ __launch_bounds__(256) void aov_lens_kernel(RenderParams P, AovLensLaunch A) {
  __shared__ int lds_stack[MODE == DR_TRAVERSAL_ORDERED ? ORDERED_STACK * 256 : (MODE == DR_TRAVERSAL_WIDE ? WIDE_STACK * 256 : 1)];
  const int wave = (int)(blockIdx.x * 4 + (threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63);
  const int tiles_x = (A.w + 7) >> 3;
  if (wave >= tiles_x * ((A.h + 7) >> 3)) return;
  const int wx = (wave % tiles_x) * 8 + (lane & 7), wy = (wave / tiles_x) * 8 + (lane >> 3);      // pixel inside the window
  const bool inside = wx < A.w && wy < A.h;
  const int x = A.x0 + wx, y = A.y0 + wy;
  AovLens r;
  if (!REFILL || MODE == DR_TRAVERSAL_ORDERED) {
    if (!inside) return;
    if (MODE == DR_TRAVERSAL_ORDERED) {
      int* stack = lds_stack + (threadIdx.x >> 6) * (ORDERED_STACK * 64) + lane;
      auto closest = [&](V3 o, V3 d, Ctr& c) { return closest_hit_ordered<false>(P.pairs, P.prims, o, d, c, stack); };
      r = aov_lens_pixel(P, closest, A.focus, x, y, A.nframes, A.spp, A.as_guides != 0);
    } else if (MODE == DR_TRAVERSAL_WIDE) {
      int* stack = lds_stack + (threadIdx.x >> 6) * (WIDE_STACK * 64) + lane;
      const WalkRsrc wide = wide_rsrc(P);
      auto closest = [&](V3 o, V3 d, Ctr& c) { return closest_hit_wide<false>(wide, P.wide_pmax, P.wide_mu.e, P.wide_mu.l, P.wide_mu.v, o, d, c, stack); };
      r = aov_lens_pixel(P, closest, A.focus, x, y, A.nframes, A.spp, A.as_guides != 0);
    } else {
      const WalkRsrc walk = walk_rsrc(P);
      auto closest = [&](V3 o, V3 d, Ctr& c) { return closest_hit_threaded<false>(walk, o, d, c); };
      r = aov_lens_pixel(P, closest, A.focus, x, y, A.nframes, A.spp, A.as_guides != 0);
    }
  } else {
    int* const stack = lds_stack + (MODE == DR_TRAVERSAL_WIDE ? (threadIdx.x >> 6) * (WIDE_STACK * 64) + lane : 0);
    const WalkRsrc rs = MODE == DR_TRAVERSAL_WIDE ? wide_rsrc(P) : walk_rsrc(P);
    AovLensSum a = aov_lens_begin();
    Trav tr; tr.node = inside ? LANE_REFILL : LANE_RETIRED; tr.best_t = 0; tr.best_slot = -1;      // a lane outside the window has no sample
    WideStack ws; ws.top = 0u; ws.sp = 0; ws.sb = 0;
    V3 o = mk(0, 0, 0), d = mk(0, 0, 0), inv = mk(0, 0, 0);
    WideRay wr = wide_ray_none();
    Ctr c = {0, 0, 0, 0, 0, 0, 0, 0};
    int k = 0, s = 0;                                                  // the lane's next sample: frame k, sample s
    for (;;) {
      const unsigned long long want = __ballot(tr.node == LANE_DONE || tr.node == LANE_REFILL);
      const unsigned long long walking = __ballot(tr.node >= 0);
      if (want == 0ull && walking == 0ull) break;
      if (want != 0ull) {
        if (tr.node == LANE_DONE || tr.node == LANE_REFILL) {
          if (tr.node == LANE_DONE) aov_lens_fold(P, A.focus, o, d, tr.best_slot < 0 ? -1.0f : tr.best_t, tr.best_slot, a);      // (closest_hit_*'s Hit)
          if (k < A.nframes) {
            aov_lens_ray(P, x, y, k, s, o, d);
            if (++s == A.spp) { s = 0; k++; }
            inv = mk(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
            if (MODE == DR_TRAVERSAL_WIDE) wr = wide_ray(o, d, inv, P.wide_pmax, P.wide_mu.e, P.wide_mu.l, P.wide_mu.v);
            trav_begin(tr); ws.top = 0u; ws.sp = 0; ws.sb = 0;
          } else tr.node = LANE_RETIRED;
        }
        if (__ballot(tr.node >= 0) == 0ull) break;
      }
      if (tr.node >= 0) {
        if (MODE == DR_TRAVERSAL_WIDE) {
          const WideRec rec = wide_fetch(rs, tr.node);
          if (tr.node & 1) wide_leaf_compute<false>(rec, o, d, inv, tr, ws, stack, c);
          else wide_node_compute<false>(rec, inv, wr, tr, ws, stack, c);
        } else trav_step<false>(rs, o, d, inv, tr, c);
      }
    }
    if (!inside) return;
    r = aov_lens_finish(a, A.nframes * A.spp, A.as_guides != 0);
  }
  const size_t i = (size_t)wy * (size_t)A.w + (size_t)wx;
  if (A.coverage) A.coverage[i] = r.coverage;
  if (A.depth) A.depth[i] = r.depth;
  if (A.distance) A.distance[i] = r.distance;
  if (A.material) A.material[i] = r.mat;
  if (A.normal) { A.normal[3 * i] = r.normal.x; A.normal[3 * i + 1] = r.normal.y; A.normal[3 * i + 2] = r.normal.z; }
  if (A.albedo) { A.albedo[3 * i] = r.albedo.x; A.albedo[3 * i + 1] = r.albedo.y; A.albedo[3 * i + 2] = r.albedo.z; }
}

template <bool REFILL>
static void launch_aov_lens_loop(hipStream_t stream, const RenderParams& P, int traversal, const AovLensLaunch& A, dim3 grid) {
  const dim3 block(256);
  if (traversal == DR_TRAVERSAL_WIDE) hipLaunchKernelGGL((aov_lens_kernel<DR_TRAVERSAL_WIDE, REFILL>), grid, block, 0, stream, P, A);
  else hipLaunchKernelGGL((aov_lens_kernel<DR_TRAVERSAL_THREADED, REFILL>), grid, block, 0, stream, P, A);
}
void launch_aov_lens(hipStream_t stream, const RenderParams& P, int traversal, int loop, const AovLensLaunch& A) {
  const long long tiles = (long long)((A.w + 7) >> 3) * (long long)((A.h + 7) >> 3);
  if (tiles <= 0) return;
  const dim3 grid((unsigned)((tiles + 3) / 4));
  if (traversal == DR_TRAVERSAL_ORDERED) hipLaunchKernelGGL((aov_lens_kernel<DR_TRAVERSAL_ORDERED, false>), grid, dim3(256), 0, stream, P, A);
  else if (loop == AOV_LENS_REFILL) launch_aov_lens_loop<true>(stream, P, traversal, A, grid);
  else launch_aov_lens_loop<false>(stream, P, traversal, A, grid);
}

}  // namespace dr
