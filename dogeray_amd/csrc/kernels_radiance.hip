// Radiance along caller rays (dr_trace_radiance): raycolor's bounce loop (device_shade.hpp trace_path) on the caller's rays, the samples of a ray
// summed in float.  One ray per lane for every traversal -- the kernel that makes the call complete --, and the persistent kernel of the wide walk,
// a wave's lanes a pool of path slots that refill from the ray list.  The per-ray body both must agree with: device_radiance.hpp radiance_ray.
#include <hip/hip_runtime.h>

#include "device_core.hpp"
#include "device_radiance.hpp"
#include "device_list.hpp"
#include "kernels.hpp"
#include "../../include/dogeray_amd.h"

namespace dr {

// one ray per lane in the shape of trace_plain_rays_kernel, the closest-hit functors of render_kernel: every walk carries the margin of a scattered
// ray from the root (the rays are the caller's: no camera certificate, no entry table).  A wave waits for its longest ray.
template <int MODE>
__global__ __launch_bounds__(256) void radiance_plain_kernel(RenderParams P, RadianceLaunch R) {
  __shared__ int lds_stack[MODE == DR_TRAVERSAL_ORDERED ? ORDERED_STACK * 256 : (MODE == DR_TRAVERSAL_WIDE ? WIDE_STACK * 256 : 1)];
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= R.n) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (MODE == DR_TRAVERSAL_ORDERED) {
    int* stack = lds_stack + wave * (ORDERED_STACK * 64) + lane;
    auto closest = [&](V3 o, V3 d, Ctr& cc) { return closest_hit_ordered<false>(P.pairs, P.prims, o, d, cc, stack); };
    radiance_ray(P, R, i, closest);
  } else if (MODE == DR_TRAVERSAL_WIDE) {
    const WalkRsrc wide = wide_rsrc(P);
    int* stack = lds_stack + wave * (WIDE_STACK * 64) + lane;
    auto closest = [&](V3 o, V3 d, Ctr& cc) { return closest_hit_wide<false>(wide, P.wide_pmax, P.wide_mu.e, P.wide_mu.l, P.wide_mu.v, o, d, cc, stack); };
    radiance_ray(P, R, i, closest);
  } else {
    const WalkRsrc walk = walk_rsrc(P);
    auto closest = [&](V3 o, V3 d, Ctr& cc) { return closest_hit_threaded<false>(walk, o, d, cc); };
    radiance_ray(P, R, i, closest);
  }
}

// The persistent kernel (the wave loop: device_list.hpp; parameters: launch_plan.hpp): a wave's lanes are a pool of PATH slots.  A lane keeps its path
// across bounces and the spp samples of its ray one after another -- so a ray's samples are summed in sample order, on one lane --, and takes a
// new ray from the list only when the last sample's path has ended: emissive hit, miss, or depth exhausted.  Once REFILL_MIN lanes have finished their
// walk or want a ray (or nobody walks) the phase runs: the finished lanes shade -- shade_hit / shade_miss as trace_path calls them, each lane its own
// draws --, then the lanes without a ray refill.
// Lane states (tr.node): >= 0 walking; LANE_DONE walk finished, to be shaded; LANE_REFILL wants a ray; LANE_RETIRED.  Every state reaches
// LANE_RETIRED: a walk ends (the walks of trace_persistent_kernel); a LANE_DONE lane leaves the phase walking again with depth + 1 <= max_depth or
// with sample + 1 <= spp, or as LANE_REFILL; a LANE_REFILL lane leaves it with a ray, retired (the list is used up), or -- its wave's chunk ran
// out in the middle of the request -- as it is, and the next phase starts with a new chunk.  The phase cannot starve: while fewer than REFILL_MIN
// lanes wait the others walk, each step brings one of them closer to LANE_DONE, and with nobody walking the phase runs for any number of waiters.
template <int OCC, int REFILL_MIN, int PARK>
__global__ __launch_bounds__(256, OCC) void radiance_persistent_kernel(RenderParams P, RadianceLaunch R) {
  __shared__ int lds[4 * WIDE_STACK * 64];
  const int lane = threadIdx.x & 63;
  int* const my_stack = lds + (threadIdx.x >> 6) * (WIDE_STACK * 64) + lane;
  const WalkRsrc walk = wide_rsrc(P);
  const unsigned n = R.n;
  Trav tr; tr.node = LANE_REFILL; tr.best_t = 0; tr.best_slot = -1;
  WideStack ws; ws.top = 0u; ws.sp = 0; ws.sb = 0;
  Path path; path.rayo = mk(0, 0, 0); path.raydir = mk(0, 0, 0); path.atten = mk(0, 0, 0);
  V3 inv = mk(0, 0, 0), sum = mk(0, 0, 0);
  WideRay wr = wide_ray_none();
  SignMask sg = sign_mask(inv);
  Ctr c = {0, 0, 0, 0, 0, 0, 0, 0};
  Xorwow rng; rng.init(0);
  unsigned idx = 0;
  int sample = 0, depth = 0, bounces = 0;      // of ray idx: the sample under way, its closest-hit queries so far, those of all samples
  ListFeed feed;
  for (;;) {
    const unsigned long long want = __ballot(tr.node == LANE_DONE || tr.node == LANE_REFILL);
    const unsigned long long walking = __ballot(tr.node >= 0);
    if (want != 0ull && ((int)__popcll(want) >= REFILL_MIN || walking == 0ull)) {
      bool begin = false, go = false;      // the lane starts a sample of ray idx / a walk along its path
      if (tr.node == LANE_DONE) {          // one turn of trace_path's loop behind its closest()
        const float t = tr.best_slot < 0 ? -1.0f : tr.best_t;
        V3 result = mk(0, 0, 0);
        if (t > 0.0f) {
          V3 emitted;
          if (!shade_hit<false>(P, path, t, tr.best_slot, rng, c, emitted)) result = emitted;
          else go = depth < P.max_depth;     // (depth exhausted: the path ends with 0)
        } else result = shade_miss<false>(P, path, c);
        if (!go) {
          sum = sum + result;
          sample++;
          if (sample < R.spp) begin = true;
          else { radiance_store(R, idx, sum, bounces); tr.node = LANE_REFILL; }
        }
      }
      const bool mine = tr.node == LANE_REFILL;
      const unsigned long long asking = __ballot(mine);
      if (asking != 0ull) {
        const ListItem it = feed.take<RADIANCE_CHUNK>(asking, R.cursor, n);
        if (mine) {
          if (it.ok) { idx = it.index; sample = 0; bounces = 0; sum = mk(0, 0, 0); begin = true; }
          else tr.node = it.state;
        }
      }
      if (begin) {
        radiance_begin(R, idx, sample, rng);
        path.rayo = ld3(R.origin + 3 * (size_t)idx); path.raydir = ld3(R.dir + 3 * (size_t)idx); path.atten = splat(1.0f);
        depth = 0; go = true;
      }
      if (go) {
        inv = mk(1.0f / path.raydir.x, 1.0f / path.raydir.y, 1.0f / path.raydir.z);
        wr = wide_ray(path.rayo, path.raydir, inv, P.wide_pmax, P.wide_mu.e, P.wide_mu.l, P.wide_mu.v); sg = sign_mask(inv);
        trav_begin(tr); ws.top = 0u; ws.sp = 0; ws.sb = 0;
        depth++; bounces++;
      }
      if (__ballot(tr.node != LANE_RETIRED) == 0ull) break;
    }
    list_walk_round<PARK>(walk, wr, sg, feed.exhausted, tr, ws, my_stack, c,
                          [&](const WideRec& r) { wide_leaf_compute<false>(r, path.rayo, path.raydir, inv, sg, tr, ws, my_stack, c); });
  }
}

void launch_radiance(hipStream_t stream, const RenderParams& P, const RadiancePlan& plan, const RadianceLaunch& R) {
  const dim3 grid((unsigned)plan.blocks), block(256);
  if (plan.kernel == QUERY_KERNEL_PERSISTENT) {      // (R.cursor: zeroed on this stream by the caller)
    hipLaunchKernelGGL((radiance_persistent_kernel<RADIANCE_OCC, RADIANCE_REFILL_MIN, RADIANCE_PARK>), grid, block, 0, stream, P, R);
  }
  else if (plan.traversal == DR_TRAVERSAL_WIDE) hipLaunchKernelGGL((radiance_plain_kernel<DR_TRAVERSAL_WIDE>), grid, block, 0, stream, P, R);
  else if (plan.traversal == DR_TRAVERSAL_ORDERED) hipLaunchKernelGGL((radiance_plain_kernel<DR_TRAVERSAL_ORDERED>), grid, block, 0, stream, P, R);
  else hipLaunchKernelGGL((radiance_plain_kernel<DR_TRAVERSAL_THREADED>), grid, block, 0, stream, P, R);
}

}  // namespace dr
