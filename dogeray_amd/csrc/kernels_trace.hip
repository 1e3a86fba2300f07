// Ray queries on caller rays (dr_trace_rays): closest hit below a per-ray tmax and occlusion (any hit).  A trace kernel -- the persistent one of the wide
// walk, or one ray per lane for every traversal -- that reads the caller's origin / dir / tmax arrays as they are and holds no shading state (the walk is bound
// by VALU issue and the texture addressers), and a surface pass, one thread per ray, for the channels beyond t and object.  The walks: device_trace.hpp.
#include <hip/hip_runtime.h>

#include "device_trace.hpp"
#include "device_list.hpp"
#include "device_aov.hpp"
#include "kernels.hpp"
#include "../../include/dogeray_amd.h"

namespace dr {

// what a finished ray leaves behind (the walk's best against the ray's cap: device_trace.hpp trace_result); every pointer is wave-uniform
__device__ __forceinline__ void trace_store(const TraceLaunch& T, unsigned i, Hit h) {
  const bool hit = h.slot >= 0;
  if (T.t) T.t[i] = h.t;
  if (T.object) T.object[i] = hit ? T.slot_to_orig[h.slot] : -1;
  if (T.occluded) T.occluded[i] = hit ? 1 : 0;
  if (T.hit) { T.hit[2 * (size_t)i] = __float_as_uint(h.t); T.hit[2 * (size_t)i + 1] = (unsigned)h.slot; }
}

// The persistent kernel (the wave loop: device_list.hpp; parameters: launch_plan.hpp): lanes refill from the ray list once REFILL_MIN of them want a ray or
// nobody walks; a finished lane's result is written at the refill that gives it its next ray.
// ANY: a lane whose ray holds a primitive at t <= its cap is LANE_DONE at once and takes the next ray at the next refill.
template <bool ANY, int OCC, int REFILL_MIN, int PARK>
__global__ __launch_bounds__(256, OCC) void trace_persistent_kernel(RenderParams P, TraceLaunch T) {
  __shared__ int lds[4 * WIDE_STACK * 64];
  const int lane = threadIdx.x & 63;
  int* const my_stack = lds + (threadIdx.x >> 6) * (WIDE_STACK * 64) + lane;
  const WalkRsrc walk = wide_rsrc(P);
  const unsigned n = T.n;
  Trav tr; tr.node = LANE_REFILL; tr.best_t = 0; tr.best_slot = -1;      // LANE_REFILL: wants a ray; LANE_DONE: result not written yet (device_walk.hpp)
  WideStack ws; ws.top = 0u; ws.sp = 0; ws.sb = 0;
  V3 o = mk(0, 0, 0), d = mk(0, 0, 0), inv = mk(0, 0, 0);
  WideRay wr = wide_ray_none();
  SignMask sg = sign_mask(inv);
  Ctr c = {0, 0, 0, 0, 0, 0, 0, 0};
  unsigned idx = 0;
  float cap = 0;
  ListFeed feed;
  for (;;) {
    const unsigned long long want = __ballot(tr.node == LANE_DONE || tr.node == LANE_REFILL);
    const unsigned long long walking = __ballot(tr.node >= 0);
    if (want != 0ull && ((int)__popcll(want) >= REFILL_MIN || walking == 0ull)) {
      if (tr.node == LANE_DONE) trace_store(T, idx, trace_result(tr.best_t, tr.best_slot, cap));
      const bool mine = tr.node == LANE_DONE || tr.node == LANE_REFILL;
      const ListItem it = feed.take<TRACE_CHUNK>(want, T.cursor, n);
      if (mine) {
        if (it.ok) {
          idx = it.index;
          o = ld3(T.origin + 3 * (size_t)idx); d = ld3(T.dir + 3 * (size_t)idx);
          cap = trace_cap(T.tmax ? T.tmax[idx] : 10000.0f);
          inv = mk(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
          wr = wide_ray(o, d, inv, P.wide_pmax, P.wide_mu.e, P.wide_mu.l, P.wide_mu.v); sg = sign_mask(inv);
          trav_begin(tr); ws.top = 0u; ws.sp = 0; ws.sb = 0;
          if (!(cap > 0.0f)) tr.node = LANE_DONE;      // a tmax that admits nothing: a miss, written at the next refill
        } else tr.node = it.state;
      }
      if (__ballot(tr.node != LANE_RETIRED) == 0ull) break;
    }
    list_walk_round<PARK>(walk, wr, sg, feed.exhausted, tr, ws, my_stack, c, [&](const WideRec& r) {
      wide_leaf_compute<false>(r, o, d, inv, sg, tr, ws, my_stack, c);
      if (ANY && tr.best_slot >= 0 && tr.best_t <= cap) tr.node = LANE_DONE;
    });
  }
}

// one ray per lane, each wave waiting for its slowest, in the shape of kat_hit_kernel: every traversal, scenes without a wide tree, short lists
template <int MODE, bool ANY>
__global__ __launch_bounds__(256) void trace_plain_rays_kernel(RenderParams P, TraceLaunch T) {
  __shared__ int lds_stack[MODE == DR_TRAVERSAL_ORDERED ? ORDERED_STACK * 256 : (MODE == DR_TRAVERSAL_WIDE ? WIDE_STACK * 256 : 1)];
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= T.n) return;
  int* stack = lds_stack;
  if (MODE == DR_TRAVERSAL_ORDERED) stack = lds_stack + (threadIdx.x >> 6) * (ORDERED_STACK * 64) + (threadIdx.x & 63);
  else if (MODE == DR_TRAVERSAL_WIDE) stack = lds_stack + (threadIdx.x >> 6) * (WIDE_STACK * 64) + (threadIdx.x & 63);
  Ctr c = {0, 0, 0, 0, 0, 0, 0, 0};
  const Hit h = trace_ray<MODE, false, ANY>(P, ld3(T.origin + 3 * (size_t)i), ld3(T.dir + 3 * (size_t)i), T.tmax ? T.tmax[i] : 10000.0f, c, stack);
  trace_store(T, i, h);
}

// the surface pass: (origin, dir, hit) -> the channels beyond t and object
__global__ __launch_bounds__(256) void trace_surface_kernel(RenderParams P, TraceLaunch T) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= T.n) return;
  const AovHit a = ray_surface(P, ld3(T.origin + 3 * (size_t)i), ld3(T.dir + 3 * (size_t)i), __uint_as_float(T.hit[2 * (size_t)i]), (int)T.hit[2 * (size_t)i + 1]);
  if (T.distance) T.distance[i] = a.distance;
  if (T.material) T.material[i] = a.mat;
  if (T.normal) { T.normal[3 * (size_t)i] = a.normal.x; T.normal[3 * (size_t)i + 1] = a.normal.y; T.normal[3 * (size_t)i + 2] = a.normal.z; }
  if (T.uv) { T.uv[2 * (size_t)i] = a.u; T.uv[2 * (size_t)i + 1] = a.v; }
  if (T.albedo) { T.albedo[3 * (size_t)i] = a.albedo.x; T.albedo[3 * (size_t)i + 1] = a.albedo.y; T.albedo[3 * (size_t)i + 2] = a.albedo.z; }
}

template <bool ANY>
static void launch_trace_mode(hipStream_t stream, const RenderParams& P, const TracePlan& plan, const TraceLaunch& T) {
  const dim3 grid((unsigned)plan.blocks), block(256);
  if (plan.kernel == QUERY_KERNEL_PERSISTENT) {      // (T.cursor: zeroed on this stream by the caller)
    hipLaunchKernelGGL((trace_persistent_kernel<ANY, TRACE_OCC, TRACE_REFILL_MIN, TRACE_PARK>), grid, block, 0, stream, P, T);
  }
  else if (plan.traversal == DR_TRAVERSAL_WIDE) hipLaunchKernelGGL((trace_plain_rays_kernel<DR_TRAVERSAL_WIDE, ANY>), grid, block, 0, stream, P, T);
  else if (plan.traversal == DR_TRAVERSAL_ORDERED) hipLaunchKernelGGL((trace_plain_rays_kernel<DR_TRAVERSAL_ORDERED, ANY>), grid, block, 0, stream, P, T);
  else hipLaunchKernelGGL((trace_plain_rays_kernel<DR_TRAVERSAL_THREADED, ANY>), grid, block, 0, stream, P, T);
}
void launch_trace(hipStream_t stream, const RenderParams& P, const TracePlan& plan, bool any, const TraceLaunch& T) {
  if (any) launch_trace_mode<true>(stream, P, plan, T);
  else launch_trace_mode<false>(stream, P, plan, T);
}
void launch_trace_surface(hipStream_t stream, const RenderParams& P, const TraceLaunch& T) {
  hipLaunchKernelGGL(trace_surface_kernel, dim3((T.n + 255u) / 256u), dim3(256), 0, stream, P, T);
}

}  // namespace dr
