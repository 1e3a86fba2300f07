// Every crossing of a caller ray, the first K sorted (dr_trace_all_hits): a walk kernel -- one ray per lane for either tree, or the persistent one of the wide
// walk -- and a surface pass, one thread per (ray, k), for the channels beyond count, t and object.  The walks, the list and the per-ray bodies:
// device_allhits.hpp.  Per 256-thread workgroup the lanes' stacks take 16 KiB of LDS and their lists (DR_ALLHITS_MAX keys of two words) another 16 KiB,
// both lane-strided: 32 KiB, five workgroups per CU.
#include <hip/hip_runtime.h>

#include "device_allhits.hpp"
#include "device_list.hpp"
#include "kernels.hpp"
#include "../../include/dogeray_amd.h"

namespace dr {

__device__ __forceinline__ void allhits_flush(const AllHitsLaunch& A, unsigned i, int count, const unsigned* list) {
  allhits_store((size_t)i, count, A.K, list, A.slot_to_orig, A.count, A.t, A.object, A.hit);
}

// one ray per lane, each wave waiting for its slowest: either tree, short lists -- the baseline
template <bool WIDE>
__global__ __launch_bounds__(256) void allhits_plain_kernel(RenderParams P, AllHitsLaunch A) {
  __shared__ int lds_stack[WIDE ? WIDE_STACK * 256 : 1];
  __shared__ unsigned lds_list[ALLHITS_LIST_WORDS * 256];
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= A.n) return;
  int* const stack = WIDE ? lds_stack + (threadIdx.x >> 6) * (WIDE_STACK * 64) + (threadIdx.x & 63) : lds_stack;
  unsigned* const list = lds_list + (threadIdx.x >> 6) * (ALLHITS_LIST_WORDS * 64) + (threadIdx.x & 63);
  Ctr c = {0, 0, 0, 0, 0, 0, 0, 0};
  const int count = allhits_ray<WIDE, false>(P, ld3(A.origin + 3 * (size_t)i), ld3(A.dir + 3 * (size_t)i), A.tmax ? A.tmax[i] : 10000.0f, A.kind_mask, A.K, list, c, stack);
  allhits_flush(A, i, count, list);
}

// The persistent kernel (the wave loop: device_list.hpp; parameters: launch_plan.hpp): lanes refill from the ray list once REFILL_MIN of them want a ray or
// nobody walks.  A lane's list is flushed at the refill that gives it its next ray.
template <int OCC, int REFILL_MIN, int PARK>
__global__ __launch_bounds__(256, OCC) void allhits_persistent_kernel(RenderParams P, AllHitsLaunch A) {
  __shared__ int lds[4 * WIDE_STACK * 64];
  __shared__ unsigned lds_list[ALLHITS_LIST_WORDS * 256];
  const int lane = threadIdx.x & 63;
  int* const my_stack = lds + (threadIdx.x >> 6) * (WIDE_STACK * 64) + lane;
  unsigned* const my_list = lds_list + (threadIdx.x >> 6) * (ALLHITS_LIST_WORDS * 64) + lane;
  const WalkRsrc walk = wide_rsrc(P);
  const unsigned n = A.n;
  const int K = A.K, kind_mask = A.kind_mask;
  Trav tr; tr.node = LANE_REFILL; tr.best_t = 10000.0f; tr.best_slot = -1;      // (best_t stays 10000: the node step's cap on the exit distance)
  WideStack ws; ws.top = 0u; ws.sp = 0; ws.sb = 0;
  V3 o = mk(0, 0, 0), d = mk(0, 0, 0), inv = mk(0, 0, 0);
  WideRay wr = wide_ray_none();
  SignMask sg = sign_mask(inv);
  Ctr c = {0, 0, 0, 0, 0, 0, 0, 0};
  unsigned idx = 0;
  float cap = 0;
  int count = 0;
  ListFeed feed;
  for (;;) {
    const unsigned long long want = __ballot(tr.node == LANE_DONE || tr.node == LANE_REFILL);
    const unsigned long long walking = __ballot(tr.node >= 0);
    if (want != 0ull && ((int)__popcll(want) >= REFILL_MIN || walking == 0ull)) {
      if (tr.node == LANE_DONE) allhits_flush(A, idx, count, my_list);
      const bool mine = tr.node == LANE_DONE || tr.node == LANE_REFILL;
      const ListItem it = feed.take<ALLHITS_CHUNK>(want, A.cursor, n);
      if (mine) {
        if (it.ok) {
          idx = it.index;
          o = ld3(A.origin + 3 * (size_t)idx); d = ld3(A.dir + 3 * (size_t)idx);
          cap = trace_cap(A.tmax ? A.tmax[idx] : 10000.0f);
          inv = mk(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
          wr = wide_ray(o, d, inv, P.wide_pmax, P.wide_mu.e, P.wide_mu.l, P.wide_mu.v); sg = sign_mask(inv);
          trav_begin(tr); ws.top = 0u; ws.sp = 0; ws.sb = 0;
          count = 0;
          if (!(cap > 0.0f)) tr.node = LANE_DONE;      // a tmax that admits nothing: count 0, written at the next refill
        } else tr.node = it.state;
      }
      if (__ballot(tr.node != LANE_RETIRED) == 0ull) break;
    }
    list_walk_round<PARK>(walk, wr, sg, feed.exhausted, tr, ws, my_stack, c, [&](const WideRec& r) {
      allhits_wide_leaf(r, o, d, inv, sg, cap, kind_mask, K, count, my_list);
      wide_pop(tr, ws, my_stack);
    });
  }
}

// the surface pass: (origin, dir, hit) -> the channels beyond t and object, one thread per entry
__global__ __launch_bounds__(256) void allhits_surface_kernel(RenderParams P, AllHitsLaunch A) {
  const size_t e = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (e >= (size_t)A.n * (size_t)A.K) return;
  const AllHitsSurface S = {A.distance, A.material, A.normal, A.uv, A.albedo};
  allhits_surface(P, A.origin, A.dir, A.hit, A.K, e, S);
}

void launch_allhits(hipStream_t stream, const RenderParams& P, const AllHitsPlan& plan, const AllHitsLaunch& A) {
  const dim3 grid((unsigned)plan.blocks), block(256);
  if (plan.kernel == QUERY_KERNEL_PERSISTENT) {      // (A.cursor: zeroed on this stream by the caller)
    hipLaunchKernelGGL((allhits_persistent_kernel<ALLHITS_OCC, ALLHITS_REFILL_MIN, ALLHITS_PARK>), grid, block, 0, stream, P, A);
  }
  else if (plan.wide) hipLaunchKernelGGL((allhits_plain_kernel<true>), grid, block, 0, stream, P, A);
  else hipLaunchKernelGGL((allhits_plain_kernel<false>), grid, block, 0, stream, P, A);
}
void launch_allhits_surface(hipStream_t stream, const RenderParams& P, const AllHitsLaunch& A) {
  const size_t entries = (size_t)A.n * (size_t)A.K;
  hipLaunchKernelGGL(allhits_surface_kernel, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, stream, P, A);
}

}  // namespace dr
