// Nearest-surface point queries (dr_query_nearest): a walk kernel, one query per lane -- the 4-way records on the ray walk's per-lane LDS stack where
// the scene has them, the threaded links otherwise -- and a finishing pass, one thread per query, for the nearest point, its barycentrics and the
// material.  The walks, the pruning rule and the per-query bodies: device_nearest.hpp.
#include <hip/hip_runtime.h>

#include "device_nearest.hpp"
#include "kernels.hpp"

namespace dr {

template <bool WIDE>
__global__ __launch_bounds__(256) void nearest_walk_kernel(RenderParams P, NearestLaunch N) {
  __shared__ int lds_stack[WIDE ? WIDE_STACK * 256 : 1];
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= N.n) return;
  int* const stack = WIDE ? lds_stack + (threadIdx.x >> 6) * (WIDE_STACK * 64) + (threadIdx.x & 63) : lds_stack;
  Ctr c = {0, 0, 0, 0, 0, 0, 0, 0};
  nearest_query<WIDE, false>(P, N, i, c, stack);
}

__global__ __launch_bounds__(256) void nearest_finish_kernel(RenderParams P, NearestLaunch N) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= N.n) return;
  nearest_finish(P, N, i);
}

void launch_nearest(hipStream_t stream, const RenderParams& P, const NearestPlan& plan, const NearestLaunch& N) {
  const dim3 grid((unsigned)plan.blocks), block(256);
  if (plan.wide) hipLaunchKernelGGL((nearest_walk_kernel<true>), grid, block, 0, stream, P, N);
  else hipLaunchKernelGGL((nearest_walk_kernel<false>), grid, block, 0, stream, P, N);
}
void launch_nearest_finish(hipStream_t stream, const RenderParams& P, const NearestPlan& plan, const NearestLaunch& N) {
  hipLaunchKernelGGL(nearest_finish_kernel, dim3((unsigned)plan.blocks), dim3(256), 0, stream, P, N);
}

}  // namespace dr
