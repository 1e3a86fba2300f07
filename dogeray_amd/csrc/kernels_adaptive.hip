// Adaptive sampling (dr_render_adaptive): two kernels around launches of the persistent kernel, which is not touched -- it takes the
// launch's own, shorter order / region_start pair (kernels_aux.hip order_split_kernel by the selection's flags) as it takes the sky split's.  What a pixel
// and a tile do are the bodies of device_adaptive.hpp (ad_asks, ad_tile_active, ad_fold_pixel), which run unchanged in the host build; here are the
// wave-to-tile mappings and the ballots.
//   select   a wave per tile, lane l pixel (8 col + (l >> 3), 8 by + (l & 7)) as in the render kernels: the eight lanes of a column read 96-byte runs
//            of the column-major sums, 64-byte runs of M2 and 32-byte runs of the history plane.  `ask` by ballot, its popcount against tile_pixels;
//            lane 0 stores the tile's flag (a vector store) and adds the two counts with one vector atomic per wave and field: integers, so any
//            order gives the same bits.  No LDS, no scratch.
//   add      waves stride over the positions of the compacted list, whose length they read from launch_region_start[regions] on the device (no host
//            sync between selection and launch); a lane keeps its pixel's sums and M2 in registers across the group's frames and writes sums, M2
//            and history once.
#include <hip/hip_runtime.h>

#include "device_adaptive.hpp"
#include "kernels.hpp"

namespace dr {

namespace {

__global__ __launch_bounds__(256) void adaptive_select_kernel(AdLaunch L) {
  const int tile = (int)(blockIdx.x * 4 + (threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63);
  if (tile >= L.gx * L.gy) return;
  const int asking = __popcll(__ballot(ad_asks(L, tile, lane)));
  const bool active = ad_tile_active(L, asking);
  if (lane == 0) {
    L.flags[tile] = active ? 1 : 0;
    if (active) atomicAdd(L.counts + AD_ACTIVE, 1u);
    if (asking) atomicAdd(L.counts + AD_ASKING, (unsigned)asking);
  }
}

__global__ __launch_bounds__(256) void adaptive_add_kernel(AdLaunch L, const int* __restrict__ launch_order, const int* __restrict__ launch_region_start,
                                                            int regions) {
  const int n = launch_region_start[regions], waves = (int)gridDim.x * 4, lane = (int)(threadIdx.x & 63);
  for (int i = (int)(blockIdx.x * 4 + (threadIdx.x >> 6)); i < n; i += waves) ad_fold_pixel(L, launch_order[i], lane);
}

}  // namespace

void launch_adaptive_select(hipStream_t stream, const AdLaunch& L) {
  const long long tiles = (long long)L.gx * (long long)L.gy;
  if (tiles <= 0) return;
  hipLaunchKernelGGL(adaptive_select_kernel, dim3((unsigned)((tiles + 3) / 4)), dim3(256), 0, stream, L);
}

void launch_adaptive_add(hipStream_t stream, const AdLaunch& L, const int* launch_order, const int* launch_region_start, int regions) {
  const long long tiles = (long long)L.gx * (long long)L.gy;
  if (tiles <= 0 || L.nframes <= 0) return;
  long long blocks = (tiles + 3) / 4; if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(adaptive_add_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, L, launch_order, launch_region_start, regions);
}

}  // namespace dr
