// Adaptive sampling (dr_render_adaptive): three kernels around launches of the persistent kernel, which is not touched -- it takes the
// launch's own, shorter order / region_start pair as it takes the sky split's.  What a pixel and a tile do are the bodies of device_adaptive.hpp
// (ad_asks, ad_tile_active, ad_fold_pixel; subset_split_plain says what the split writes), which run unchanged in the host build; here are the
// wave-to-tile mappings, the ballots and the scan.
//   select   a wave per tile, lane l pixel (8 col + (l >> 3), 8 by + (l & 7)) as in the render kernels: the eight lanes of a column read 96-byte runs
//            of the column-major sums, 64-byte runs of M2 and 32-byte runs of the history plane.  `ask` by ballot, its popcount against tile_pixels;
//            lane 0 stores the tile's flag (a vector store) and adds the two counts with one vector atomic per wave and field: integers, so any
//            order gives the same bits.  No LDS, no scratch.
//   split    one workgroup: the stable partition of the launch's order by the flags, as sky_split_kernel (kernels_aux.hip) makes its own by the tiles'
//            words -- wave w owns a contiguous range of positions and walks it twice, counting, then placing through ballots and prefix counts.
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

// own: the region starts of the identity order (order null)
struct SubsetRegions { int start[MAX_REGIONS + 1]; };
__global__ __launch_bounds__(1024) void subset_split_kernel(const int* __restrict__ order, const int* __restrict__ region_start, SubsetRegions own,
                                                             const uint8_t* __restrict__ flag, int ntiles, int regions, int* __restrict__ launch_order,
                                                             int* __restrict__ launch_region_start) {
  constexpr int WAVES = 16;
  __shared__ int rs[MAX_REGIONS + 1];
  __shared__ unsigned kept_cnt[WAVES];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (tid <= MAX_REGIONS) {
    int v = ntiles;
    if (tid <= regions) {
      if (order) v = region_start[tid];
      else {
#pragma unroll
        for (int k = 0; k <= MAX_REGIONS; k++) if (tid == k) v = own.start[k];
      }
    }
    rs[tid] = v;
  }
  if (tid > regions && tid < 2 * MAX_REGIONS + 1) launch_region_start[tid] = 0;      // (the split counts among them: no tile is handed out in parts)
  __syncthreads();
  const int per = ((ntiles + WAVES - 1) / WAVES + 63) & ~63;
  const int w0 = w * per < ntiles ? w * per : ntiles, w1 = w0 + per < ntiles ? w0 + per : ntiles;
  auto mbcnt = [](unsigned long long m) { return (unsigned)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u)); };
  // body(i, t, kept): position i of the order holds tile t, which is (not) kept; whole waves come here, i >= w1 in the lanes past the range
  auto for_range = [&](auto&& body) {
    for (int g0 = w0; g0 < w1; g0 += 64) {
      const int i = g0 + lane;
      const int t = i < w1 ? (order ? order[i] : i) : -1;
      body(i, t, (unsigned)t < (unsigned)ntiles && flag[t] != 0);
    }
  };
  {
    unsigned n = 0;
    for_range([&](int, int, bool kept) { n += (unsigned)__popcll(__ballot(kept)); });
    if (lane == 0) kept_cnt[w] = n;
  }
  __syncthreads();
  unsigned base = 0, total = 0;
  for (int k = 0; k < WAVES; k++) {
    if (k < w) base += kept_cnt[k];
    total += kept_cnt[k];
  }
  for_range([&](int i, int t, bool kept) {
    const unsigned long long b = __ballot(kept);
    const unsigned p = base + mbcnt(b);                      // kept tiles in front of position i
    if (i < w1)
      for (int r = 0; r <= regions; r++) if (i == rs[r]) launch_region_start[r] = (int)p;
    if (kept) launch_order[p] = t;
    base += (unsigned)__popcll(b);
  });
  if (tid <= regions && rs[tid] >= ntiles) launch_region_start[tid] = (int)total;      // (the end, and regions that start there)
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

void launch_subset_split(hipStream_t stream, const int* order, const int* region_start, const int* own_region_start, const uint8_t* flag, int tiles, int regions,
                         int* launch_order, int* launch_region_start) {
  if (tiles <= 0) return;
  SubsetRegions own;
  for (int r = 0; r <= MAX_REGIONS; r++) own.start[r] = own_region_start[r];
  hipLaunchKernelGGL(subset_split_kernel, dim3(1), dim3(1024), 0, stream, order, order ? region_start : nullptr, own, flag, tiles, regions, launch_order,
                     launch_region_start);
}

void launch_adaptive_add(hipStream_t stream, const AdLaunch& L, const int* launch_order, const int* launch_region_start, int regions) {
  const long long tiles = (long long)L.gx * (long long)L.gy;
  if (tiles <= 0 || L.nframes <= 0) return;
  long long blocks = (tiles + 3) / 4; if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(adaptive_add_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, L, launch_order, launch_region_start, regions);
}

}  // namespace dr
