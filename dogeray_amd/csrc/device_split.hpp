// The split of a launch's tile order: the stable partition that hands the persistent kernel's queues only the tiles a predicate keeps.  Written
// once, here, as plain C++ over a keep predicate; kernels_aux.hip order_split_kernel computes the same arrays with one workgroup, the host build
// exports this one (hk_sky_split, hk_subset_split), tests/split_cases.py restates it in numpy and tests/test_gpu_order_split.py holds the kernel
// to it.  Two predicates: device_sky.hpp SkyKeep (kept unless the tile's word says it sees no leaf; the dropped are listed) and device_adaptive.hpp FlagKeep.
#pragma once
#include "launch_plan.hpp"

namespace dr {

struct SplitCounts { int kept, dropped; };

// order (null: the identity) and region_start in the persistent kernel's format (region r owns positions [region_start[r], region_start[r + 1]) of
// the order, region_start[regions] = tiles); keep(t): tile t stays.
//   launch_order          the kept tiles, in the order they had (a stable partition: every region keeps its heavy-first, then natural order)
//   launch_region_start   2 * MAX_REGIONS + 1 ints: the starts of the compacted regions, [regions] = the kept tiles; the split counts
//                         [MAX_REGIONS + 1 + r] = 0
//   dropped_list          the dropped tiles, ascending (null: not listed)
// Returns both counts.
template <class Keep>
inline SplitCounts order_split_plain(const int* order, const int* region_start, const Keep& keep, int tiles, int regions, int* launch_order,
                                     int* launch_region_start, int* dropped_list) {
  int n_kept = 0, n_dropped = 0, r = 0;
  for (int k = 0; k < 2 * MAX_REGIONS + 1; k++) launch_region_start[k] = 0;
  for (int i = 0; i < tiles; i++) {
    while (r <= regions && region_start[r] <= i) launch_region_start[r++] = n_kept;
    const int t = order ? order[i] : i;
    if (keep(t)) launch_order[n_kept++] = t;
    if (!keep(i)) {
      if (dropped_list) dropped_list[n_dropped] = i;
      n_dropped++;
    }
  }
  while (r <= regions) launch_region_start[r++] = n_kept;
  return {n_kept, n_dropped};
}

}  // namespace dr
