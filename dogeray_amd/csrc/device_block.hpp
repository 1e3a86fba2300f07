// What the one-workgroup kernels of kernels_aux.hip (tile_order_kernel, order_split_kernel) share: how the waves of a block divide a range of items
// among themselves, and a lane's rank in a ballot.  Includes nothing.
#pragma once

namespace dr {

// Wave w of `waves` owns the contiguous items [w0, w1) of n: equal ranges of whole 64-item groups, walked 64 at a time with lane l on item g + l
// (the last waves' ranges may be empty, the last non-empty one ragged)
struct WaveRange { int w0, w1; };
__device__ __forceinline__ WaveRange wave_range(int n, int waves, int w) {
  const int per = ((n + waves - 1) / waves + 63) & ~63;
  const int w0 = w * per < n ? w * per : n, w1 = w0 + per < n ? w0 + per : n;
  return {w0, w1};
}

// the lanes below this one whose bit is set in the ballot m
__device__ __forceinline__ unsigned lanes_before(unsigned long long m) {
  return (unsigned)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

}  // namespace dr
