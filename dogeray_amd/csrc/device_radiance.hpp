// Radiance along caller rays (dr_trace_radiance): the seed rule, the skip, the sample loop, the sum and the bounce count of one ray, over trace_path
// (device_shade.hpp: raycolor K:787-982) and a closest-hit functor.  Host and device: tools/host_kernel.cpp hk_radiance loops radiance_ray.
#pragma once
#include "device_launch.h"
#include "device_shade.hpp"

namespace dr {

// Sample s of ray i: Xorwow::init(S_i + s * 0x9E3779B97F4A7C15), S_i = seed[i] or base_seed + i (64-bit wrapping) -- sample_seed's sample term
// (K:1065) with the caller's word in place of the pixel's --, then skip[i] outputs discarded (a negative skip discards none)
__device__ __forceinline__ uint64_t radiance_seed(const RadianceLaunch& R, unsigned i, int s) {
  const uint64_t S = R.seed ? R.seed[i] : R.base_seed + (uint64_t)i;
  return S + (uint64_t)s * 0x9E3779B97F4A7C15ull;
}
__device__ __forceinline__ void radiance_begin(const RadianceLaunch& R, unsigned i, int s, Xorwow& rng) {
  rng.init(radiance_seed(R, i, s));
  const int skip = R.skip ? R.skip[i] : 0;
  for (int k = 0; k < skip; k++) (void)rng.next();
}

// what a finished ray leaves behind (every pointer is wave-uniform)
__device__ __forceinline__ void radiance_store(const RadianceLaunch& R, unsigned i, V3 sum, int bounces) {
  if (R.radiance) { float* out = R.radiance + 3 * (size_t)i; out[0] = sum.x; out[1] = sum.y; out[2] = sum.z; }
  if (R.bounces) R.bounces[i] = bounces;
}

// Ray i: render_pixel's sample loop (K:1062-1078: color = color + raycolor(...), from 0, in sample order) on the caller's ray instead of a camera
// ray, neither divided by the samples nor quantised; bounces = the closest() calls of all samples.  P: the scene, max_depth, bgint, backtex.
template <class Closest>
__device__ __forceinline__ void radiance_ray(const RenderParams& P, const RadianceLaunch& R, unsigned i, const Closest& closest) {
  const V3 origin = ld3(R.origin + 3 * (size_t)i), dir = ld3(R.dir + 3 * (size_t)i);
  int bounces = 0;
  auto counted = [&](V3 o, V3 d, Ctr& cc) { bounces++; return closest(o, d, cc); };
  Ctr c = {0, 0, 0, 0, 0, 0, 0, 0};
  V3 sum = mk(0, 0, 0);
  for (int s = 0; s < R.spp; s++) {
    Xorwow rng;
    radiance_begin(R, i, s, rng);
    sum = sum + trace_path<false>(P, counted, origin, dir, rng, c);
  }
  radiance_store(R, i, sum, bounces);
}

}  // namespace dr
