// The host's side of dogeray_amd/csrc/device_prims.hpp: the same names in plain C++, for a "wave" of one lane.  Test / bench infrastructure
// (tools/host_kernel.cpp, tools/study_wide_walk.cpp); the product library never sees this file and has no CPU path.
#pragma once
#include "host_stubs.hpp"

namespace dr {

// ---- RNG
__device__ __forceinline__ double bits_double(uint32_t hi, uint32_t lo) {      // the double with these two words
  const uint64_t b = ((uint64_t)hi << 32) | lo;
  double r; __builtin_memcpy(&r, &b, 8);
  return r;
}
__device__ __forceinline__ uint32_t xorwow_combine(uint32_t t, uint32_t v4) { return (v4 ^ (v4 << 4)) ^ (t ^ (t << 1)); }

// ---- the wave: one lane
#define DR_WAVE_ANY(p) (p)
__device__ __forceinline__ bool first_active_lane() { return true; }
__device__ __forceinline__ bool lane_bit(unsigned long long wave_mask) { return (wave_mask & 1ull) != 0ull; }      // (the one lane is lane 0)
__device__ __forceinline__ int wave_count(unsigned long long wave_mask) { return __builtin_popcountll(wave_mask); }
__device__ __forceinline__ int wave_uniform(int v) { return v; }
#define DR_PIN(s) do {} while (0)
constexpr bool LEAF_PRIM_FIRST = false;      // the reference's order: the box, then the primitive (L counts primitives tested behind a passed box)
constexpr bool HIT_UV_CARRIED = false, HIT_FETCH_LAZY = false;      // the host's walks and renders keep the plain shade path; hk_hit_inputs names the forms itself

// ---- 128-bit loads through a buffer descriptor
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
struct WalkRsrc { const unsigned char* base; unsigned bytes; };      // a buffer descriptor's base and range; loads past the range return 0, as the hardware's do
__device__ __forceinline__ WalkRsrc make_rsrc(const void* p, uint32_t bytes) { WalkRsrc r; r.base = (const unsigned char*)p; r.bytes = bytes; return r; }
__device__ __forceinline__ u32x4 ld_unit_raw(WalkRsrc r, unsigned byte_off) {
  u32x4 v = {0u, 0u, 0u, 0u};
  if ((unsigned long long)byte_off + 16ull <= (unsigned long long)r.bytes) memcpy(&v, r.base + byte_off, 16);
  return v;
}
__device__ __forceinline__ void no_value(u32x4& v) { v = u32x4{0u, 0u, 0u, 0u}; }
__device__ __forceinline__ void pin_loads(u32x4&, u32x4&, u32x4&, u32x4&) {}
__device__ __forceinline__ unsigned one_register(unsigned v) { return v; }

// ---- three-input bit operations
__device__ __forceinline__ unsigned bit_select(unsigned if0, unsigned if1, unsigned m) { return (if0 & ~m) | (if1 & m); }
__device__ __forceinline__ unsigned bit_and_or(unsigned a, unsigned b, unsigned c) { return (a & b) | c; }
__device__ __forceinline__ unsigned bit_andn(unsigned a, unsigned b, unsigned c) { return ~a & b & c; }
__device__ __forceinline__ int lowest_bit(unsigned w) { return w ? __builtin_ctz(w) : -1; }
__device__ __forceinline__ int at_least_minus_one(int v) { return v > -1 ? v : -1; }

// ---- The four plane bytes of a word as f16 denormals: (byte0, byte2) and (byte1, byte3), each pair in one register
struct PlanePairs { unsigned even, odd; };
__device__ __forceinline__ PlanePairs plane_pairs(unsigned w) { PlanePairs p; p.even = w & 0x00ff00ffu; p.odd = (w >> 8) & 0x00ff00ffu; return p; }
__device__ __forceinline__ float plane_t(const PlanePairs& p, int k, float a, float b) {     // fma(byte_k * 2^-24, a, b), rounded once
  const unsigned h = ((k & 1) ? p.odd : p.even) >> ((k & 2) ? 16 : 0) & 0xffffu;
  return __builtin_fmaf((float)h * 0x1p-24f, a, b);
}

// ---- the camera rays' entry table
__device__ __forceinline__ void entry_min(uint32_t* p, uint32_t v) { if (v < *p) *p = v; }
// (ENTRY_MUTANT: a wrong rule on purpose -- tests/test_camera_entry_host.py shows that its cases catch each)
static thread_local int entry_mutant = 0;
#define ENTRY_MUTANT(k) (entry_mutant == (k))

}  // namespace dr
