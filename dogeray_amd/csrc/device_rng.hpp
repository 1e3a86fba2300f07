// The random numbers of the device functions: cuRAND's XORWOW, the uniform draws restated with the same roundings, and the rejection samplers.
#pragma once
#include "device_math.hpp"

namespace dr {

// ------------------------------------------------------------------ RNG: cuRAND XORWOW
// curand_init(seed, 0, 0) / curand() / curand_uniform_double() (call sites K:644,657,1065-1068)
__device__ __forceinline__ double z_plus_half_of(uint32_t x, uint32_t y) {      // Xorwow::z_plus_half() of the two outputs x, y
  const uint32_t lo = x ^ (y << 21), hi = y >> 11;
  const double d_hi = bits_double(0x45300000u, hi), d_lo = bits_double(0x43300000u, lo);
  return ((d_hi - 19342813118337666422669312.0) + d_lo) + 0.5;
}
struct Xorwow {
  uint32_t v0, v1, v2, v3, v4, d;
  __device__ __forceinline__ void init(uint64_t seed) {
    uint32_t s0 = (uint32_t)seed ^ 0xaad26b49u;
    uint32_t s1 = (uint32_t)(seed >> 32) ^ 0xf7dcefddu;
    uint32_t t0 = 1099087573u * s0;
    uint32_t t1 = 2591861531u * s1;
    d = 6615241u + t1 + t0;
    v0 = 123456789u + t0;
    v1 = 362436069u ^ t0;
    v2 = 521288629u + t1;
    v3 = 88675123u ^ t1;
    v4 = 5783321u + t0;
  }
  __device__ __forceinline__ uint32_t next() {
    uint32_t t = v0 ^ (v0 >> 2);
    v0 = v1; v1 = v2; v2 = v3; v3 = v4;
    v4 = xorwow_combine(t, v4);
    d += 362437u;
    return v4 + d;
  }
  // curand_uniform_double(): z = x ^ (y << 21) (53 bits), (double)z * 2^-53 + 2^-54.  The conversion and the arithmetic behind it are restated
  // with fewer operations and THE SAME roundings (tools/host_kernel.cpp hk_check_uniform compares them with the plain expressions):
  //  * (double)z = ((2^84 + hi * 2^32) - (2^84 + 2^52)) + (2^52 + lo), hi = z >> 32, lo = the low word: both terms are doubles whose high word is a
  //    constant and whose low word is hi / lo, and both additions are exact -- two f64 adds instead of two conversions, a scaling and an add
  //    (and no 64-bit shift);
  //  * RN(z * 2^-53 + 2^-54) = RN(z + 0.5) * 2^-53 (a power of two commutes with the rounding);
  //  * (float)(u * 2 - 1) of the unit-sphere draw = (float)fma(RN(z + 0.5), 2^-52, -1): u * 2 is exact, so the subtraction's rounding is the fma's.
  __device__ __forceinline__ double z_plus_half() {               // RN((double)z + 0.5)
    const uint32_t x = next(), y = next();      // (in this order)
    return z_plus_half_of(x, y);
  }
  __device__ __forceinline__ double uniform_double() { return z_plus_half() * 0x1p-53; }
  __device__ __forceinline__ float uniform_pm1() { return (float)__builtin_fma(z_plus_half(), 0x1p-52, -1.0); }      // (float)(uniform_double() * 2 - 1)
};

// The rejection test of K:645 / K:992 is pow(length(p), 2.0f) >= 1 with length = sqrtf(dot): l = RN(sqrt(d2)), then RN(l * l) >= 1.  Away from 1 the
// outcome is that of d2 >= 1 itself: for d2 <= 1 - 2^-20, sqrt(d2) <= 1 - 2^-21 (a float), so l <= 1 - 2^-21 and l * l <= 1 - 2^-20 + 2^-42 rounds
// below 1; for d2 >= 1 + 2^-20, sqrt(d2) >= 1 + 2^-21 - 2^-43 rounds to at least 1 + 2^-21 and l * l > 1.  Only inside that band is the correctly
// rounded square root (some fifteen instructions) really taken -- and the wave branches around it when none of its lanes is in the band.
__device__ __forceinline__ bool outside_unit(float d2) {
  const bool band = __builtin_fabsf(d2 - 1.0f) < 0x1p-20f;
  bool out = d2 >= 1;
  if (DR_WAVE_ANY(band)) {                                          // (wave-uniform)
    DR_PIN("rare: a lane within 2^-20 of the unit sphere");      // (keeps the compiler from hoisting the square root out of the branch)
    if (band) {
      const float l = __builtin_sqrtf(d2);
      out = l * l >= 1;                                           // pow(len, 2.0f)
    }
  }
  return out;
}
__device__ __forceinline__ V3 rand_in_unit_sphere(Xorwow& r) {   // K:640-648
  for (;;) {
    float x = r.uniform_pm1();
    float y = r.uniform_pm1();
    float z = r.uniform_pm1();
    V3 p = mk(x, y, z);
    if (outside_unit(dot(p, p))) continue;
    return p;
  }
}
__device__ __forceinline__ float randy(Xorwow& r) { return (float)r.uniform_double(); }   // K:651
__device__ __forceinline__ V3 rand_in_unit_disk(Xorwow& r) {     // K:988-994
  for (;;) {
    float x = randy(r) * 2 - 1;
    float y = randy(r) * 2 - 1;
    V3 p = mk(x, y, 0);
    if (outside_unit(dot(p, p))) continue;
    return p;
  }
}

// One rejection loop for a whole wave: lanes with kind 3 draw a point in the unit sphere (K:640-648: three uniforms per candidate, in double, x y z),
// lanes with kind 2 a point in the unit disk (K:988-994: two uniforms per candidate, in float), lanes with kind 0 nothing -- each lane's sequence of
// draws is exactly that of rand_in_unit_sphere / rand_in_unit_disk, but the wave runs the loop once, for as many turns as its unluckiest lane needs,
// instead of once per kind (the persistent kernel's shade / refill phase: the lanes that scatter and the lanes that start a path).
// (turns: counting builds only -- the number of candidates this lane drew; the wave runs the loop for as many turns as its unluckiest lane)
// A turn of that loop does not convert its candidate exactly.  It classifies it from the top 32 bits of each 53-bit draw -- T = y ^ (x >> 21) are the
// top 32 bits of z = x ^ (y << 21) | (y >> 11) << 32 -- as c~ = RN32(RN32((float)T) * 2^-31 - 1), and rejects it only when the approximate squared length
// says "certainly outside"; whatever is not rejected is converted exactly AFTER the loop and put to the reference's own test (outside_unit), and a lane
// whose candidate fails that test goes back into the loop.  So the sequence of draws and the accepted point are the reference's as long as
//     d2~ >= 1 + 2^-16   implies   outside_unit(d2) for the exactly converted candidate:
//  * with v = 2 (z + 0.5) 2^-53 - 1 the real number both conversions approximate: exact conversion |c - v| <= 3 * 2^-25 (sphere lanes: RN64 then RN32 of
//    fma(Z, 2^-52, -1) <= 2^-25 + 2^-52; disk lanes: RN32(u) * 2 - 1 with one more rounding <= 2^-25 when the result is below -0.5); the approximation
//    |c~ - v| <= 2^-24 ((float)T, half an ulp of 2^32, times 2^-31) + 2^-25 (the fma's rounding) + 2^-31 (the 21 bits dropped) -- so |c~ - c| < 2^-22;
//  * three coordinates of magnitude <= 1: the real sums of squares differ by less than 3 * 2 * 2^-22 < 2^-19; either float evaluation (three products <= 1,
//    two sums < 4) is within 5 * 2^-23 of its real sum; so |d2~ - d2| < 2^-19 + 2 * 5 * 2^-23 < 2^-17;
//  * hence d2~ >= 1 + 2^-16 gives d2 > 1 + 2^-17 > 1 + 2^-20, where outside_unit() is true (its own argument above).
// The accepted candidate's words are not kept through the loop: XORWOW's state IS its last five outputs (v0..v4 = w[n-4..n], output k = w[k] + d[k], d[k] =
// d - (n - k) * 362437), so the last four draws of a disk lane are rebuilt from the state and a sphere lane keeps one word, the first of its six.
// (tools/host_kernel.cpp hk_check_reject compares the loop with rand_in_unit_sphere / rand_in_unit_disk, draw for draw.)
__device__ __forceinline__ float reject_coord(uint32_t x, uint32_t y) {
  return __builtin_fmaf((float)(y ^ (x >> 21)), 0x1p-31f, -1.0f);
}
template <bool COUNT = false>
__device__ __forceinline__ V3 rand_points_merged(Xorwow& r, int kind, unsigned* turns = nullptr) {
  V3 p = mk(0, 0, 0);
  bool todo = kind != 0;
  uint32_t first = 0;
  for (;;) {
    while (todo) {
      DR_MARK("reject_turn");
      if (COUNT) (*turns)++;
      const uint32_t a = r.next(), b = r.next(), c = r.next(), e = r.next();
      first = a;
      const float x = reject_coord(a, b), y = reject_coord(c, e);
      float d2 = __builtin_fmaf(y, y, x * x);
      if (kind == 3) {
        const uint32_t f = r.next(), g = r.next();
        const float z = reject_coord(f, g);
        d2 = __builtin_fmaf(z, z, d2);
      }
      todo = d2 >= 1.0f + 0x1p-16f;
    }
    DR_MARK("reject_done");
    if (kind == 0) break;
    // the candidate's words, out of the generator's state
    const uint32_t d0 = r.d, d1 = d0 - 362437u, d2w = d1 - 362437u, d3 = d2w - 362437u, d4 = d3 - 362437u;
    const uint32_t o0 = r.v4 + d0, o1 = r.v3 + d1, o2 = r.v2 + d2w, o3 = r.v1 + d3, o4 = r.v0 + d4;
    const bool sphere = kind == 3;
    const double zx = z_plus_half_of(sphere ? first : o3, sphere ? o4 : o2), zy = z_plus_half_of(sphere ? o3 : o1, sphere ? o2 : o0);
    float x, y, z = 0.0f;
    if (sphere) {
      x = (float)__builtin_fma(zx, 0x1p-52, -1.0); y = (float)__builtin_fma(zy, 0x1p-52, -1.0);
      z = (float)__builtin_fma(z_plus_half_of(o1, o0), 0x1p-52, -1.0);
    } else {
      x = (float)(zx * 0x1p-53) * 2 - 1; y = (float)(zy * 0x1p-53) * 2 - 1;      // randy() * 2 - 1
    }
    p = mk(x, y, z);
    todo = outside_unit(dot(p, p));
    if (!todo) break;
  }
  return p;
}

}  // namespace dr
