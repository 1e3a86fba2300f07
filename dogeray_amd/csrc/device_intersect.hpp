// The intersection tests of the device functions: the slab test on a box, triangle and sphere, a primitive record, and the leaf's side of the pruning rule.
#pragma once
#include "device_layout.h"
#include "device_math.hpp"

namespace dr {

// ------------------------------------------------------------------ intersection
// Which plane of a box a ray meets first depends on the sign of 1/direction only (aabb2's swap, K:262-266).  SignCmp decides by comparing, as
// the reference does.  SignMask (persistent kernel) keeps the outcome of those three comparisons as per-lane words, all ones or all zeros,
// rebuilt whenever the lane's ray changes: a select is then (if_pos & ~m) | (if_neg & m), ONE v_bitop3_b32 -- which issues in 2.4 SIMD cycles
// where the compare and the v_cndmask take 4.2 each (tools/valu_rate.hip): 14 instead of 38 cycles per node step and per leaf step.
struct SignCmp {
  V3 inv;
  __device__ __forceinline__ unsigned sel(int axis, unsigned if_pos, unsigned if_neg) const { return (axis == 0 ? inv.x : axis == 1 ? inv.y : inv.z) < 0.0f ? if_neg : if_pos; }
};
struct SignMask {
  unsigned x, y, z;
  __device__ __forceinline__ unsigned sel(int axis, unsigned if_pos, unsigned if_neg) const {
    const unsigned m = axis == 0 ? x : axis == 1 ? y : z;
    return bit_select(if_pos, if_neg, m);      // m ? if_neg : if_pos, bit by bit (written out, the compiler splits the expression into three operations)
  }
};
__device__ __forceinline__ SignMask sign_mask(V3 inv) {
  SignMask g; g.x = inv.x < 0.0f ? 0xffffffffu : 0u; g.y = inv.y < 0.0f ? 0xffffffffu : 0u; g.z = inv.z < 0.0f ? 0xffffffffu : 0u;
  return g;
}
// aabb2 K:244-274 with the reciprocal direction hoisted out of the node loop (same divide,
// same operands) and the per-axis early return folded into one final comparison: t_min only
// grows, t_max only shrinks and neither can become NaN, so "t_max <= t_min after some axis"
// and "t_max <= t_min after the last axis" are the same predicate.
// The reference swaps (t0, t1) when invD < 0, i.e. the plane entered first is max for a
// negative direction: select the planes first (same products afterwards).  "x > m ? x : m" with
// m never NaN is fmax(x, m) (a NaN x is ignored either way; the sign of a zero result feeds
// comparisons only), so the three-axis chain folds into max3 / min3.
template <class Sign>
__device__ __forceinline__ bool slab_sel(V3 o, V3 inv, const Sign& sg, const float mn[3], const float mx[3], float& dist) {      // slab() with the planes chosen by sg
  auto pf = [&sg](int axis, float if_pos, float if_neg) { return __uint_as_float(sg.sel(axis, __float_as_uint(if_pos), __float_as_uint(if_neg))); };
  float nx = pf(0, mn[0], mx[0]), fx = pf(0, mx[0], mn[0]);
  float ny = pf(1, mn[1], mx[1]), fy = pf(1, mx[1], mn[1]);
  float nz = pf(2, mn[2], mx[2]), fz = pf(2, mx[2], mn[2]);
  float t0x = (nx - o.x) * inv.x, t1x = (fx - o.x) * inv.x;
  float t0y = (ny - o.y) * inv.y, t1y = (fy - o.y) * inv.y;
  float t0z = (nz - o.z) * inv.z, t1z = (fz - o.z) * inv.z;
  float t_min = __builtin_fmaxf(__builtin_fmaxf(__builtin_fmaxf(t0x, 0.0f), t0y), t0z);
  float t_max = __builtin_fminf(__builtin_fminf(__builtin_fminf(t1x, 10000.0f), t1y), t1z);
  dist = t_min;
  return t_max > t_min;
}
__device__ __forceinline__ bool slab(V3 o, V3 inv, const float mn[3], const float mx[3], float& dist) {      // the planes chosen by comparing, as the reference does
  SignCmp sg{inv};
  return slab_sel(o, inv, sg, mn, mx, dist);
}

// hit_tri K:277-313 on {v0, e1 = v1 - v0, e2 = v2 - v0}; returns t or -1.
// 1.0/a is a double division narrowed to float in the reference; narrowing a correctly
// rounded double quotient of two floats equals the correctly rounded float quotient.
__device__ __forceinline__ float tri_hit(V3 ro, V3 rd, V3 v0, V3 e1, V3 e2) {
  const float EPS = 0.0001f;
  V3 h = cross(rd, e2);
  float a = dot(e1, h);
  if (a > -EPS && a < EPS) return -1.0f;
  float f = 1.0f / a;
  V3 s = ro - v0;
  float u = f * dot(s, h);
  if (u < 0.0f || u > 1.0f) return -1.0f;
  V3 q = cross(s, e1);
  float v = f * dot(rd, q);
  if (v < 0.0f || u + v > 1.0f) return -1.0f;
  float t = f * dot(e2, q);
  return t > EPS ? t : -1.0f;
}
// The same test, which also hands out the barycentrics u, v as it forms them: they mean something only when the result is > 0 (a test that returns
// early leaves them as they were: no select on the way out).  They are the ux, uy that surface_normal (device_surface.hpp) forms from the same ray and
// the same v0, e1, e2, bit for bit: h, a, f, s, q here are its pvec, det, invDet, tvec, qvec, and a product of two floats does not depend on the order of
// its factors (tests/test_hit_inputs_host.py compares the words).
__device__ __forceinline__ float tri_hit(V3 ro, V3 rd, V3 v0, V3 e1, V3 e2, float& u_out, float& v_out) {
  const float EPS = 0.0001f;
  V3 h = cross(rd, e2);
  float a = dot(e1, h);
  if (a > -EPS && a < EPS) return -1.0f;
  float f = 1.0f / a;
  V3 s = ro - v0;
  float u = f * dot(s, h);
  u_out = u;
  if (u < 0.0f || u > 1.0f) return -1.0f;
  V3 q = cross(s, e1);
  float v = f * dot(rd, q);
  v_out = v;
  if (v < 0.0f || u + v > 1.0f) return -1.0f;
  float t = f * dot(e2, q);
  return t > EPS ? t : -1.0f;
}

// hit_sphere K:316-333
__device__ __forceinline__ float sphere_hit(V3 c, float radius, V3 o, V3 d) {
  V3 oc = o - c;
  float ld = length(d);
  float a = ld * ld;
  float half_b = dot(oc, d);
  float lo = length(oc);
  float cc = lo * lo - radius * radius;
  float disc = half_b * half_b - a * cc;
  if (disc < 0) return -1.0f;
  return (-half_b - __builtin_sqrtf(disc)) / a;
}

// singlehit K:432-464 on one primitive record (three 16-byte units); returns t or -1
__device__ __forceinline__ float prim_hit_regs(float4 A, float4 B, float4 C, V3 o, V3 d) {
  int type = __float_as_int(C.y);
  float dist = -1.0f;
  if (type == 2) dist = tri_hit(o, d, mk(A.x, A.y, A.z), mk(A.w, B.x, B.y), mk(B.z, B.w, C.x));
  else if (type == 0) dist = sphere_hit(mk(A.x, A.y, A.z), A.w, o, d);
  if (dist < 10000.0f && dist > -0.0f) return dist;          // K:449
  return -1.0f;
}
// the same on the walk array's leaf record: kind (WALK_KIND_*), v0 / centre, e1 (e1.x = radius), e2
__device__ __forceinline__ float prim_hit_kind(int kind, V3 v0, V3 e1, V3 e2, V3 o, V3 d) {
  float dist = -1.0f;
  if (kind == WALK_KIND_TRIANGLE) dist = tri_hit(o, d, v0, e1, e2);
  else if (kind == WALK_KIND_SPHERE) dist = sphere_hit(v0, e1.x, o, d);
  if (dist < 10000.0f && dist > -0.0f) return dist;          // K:449
  return -1.0f;
}
// ... with a triangle's barycentrics handed out (tri_hit above).  A sphere has none: it writes zeros, which nobody reads, so that the caller's words have
// a value on every path that can return t > 0 and may stay without one on the others.
__device__ __forceinline__ float prim_hit_kind(int kind, V3 v0, V3 e1, V3 e2, V3 o, V3 d, float& u_out, float& v_out) {
  float dist = -1.0f;
  if (kind == WALK_KIND_TRIANGLE) dist = tri_hit(o, d, v0, e1, e2, u_out, v_out);
  else if (kind == WALK_KIND_SPHERE) { dist = sphere_hit(v0, e1.x, o, d); u_out = v_out = 0.0f; }
  if (dist < 10000.0f && dist > -0.0f) return dist;          // K:449
  return -1.0f;
}
// successor of the leaf record that link `node` (bit 0 set) points to: the next record (4 units on), or the end
// of the walk.  The walk array ends with a terminator record (an internal node with an empty box and both links
// -1), so the plain build needs no end test: the last leaf's successor is that record (two instructions instead
// of eight on the hot path).  The counting build stops at the last leaf itself so that its visit counter stays
// the reference's.
template <bool COUNT>
__device__ __forceinline__ int leaf_successor(int node, int info) {
  const int next = node + (2 * WALK_UNITS_LEAF - 1) + ((info >> 28) & 1);
  if (COUNT) return (info >> 29) & 1 ? -1 : next;
  return next;
}
__device__ __forceinline__ float prim_hit(const DevPrim* __restrict__ prims, int slot, V3 o, V3 d) {
  const float4* p = reinterpret_cast<const float4*>(prims + slot);
  return prim_hit_regs(p[0], p[1], p[2], o, d);
}

struct Hit { float t; int slot; };

struct Ctr { unsigned rays, V, L, S, T, samples, trav_slots, ray_slots; };   // *_slots: 64 per wave-level iteration / query (SIMD efficiency probes)

// The leaf's side of hit()'s pruning test for a walk that is not in the reference's order.  hit() K:484 enters a box only if its entry distance is < the
// running best t; the near-first walks enter at <=, because a leaf entered exactly at the best t may hold a TIE on t with a leaf that comes earlier in the
// reference's order (lower slot), which hit() would have met first.  At entry == best t that is the only thing it may hold: a hit NEARER than the best from a
// leaf that comes LATER in the reference's order is one hit() never sees -- it has the best already (or something nearer) when it reaches that box, and
// prunes it.  Such a leaf exists only where the computed entry distance of a box exceeds the computed t of the primitive inside it, which the 0.01 of padding
// rules out until floats step by more than that (coordinates of 2^20: tests/ray_cases.py far_mesh, long_short).  "No hit yet" is slot -1: the largest unsigned.
__device__ __forceinline__ bool leaf_entry_admits(float dist, int slot, float best_t, int best_slot) {
  return dist < best_t || (dist == best_t && (unsigned)slot < (unsigned)best_slot);
}

}  // namespace dr
