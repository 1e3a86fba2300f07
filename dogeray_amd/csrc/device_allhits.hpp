// Every crossing of a caller ray (dr_trace_all_hits; DESIGN.md 4.19 has the contract and the reachability argument): the acceptance test of one leaf, the
// per-lane sorted list of the K smallest keys, the two walks that never shrink their best t, and the per-ray bodies of the kernels of kernels_allhits.hip.
#pragma once
#include "device_trace.hpp"
#include "device_aov.hpp"

namespace dr {

// ------------------------------------------------------------------ the list
// K hit_key(t, slot) pairs per lane, ascending, as two 32-bit words each -- t's bits (t > 0: they order like the value), then the slot --, word w of lane l at
// list[w * 64 + l]: the WideStack layout, so a wave's reads and writes touch 64 consecutive words and never bank-conflict.  `list` points at the lane's
// word 0.  It lives in LDS beside the stack (kernels_allhits.hip has the figures); the host build hands in an array of the same shape.  Entries
// [0, min(count, K)) are valid, nothing is initialised per ray.  An insertion shifts the larger keys up by one, from the end: memory words under a
// run-time index, no register array.  A slot is offered at most once per ray (every leaf record has one parent), so equal keys do not occur.
constexpr int ALLHITS_MAX = DR_ALLHITS_MAX;
constexpr int ALLHITS_LIST_WORDS = 2 * ALLHITS_MAX;      // per lane
__device__ __forceinline__ bool allhits_key_less(unsigned tb, unsigned slot, unsigned etb, unsigned eslot) { return tb < etb || (tb == etb && slot < eslot); }
__device__ __forceinline__ void allhits_insert(unsigned* __restrict__ list, int K, int count, unsigned tb, unsigned slot) {
  if (K <= 0) return;
  int j = count < K ? count : K;      // the entries listed so far; the new key lands at j or below
  if (j == K) {                       // full: the largest key leaves, unless the new one is larger still
    if (!allhits_key_less(tb, slot, list[(2 * K - 2) * 64], list[(2 * K - 1) * 64])) return;
    j = K - 1;
  }
  while (j > 0) {
    const unsigned etb = list[(2 * j - 2) * 64], eslot = list[(2 * j - 1) * 64];
    if (!allhits_key_less(tb, slot, etb, eslot)) break;
    list[(2 * j) * 64] = etb; list[(2 * j + 1) * 64] = eslot;
    j--;
  }
  list[(2 * j) * 64] = tb; list[(2 * j + 1) * 64] = slot;
}

// ------------------------------------------------------------------ one leaf
// Slot s is CROSSED by the ray (o, d, cap) when its kind is in kind_mask (bit 0 triangles, bit 1 spheres), slab() passes on the box of its leaf record (the
// reference's padded box, in both trees) and t = prim_hit_kind satisfies 0 < t <= cap: the acceptance rule of hit() K:484-488 without the running best -- a
// conjunction of pure tests of the ray and of that one record, so the set of a ray's crossings is defined without any tree.  The order here (box,
// primitive, cap, kind) changes nothing.
__device__ __forceinline__ bool allhits_kind_in(int kind, int kind_mask) {
  return kind == WALK_KIND_TRIANGLE ? (kind_mask & DR_ALLHITS_TRIANGLES) != 0 : (kind == WALK_KIND_SPHERE && (kind_mask & DR_ALLHITS_SPHERES) != 0);
}
template <class Sign>
__device__ __forceinline__ void allhits_leaf(const float mn[3], const float mx[3], int info, V3 a, V3 b, V3 c, V3 o, V3 d, V3 inv, const Sign& sg, float cap,
                                             int kind_mask, int K, int& count, unsigned* __restrict__ list) {
  float dist;
  if (!slab_sel(o, inv, sg, mn, mx, dist)) return;
  const int kind = (info >> WALK_SLOT_BITS) & 3;
  const float t = prim_hit_kind(kind, a, b, c, o, d);
  if (!(t > 0.0f && t <= cap)) return;
  if (!allhits_kind_in(kind, kind_mask)) return;
  allhits_insert(list, K, count, __float_as_uint(t), (unsigned)(info & ((1 << WALK_SLOT_BITS) - 1)));
  count++;
}
template <class Sign>
__device__ __forceinline__ void allhits_wide_leaf(const WideRec& r, V3 o, V3 d, V3 inv, const Sign& sg, float cap, int kind_mask, int K, int& count,
                                                  unsigned* __restrict__ list) {
  auto f = [](unsigned v) { return __uint_as_float(v); };
  const float mn[3] = {f(r.A.x), f(r.A.y), f(r.A.z)}, mx[3] = {f(r.B.x), f(r.B.y), f(r.B.z)};
  allhits_leaf(mn, mx, (int)r.A.w, mk(f(r.B.w), f(r.C.x), f(r.C.y)), mk(f(r.C.z), f(r.C.w), f(r.D.x)), mk(f(r.D.y), f(r.D.z), f(r.D.w)), o, d, inv, sg, cap, kind_mask,
               K, count, list);
}

// ------------------------------------------------------------------ the walks
// Both visit every leaf a ray crosses: nothing is pruned by t, the cap decides candidates and never boxes (device_trace.hpp says why).
//
// Over the walk array: the hit link when slab() passes on an inner box, the miss link otherwise -- trav_step without its `dist < best` clause (slab()'s exit
// distance starts at 10000, so a box that passes is entered below 10000 anyway).  The inner boxes are the reference's: unions of the padded leaf boxes.
template <bool COUNT>
__device__ __forceinline__ void allhits_threaded(WalkRsrc walk, V3 o, V3 d, float cap, int kind_mask, int K, int& count, unsigned* __restrict__ list, Ctr& c) {
  const V3 inv = mk(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
  const SignCmp sg{inv};
  int node = 0;
  if (COUNT) c.rays++;
  while (node >= 0) {
    const bool leaf = node & 1;
    const unsigned off = (unsigned)(node >> 1) << 4;
    const float4 A = ld_unit(walk, off), B = ld_unit(walk, off + 16);
    float4 C = A, D = A;
    if (leaf) { C = ld_unit(walk, off + 32); D = ld_unit(walk, off + 48); }
    const float mn[3] = {A.x, A.y, A.z}, mx[3] = {B.x, B.y, B.z};
    const int w0 = __float_as_int(A.w);
    const int next_miss = leaf ? leaf_successor<COUNT>(node, w0) : __float_as_int(B.w);
    if (COUNT) c.V++;
    if (leaf) {
      allhits_leaf(mn, mx, w0, mk(B.w, C.x, C.y), mk(C.z, C.w, D.x), mk(D.y, D.z, D.w), o, d, inv, sg, cap, kind_mask, K, count, list);
      node = next_miss;
    } else {
      float dist;
      node = slab_sel(o, inv, sg, mn, mx, dist) ? w0 : next_miss;
    }
  }
}

// Over the 4-way records: wide_fetch, the ray's margins (wide_ray with the scene's WideMu), the node step, wide_pop and the WideStack words are the closest-hit
// walk's, unchanged; tr.best_t keeps trav_begin's 10000 for the whole walk, so the node step's cap on the exit distance is slab()'s own and never a hit's t.
template <bool COUNT>
__device__ __forceinline__ void allhits_wide(WalkRsrc wide, const WideRay& wr, V3 o, V3 d, V3 inv, float cap, int kind_mask, int K, int& count,
                                             unsigned* __restrict__ list, Ctr& c, int* __restrict__ stack /* [word * 64] */) {
  Trav tr;
  trav_begin(tr);
  WideStack ws; ws.top = 0u; ws.sp = 0; ws.sb = 0;
  const SignCmp sg{inv};
  if (COUNT) c.rays++;
  while (tr.node >= 0) {
    const WideRec r = wide_fetch(wide, tr.node);
    if (tr.node & 1) {
      if (COUNT) c.V++;
      allhits_wide_leaf(r, o, d, inv, sg, cap, kind_mask, K, count, list);
      wide_pop(tr, ws, stack);
    } else wide_node_compute<COUNT>(r, wr, sg, tr, ws, stack, c);
  }
}

// ------------------------------------------------------------------ the per-ray bodies
// One ray: the number of its crossings; their K smallest keys are left in `list`.  A tmax that admits nothing (NaN, <= 0: trace_cap) is 0 without a walk.
// WIDE: the 4-way records (the caller has checked that the scene has them), else the threaded links.
template <bool WIDE, bool COUNT>
__device__ __forceinline__ int allhits_ray(const RenderParams& P, V3 o, V3 d, float tmax, int kind_mask, int K, unsigned* __restrict__ list, Ctr& c, int* __restrict__ stack) {
  const float cap = trace_cap(tmax);
  int count = 0;
  if (!(cap > 0.0f)) return 0;
  if (WIDE) {
    const V3 inv = mk(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
    allhits_wide<COUNT>(wide_rsrc(P), wide_ray(o, d, inv, P.wide_pmax, P.wide_mu.e, P.wide_mu.l, P.wide_mu.v), o, d, inv, cap, kind_mask, K, count, list, c, stack);
  } else allhits_threaded<COUNT>(walk_rsrc(P), o, d, cap, kind_mask, K, count, list, c);
  return count;
}

// What a finished ray leaves behind: count[i], and in row i of the [n, K] outputs the listed hits in key order, then the unused entries -- t -1, object -1,
// hit {bits of -1, -1}.  hit: two words per entry, {t bits, slot}, what the surface pass reads.  Null: not written.
__device__ __forceinline__ void allhits_store(size_t i, int count, int K, const unsigned* __restrict__ list, const int32_t* __restrict__ slot_to_orig,
                                              int32_t* count_out, float* t_out, int32_t* object_out, uint32_t* hit_out) {
  if (count_out) count_out[i] = count;
  const int listed = count < K ? count : K;
  for (int k = 0; k < K; k++) {
    const unsigned tb = k < listed ? list[(2 * k) * 64] : __float_as_uint(-1.0f);
    const int slot = k < listed ? (int)list[(2 * k + 1) * 64] : -1;
    const size_t e = i * (size_t)K + (size_t)k;
    if (t_out) t_out[e] = __uint_as_float(tb);
    if (object_out) object_out[e] = slot >= 0 ? slot_to_orig[slot] : -1;
    if (hit_out) { hit_out[2 * e] = tb; hit_out[2 * e + 1] = (unsigned)slot; }
  }
}

// The surface pass, one entry e = i * K + k: ray_surface (device_aov.hpp) at the listed hit, in the role trace_surface_kernel has for dr_trace_rays; an
// unused entry is material -1 and zeros.
struct AllHitsSurface { float* distance; int32_t* material; float* normal; float* uv; float* albedo; };
__device__ __forceinline__ void allhits_surface(const RenderParams& P, const float* __restrict__ origin, const float* __restrict__ dir, const uint32_t* __restrict__ hit,
                                                int K, size_t e, const AllHitsSurface& S) {
  const size_t i = e / (size_t)K;
  const int slot = (int)hit[2 * e + 1];
  const AovHit a = ray_surface(P, ld3(origin + 3 * i), ld3(dir + 3 * i), __uint_as_float(hit[2 * e]), slot);
  if (S.distance) S.distance[e] = a.slot >= 0 ? a.distance : 0.0f;
  if (S.material) S.material[e] = a.mat;
  if (S.normal) { S.normal[3 * e] = a.normal.x; S.normal[3 * e + 1] = a.normal.y; S.normal[3 * e + 2] = a.normal.z; }
  if (S.uv) { S.uv[2 * e] = a.u; S.uv[2 * e + 1] = a.v; }
  if (S.albedo) { S.albedo[3 * e] = a.albedo.x; S.albedo[3 * e + 1] = a.albedo.y; S.albedo[3 * e + 2] = a.albedo.z; }
}

}  // namespace dr
