// Nearest-surface point queries (dr_query_nearest; DESIGN.md 4.18 has the contract and the proof): the distance of a point to one primitive, the two
// walks that find the nearest primitive of the resident scene, and the per-query bodies of the walk kernel and of the finishing pass.
#pragma once
#include "device_wide.hpp"
#include "device_launch.h"

namespace dr {

// ------------------------------------------------------------------ one primitive
// a * b - c * d with one rounding's worth of error whatever cancels (Kahan): the fmafs are written out, nothing else here is fused
__device__ __forceinline__ float near_dop(float a, float b, float c, float d) {
  const float w = c * d;
  const float e = __builtin_fmaf(-c, d, w);      // w - c d, exactly
  const float f = __builtin_fmaf(a, b, -w);
  return f + e;
}
__device__ __forceinline__ V3 near_cross(V3 a, V3 b) { return mk(near_dop(a.y, b.z, a.z, b.y), near_dop(a.z, b.x, a.x, b.z), near_dop(a.x, b.y, a.y, b.x)); }
// the parameter in [0, 1] of the point of the segment a + t e nearest the origin (never NaN: 0 / 0 and inf / inf give 0)
__device__ __forceinline__ float near_seg_t(V3 a, V3 e) {
  const float t = -dot(a, e) / dot(e, e);
  return __builtin_fminf(__builtin_fmaxf(t, 0.0f), 1.0f);
}

struct Nearest { float d2; V3 q; float u, v; bool cand; };      // cand false: the primitive never answers (d2 = +inf then)

// The squared distance d2 of the point p to the primitive (kind, a, b, c) = (WALK_KIND_*, v0 / centre, e1 (e1.x: radius), e2) as the leaf record and
// DevPrim store them, the nearest point q of the primitive and its barycentrics (a sphere: 0, 0).
//
// Triangle.  Translated first: s = v0 - p, one rounding per component, so that every later error is relative to the DISTANCE and the edges and not to
// the coordinates.  The seven regions of the triangle (face, three edges, three corners) are classified by taking the minimum over one candidate per
// region: each edge's nearest point (its parameter clamped to [0, 1], which covers the two corners at its ends) and, when the foot of the
// perpendicular lies inside (three edge functions >= 0), the foot itself.  An edge candidate is x = s + u e1 + v e2 evaluated as written; the face
// candidate is x = n (s . n) / (n . n), n = e1 x e2 formed with near_dop, whose length is the plane distance whatever the conditioning of (u, v).  d2 =
// |x|^2, q = p + x.  A triangle with a zero edge or collinear edges has n . n = 0 (or below 2^-100: not trusted) and no face candidate: the answer is the
// distance to the segment or the point that it is.  No operation can produce a NaN from finite input: the clamps ignore one, the face candidate needs
// three comparisons to hold, and a candidate replaces the minimum only by a comparison that holds.
// Sphere (r >= 0).  d = | |p - c| - r |, d2 = d d, q = c + r (p - c) / |p - c|, or c + (r, 0, 0) at the centre.  A sphere whose radius is negative or
// NaN is never a candidate: its box (centre -/+ radius) is inverted, encloses nothing, and no ray enters it either.
__device__ __forceinline__ Nearest nearest_prim(int kind, V3 a, V3 b, V3 c, V3 p) {
  Nearest r;
  r.d2 = __builtin_inff(); r.q = mk(0, 0, 0); r.u = 0.0f; r.v = 0.0f; r.cand = false;
  if (kind == WALK_KIND_SPHERE) {
    const float rad = b.x;
    if (!(rad >= 0.0f)) return r;
    const V3 oc = p - a;
    const float len = __builtin_sqrtf(dot(oc, oc));
    const float d = __builtin_fabsf(len - rad);
    r.d2 = d * d;
    r.q = len > 0.0f ? mk(a.x + rad * (oc.x / len), a.y + rad * (oc.y / len), a.z + rad * (oc.z / len)) : mk(a.x + rad, a.y, a.z);
    r.cand = r.d2 == r.d2;
    return r;
  }
  if (kind != WALK_KIND_TRIANGLE) return r;
  const V3 s = a - p, e1 = b, e2 = c;
  V3 bx = mk(0, 0, 0);
  auto offer = [&r, &bx](float u, float v, V3 x) {
    const float d2 = dot(x, x);
    if (d2 < r.d2 || !r.cand) { if (d2 == d2) { r.d2 = d2; r.u = u; r.v = v; bx = x; r.cand = true; } }
  };
  auto on_edges = [&s, &e1, &e2](float u, float v) { return mk((s.x + u * e1.x) + v * e2.x, (s.y + u * e1.y) + v * e2.y, (s.z + u * e1.z) + v * e2.z); };
  {      // the face
    const V3 n = near_cross(e1, e2);
    const float nn = dot(n, n);
    if (nn >= 0x1p-100f && nn < __builtin_inff()) {
      // the foot is inside when the three edge functions are >= 0: tu = u n.n, tv = v n.n, tw = (1 - u - v) n.n, each the cross product of an EDGE with the
      // vector from a vertex on it -- its error is then a distance of a few u |vertex - p| from that edge's line, however thin the triangle is (u + v
      // formed from u and v would inherit their conditioning: a needle with e1 ~ e2 misplaces its short edge by u |w| |e1| / |e2 - e1|)
      const V3 w = mk(-s.x, -s.y, -s.z), wb = mk(-(s.x + e1.x), -(s.y + e1.y), -(s.z + e1.z));
      const float tu = dot(near_cross(w, e2), n), tv = dot(near_cross(e1, w), n), tw = dot(near_cross(e2 - e1, wb), n);
      if (tu >= 0.0f && tv >= 0.0f && tw >= 0.0f) {
        const float f = dot(s, n) / nn;
        offer(tu / nn, tv / nn, mk(n.x * f, n.y * f, n.z * f));
      }
    }
  }
  const float t1 = near_seg_t(s, e1);
  offer(t1, 0.0f, on_edges(t1, 0.0f));
  const float t2 = near_seg_t(s, e2);
  offer(0.0f, t2, on_edges(0.0f, t2));
  const float t3 = near_seg_t(s + e1, e2 - e1);
  offer(1.0f - t3, t3, on_edges(1.0f - t3, t3));
  r.q = p + bx;
  return r;
}

// ------------------------------------------------------------------ the pruning rule
// A box may be skipped only if no primitive under it can have a float d2 that beats or ties the best.  With u = 2^-24, b = sqrt(best), L = the scene's
// largest |e1| + |e2| (sphere: radius), M = L + |p.x| + |p.y| + |p.z|: a primitive whose float d2 is <= best has a true distance
// d <= (b + 24.3 u L) / (1 - 29.2 u) [the lower side of nearest_prim's error, itself within NEAREST_K u (d + 2 L)]; the true distance of its box is
// <= d + 2 u (|p| + d + 2 L) [a sphere's box centre -/+ radius is rounded; a triangle's reference box may miss the record's v0 + e by u L; own bounds
// and decoded planes enclose]; and the float lb2 is <= the true one times (1 + 6 u), + 2^-148.  Together: sqrt(lb2) <= b (1 + 35 u) + 29 u M for every
// box that holds such a primitive, and a box whose lb2 is above
//     thr = (b (1 + 64 u) + 64 u M)^2 (1 + 64 u) + 2^-100          [= best (1 + r) + abs(best, M): r ~ 2^-16, abs = 2 b E + E^2 + 2^-100, E = 2^-18 M]
// holds none: the larger constants pay for the roundings of thr's own five operations, 2^-100 for every underflow (a d2 or an lb2 below 2^-126
// loses bits; (2^-50)^2 is beyond all of them).  thr is formed when the best changes, not per box.  M >= 2^30 or NaN: E = inf, the query never prunes.
constexpr int NEAREST_K = 32;
constexpr float NEAR_REL = 0x1p-18f, NEAR_ABS = 0x1p-18f, NEAR_FLOOR = 0x1p-100f, NEAR_TAME = 0x1p30f;
__device__ __forceinline__ float near_abs_term(V3 p, float lmax) {      // E
  const float m = lmax + ((__builtin_fabsf(p.x) + __builtin_fabsf(p.y)) + __builtin_fabsf(p.z));
  return m < NEAR_TAME ? m * NEAR_ABS : __builtin_inff();
}
__device__ __forceinline__ float near_threshold(float best_d2, float abs_term) {
  const float t = __builtin_sqrtf(best_d2) * (1.0f + NEAR_REL) + abs_term;
  return (t * t) * (1.0f + NEAR_REL) + NEAR_FLOOR;
}
// squared distance of p to the box [lo, hi], a lower bound in the sense above (an inverted or NaN box: whatever comes out is compared with `>` only)
__device__ __forceinline__ float near_box_lb2(float lox, float loy, float loz, float hix, float hiy, float hiz, V3 p) {
  const float gx = __builtin_fmaxf(__builtin_fmaxf(lox - p.x, p.x - hix), 0.0f);
  const float gy = __builtin_fmaxf(__builtin_fmaxf(loy - p.y, p.y - hiy), 0.0f);
  const float gz = __builtin_fmaxf(__builtin_fmaxf(loz - p.z, p.z - hiz), 0.0f);
  return gx * gx + gy * gy + gz * gz;
}
// (d2, slot) against the running best by the key order (bits(d2), slot): d2 >= +0, so its bits order like its value; "none yet" is slot -1, the
// largest unsigned, at d2 = the query's cap -- a candidate AT the cap is taken, one beyond it never
__device__ __forceinline__ void near_offer(Trav& tr, float& thr, float abs_term, const Nearest& n, int slot) {
  if (n.cand && (n.d2 < tr.best_t || (n.d2 == tr.best_t && (unsigned)slot < (unsigned)tr.best_slot))) {
    tr.best_t = n.d2; tr.best_slot = slot;
    thr = near_threshold(n.d2, abs_term);
  }
}

// ------------------------------------------------------------------ the walks (Trav::best_t holds the best d2)
// Over the DFS walk array (device_layout.h): the hit link when the box survives, the miss link otherwise; a leaf's primitive behind its own box.
template <bool COUNT>
__device__ __forceinline__ void nearest_threaded(WalkRsrc walk, V3 p, float abs_term, Trav& tr, Ctr& c) {
  tr.node = 0;
  float thr = near_threshold(tr.best_t, abs_term);
  while (tr.node >= 0) {
    const bool leaf = tr.node & 1;
    const unsigned off = (unsigned)(tr.node >> 1) << 4;
    const float4 A = ld_unit(walk, off), B = ld_unit(walk, off + 16);
    float4 C = A, D = A;
    if (leaf) { C = ld_unit(walk, off + 32); D = ld_unit(walk, off + 48); }
    const int w0 = __float_as_int(A.w);
    const int next_miss = leaf ? leaf_successor<COUNT>(tr.node, w0) : __float_as_int(B.w);
    if (COUNT) c.V++;
    const float lb2 = near_box_lb2(A.x, A.y, A.z, B.x, B.y, B.z, p);
    const bool survives = !(lb2 > thr);
    if (survives && leaf) {
      if (COUNT) c.L++;
      near_offer(tr, thr, abs_term, nearest_prim((w0 >> WALK_SLOT_BITS) & 3, mk(B.w, C.x, C.y), mk(C.z, C.w, D.x), mk(D.y, D.z, D.w), p), w0 & ((1 << WALK_SLOT_BITS) - 1));
    }
    tr.node = (survives && !leaf) ? w0 : next_miss;
  }
}

// Over the 4-way records, on the ray walk's per-lane stack (device_wide.hpp WideStack, wide_pop).  The node step decodes the four children's planes as
// fmaf(byte, scale, origin) -- plane_t with a = scale * 2^24, b = origin: that number, rounded once, the decode the host builder checked for enclosure --,
// forms each child's lower bound, descends into the nearest surviving child and parks the rest as one stack word.
template <bool COUNT>
__device__ __forceinline__ void near_node_compute(const WideRec& r, V3 p, float thr, Trav& tr, WideStack& ws, int* __restrict__ stack, Ctr& c) {
  if (COUNT) c.V++;
  const float ox = __uint_as_float(r.A.x), oy = __uint_as_float(r.A.y), oz = __uint_as_float(r.A.z);
  const float sx24 = __uint_as_float(r.C.z << 16), sy24 = __uint_as_float(r.C.z & 0xffff0000u), sz24 = __uint_as_float(r.C.w);
  const PlanePairs lx = plane_pairs(r.B.x), ly = plane_pairs(r.B.y), lz = plane_pairs(r.B.z), hx = plane_pairs(r.B.w), hy = plane_pairs(r.C.x), hz = plane_pairs(r.C.y);
  const unsigned valid = (r.A.w >> 24) & 15u;
  unsigned mask = 0u, key = 0xffffffffu;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const float lb2 = near_box_lb2(plane_t(lx, k, sx24, ox), plane_t(ly, k, sy24, oy), plane_t(lz, k, sz24, oz),
                                   plane_t(hx, k, sx24, ox), plane_t(hy, k, sy24, oy), plane_t(hz, k, sz24, oz), p);
    const bool ok = ((valid >> k) & 1u) && !(lb2 > thr);
    const unsigned kk = ok ? ((__float_as_uint(lb2) & ~3u) | (unsigned)k) : 0xffffffffu;      // (the order of the visits only: the answer does not depend on it)
    mask |= ok ? (1u << k) : 0u;
    key = kk < key ? kk : key;
  }
  if (mask != 0u) {
    int near = (int)(key & 3u);
    near = ((mask >> near) & 1u) ? near : __builtin_ctz(mask);      // (a NaN bound's key can be all ones)
    const unsigned base = r.A.w & 0xffffffu, leafmask = r.A.w >> 28;
    const unsigned rest = mask & ~(1u << near);
    if (rest != 0u) {
      if (ws.top != 0u) { if (ws.sp < WIDE_STACK) { stack[ws.sp * 64] = (int)ws.top; ws.sp++; } }   // the host bounds the depth; the guard only protects the stack
      ws.top = (base << 8) | (leafmask << 4) | rest;
    }
    tr.node = (int)(((base + (unsigned)near) << 1) | ((leafmask >> near) & 1u));
  } else {
    wide_pop(tr, ws, stack);
  }
}
template <bool COUNT>
__device__ __forceinline__ void near_leaf_compute(const WideRec& r, V3 p, float abs_term, float& thr, Trav& tr, WideStack& ws, const int* __restrict__ stack, Ctr& c) {
  auto f = [](unsigned v) { return __uint_as_float(v); };
  if (COUNT) c.V++;
  const float lb2 = near_box_lb2(f(r.A.x), f(r.A.y), f(r.A.z), f(r.B.x), f(r.B.y), f(r.B.z), p);      // the best may have shrunk since the parent's test
  if (!(lb2 > thr)) {
    if (COUNT) c.L++;
    const int info = (int)r.A.w;
    near_offer(tr, thr, abs_term, nearest_prim((info >> WALK_SLOT_BITS) & 3, mk(f(r.B.w), f(r.C.x), f(r.C.y)), mk(f(r.C.z), f(r.C.w), f(r.D.x)), mk(f(r.D.y), f(r.D.z), f(r.D.w)), p),
               info & ((1 << WALK_SLOT_BITS) - 1));
  }
  wide_pop(tr, ws, stack);
}
template <bool COUNT>
__device__ __forceinline__ void nearest_wide(WalkRsrc wide, V3 p, float abs_term, Trav& tr, Ctr& c, int* __restrict__ stack /* [word * 64] */) {
  tr.node = 0;
  WideStack ws; ws.top = 0u; ws.sp = 0; ws.sb = 0;
  float thr = near_threshold(tr.best_t, abs_term);
  while (tr.node >= 0) {
    const WideRec r = wide_fetch(wide, tr.node);
    if (tr.node & 1) near_leaf_compute<COUNT>(r, p, abs_term, thr, tr, ws, stack, c);
    else near_node_compute<COUNT>(r, p, thr, tr, ws, stack, c);
  }
}

// ------------------------------------------------------------------ the per-query bodies
// The answer of query i is the minimum of (bits(d2), slot) over the candidates with d2 <= fl(cap cap), cap = rmax (NULL or +inf: unbounded); a NaN or
// negative rmax and a non-finite point are misses without a walk.  Written: key {d2 bits, slot}, d2, distance = sqrt(d2), object; a miss is
// {0, -1}, 0, -1, -1.  WIDE: the 4-way records (the caller has checked that the scene has them), else the threaded links.
template <bool WIDE, bool COUNT>
__device__ __forceinline__ void nearest_query(const RenderParams& P, const NearestLaunch& N, unsigned i, Ctr& c, int* __restrict__ stack) {
  const V3 p = ld3(N.point + 3 * (size_t)i);
  const float rmax = N.rmax ? N.rmax[i] : __builtin_inff();
  const float inf = __builtin_inff();
  Trav tr; tr.node = LANE_DONE; tr.best_t = rmax * rmax; tr.best_slot = -1;
  if (rmax >= 0.0f && __builtin_fabsf(p.x) < inf && __builtin_fabsf(p.y) < inf && __builtin_fabsf(p.z) < inf) {
    const float abs_term = near_abs_term(p, N.lmax);
    if (WIDE) nearest_wide<COUNT>(wide_rsrc(P), p, abs_term, tr, c, stack);
    else nearest_threaded<COUNT>(walk_rsrc(P), p, abs_term, tr, c);
  }
  const bool hit = tr.best_slot >= 0;
  const float d2 = hit ? tr.best_t : 0.0f;
  N.key[2 * (size_t)i] = __float_as_uint(d2); N.key[2 * (size_t)i + 1] = (unsigned)tr.best_slot;
  if (N.d2) N.d2[i] = d2;
  if (N.distance) N.distance[i] = hit ? __builtin_sqrtf(d2) : -1.0f;
  if (N.object) N.object[i] = hit ? N.slot_to_orig[tr.best_slot] : -1;
}
// The finishing pass: nearest_prim again for the winning slot, from the primitive records, for the nearest point, its barycentrics and the material
__device__ __forceinline__ void nearest_finish(const RenderParams& P, const NearestLaunch& N, unsigned i) {
  const int slot = (int)N.key[2 * (size_t)i + 1];
  Nearest n; n.q = mk(0, 0, 0); n.u = 0.0f; n.v = 0.0f;
  int mat = -1;
  if (slot >= 0) {
    const DevPrim& pr = P.prims[slot];
    const int kind = pr.type == 0 ? WALK_KIND_SPHERE : (pr.type == 2 ? WALK_KIND_TRIANGLE : WALK_KIND_NONE);
    n = nearest_prim(kind, mk(pr.v0[0], pr.v0[1], pr.v0[2]), mk(pr.e1x, pr.e1y, pr.e1z), mk(pr.e2x, pr.e2y, pr.e2z), ld3(N.point + 3 * (size_t)i));
    mat = P.shade[slot].mat;
  }
  if (N.qpoint) { N.qpoint[3 * (size_t)i] = n.q.x; N.qpoint[3 * (size_t)i + 1] = n.q.y; N.qpoint[3 * (size_t)i + 2] = n.q.z; }
  if (N.uv) { N.uv[2 * (size_t)i] = n.u; N.uv[2 * (size_t)i + 1] = n.v; }
  if (N.material) N.material[i] = mat;
}

}  // namespace dr
