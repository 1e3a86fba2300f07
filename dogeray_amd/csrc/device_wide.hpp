// The walk over the 4-way tree: the ray's margins, the folded node test, the per-lane stack, the node and the leaf step.
#pragma once
#include "device_walk.hpp"

namespace dr {

// ------------------------------------------------------------------ wide walk
// hit() K:468-512 over the 4-way tree of wide_builder.cpp (device_layout.h "wide walk").  The answer is the
// lexicographic minimum (t, slot) over the leaves whose own (exact, reference) box the ray enters no farther than
// the best t -- the reference's hit, by the argument at closest_hit_ordered below: internal boxes only have to
// ENCLOSE the leaves under them (the host checks every decoded plane with this very fmaf), and the slab test is
// monotone in the box, so a subtree is skipped only if every leaf in it would fail its own test.
//
// Per lane: `node` = record index << 1 | is-leaf; the children of a node that were entered but not yet visited
// are one word (first child's index << 8 | leaf mask << 4 | pending mask); the newest such word lives in a
// register (`top`), older ones on a per-lane stack in LDS (word k of lane l at stack[k * 64 + l]: conflict-free).
struct WideStack { unsigned top; int sp; int sb; };   // LDS words [sb, sp): sb > 0 once the oldest words have been handed to helper lanes

// Tests the four children of a node; returns the mask of those the ray may enter no farther than best_t, and the key
// of the nearest (entry distance bits with the child number in the two lowest bits).
//
// Arithmetic: the ray is folded into the node's grid once per node -- a = scale * inv, b = (origin - o) * inv -- and a plane
// costs one fma: t = fma(byte, a, b -/+ m).  The result only has to be CONSERVATIVE with respect to the slab test on the
// decoded plane p = fmaf(byte, scale, origin), which the host checked to enclose the exact boxes: near planes not later, far
// planes not earlier than fl(fl(p - o) * inv).  Both computations differ from the real number (byte * scale + origin - o) * inv
// by at most
//   |inv| * u * (3 P + 2 |o|)   [decode, subtract, multiply]   and   u |inv| (3 |o| + P) + 2 u m + u |t|   [this one],
// u = 2^-24, P = the largest |plane coordinate| of the scene's nodes; the sum is u |inv| (5 P + 6 |o|) + 3 u m < m =
// 8 u |inv| (P + |o|) (scale is a power of two in [2^-60, 2^36], so a is exact; tools/study_wide_walk.cpp checks at every node of
// every sample scene that this mask covers the decode-and-slab one).
//  * a plane byte is read as the f16 DENORMAL byte * 2^-24 (half-word 0x00bb) and the node record stores scale * 2^24
//    (device_layout.h), so that v_fma_mix_f32 converts the byte on the fly: fma(byte * 2^-24, (scale * 2^24) * inv, b) is the SAME
//    real number rounded once as fma(byte, scale * inv, b) -- one instruction per plane instead of a conversion and an fma, and two
//    plane bytes are unpacked by one v_and / v_perm (the kernel runs with f16 denormals on, .amdhsa_float_denorm_mode_16_64 3;
//    dr_kat_node_planes checks the instruction).  Powers of two scale exactly as long as nothing overflows: |inv| <= 2^60
//    (clamped), scale <= 2^36 (wide_builder.cpp refuses larger grids), so a <= 2^120.
//  * b -/+ m = fma(origin, inv, -(fl(o * inv) +- m)) with the ray-only part precomputed by wide_ray().  o * inv could overflow
//    for |o| > 2^67 where (origin - o) * inv did not: an axis with |o| >= 2^60 is left unconstrained (NaN margin).
//  * the cap of the exit distance is the running best itself (trav_begin: "no hit yet" = 10000).
// Extreme directions.  The test uses inv clamped to +-2^60 (WideRay::inv): for a zero direction component slab()
// computes (p - o) * inf = +-inf, or NaN (ignored) when p == o; (p - o) * 2^60 -/+ m, with m >= 2^20 then, lands on
// the same side of [0, 10000] for every plane at least m * 2^-60 away from the origin and leaves the nearer ones
// unconstrained -- a superset again, and such rays (a few per frame: N + random can cancel exactly) are still culled
// along that axis instead of walking the whole slab.  A NaN or > 2^60-long direction component makes m NaN: every plane of
// that axis becomes NaN and is ignored by max3 / min3 (the axis is not constrained at all).
// (The variants this replaced -- decode-and-slab, conversion + fma, compare + select -- are in the history of this file and
// A/B-measured in profiles/r3_m_node_step_ab.txt.)
struct WideRay { V3 inv, on, of; };      // inv: clamped 1/direction; on / of: fl(o * inv) + m, fl(o * inv) - m (what the near / far planes subtract)
__device__ __forceinline__ WideRay wide_ray_none() {      // a lane without a ray
  WideRay w;
  w.inv = w.on = w.of = mk(0, 0, 0);
  return w;
}
// The position margin of a ray when small triangles sit in the tree with their own bounds (WideMu, wide_tree = 2; proof: DESIGN.md 4.10).  The reference
// accepts a hit when Moeller-Trumbore, in floats, says so AND the leaf's padded box is entered; a tree built over the padded boxes visits every such leaf.
// Built over the triangles' own bounds B it still does if every box test is loosened by mu, where mu bounds how far outside B (per axis, and along the ray
// in units of position) a ray can pass and still be ACCEPTED by the float test.  With u = 2^-24, |a| >= 1e-4 for every accepted hit (hit_tri's cut-off),
// s = o - v0, E = |e1| |e2|, L = |e1| + |e2| (Euclidean norms):
//     |u_f - u^| , |v_f - v^| <= 6.03e-4 |d| |e| (8.52 |s| + 7.11 |e'|) + 2.02 u      (u^, v^, t^: the exact solution of o + t d = v0 + u e1 + v e2)
//     |t_f - t^| |d|          <= 6.03e-4 E |d| (8.52 |s| + 7.11 |t_f| |d|) + 2.02 u |t_f| |d|,   |t_f| |d| <= |s| + L + 0.02
// so the exact ray is inside B + mu_pos at t^, and B + mu_pos + |d| |t_f - t^| is entered no later than t_f and left after it, for
//     mu = |d| E (0.0197 |s| + 0.0086 L + 8.6e-5) + 1.2e-7 |s| + 3.0e-7 L      -- rounded up below to 0.021, 0.015, 1.2e-4 and 2^-21 (|s| + 4 L + 1), |s| <= |o| + |v0|.
// Above the cap the margin is the reference's own padding (B + 0.01 (1 + 2^-16) + the absolute term encloses the padded box): such rays -- camera rays with a
// long direction vector, mostly -- walk the tree exactly as they would the tree over padded boxes.  Rays or scenes beyond 2^30 take the cap too (no overflow
// inside the bound's arithmetic below that).
// cert: 1, or -- a camera ray whose tile the view's grazing certificate clears (|a^| >= a_star for every triangle it can be accepted on) -- the factor
// 1e-4 / a_star rounded up (params_host.hpp cert_factor_k): step 2 of the lemma divides by a_star instead of 1e-4, and every |d|-proportional term scales with it.
// The tame guard keeps the scene's E (a stronger condition than the scaled one).  With cert = 1 the arithmetic is the uncertified one, bit for bit.
__device__ __forceinline__ float wide_ray_margin(V3 o, V3 d, float mu_e, float mu_l, float mu_v, float cert = 1.0f) {
  if (!(mu_e > 0.0f)) return 0.0f;
  const float on = __builtin_sqrtf(dot(o, o)) * 1.0001f, dn = __builtin_sqrtf(dot(d, d)) * 1.0001f, s = on + mu_v;
  const float abs_term = (s + 4.0f * mu_l + 1.0f) * 0x1p-21f;
  const float cap = 0.01f * (1.0f + 0x1p-16f) + abs_term;
  const float m = dn * mu_e * cert * 1.0001f * (0.021f * s + 0.015f * mu_l + 1.2e-4f) * 1.0001f + abs_term;
  const bool tame = dn <= 0x1p30f && s <= 0x1p30f && dn * mu_e <= 2.0f;      // (false for NaNs)
  return (tame && m < cap) ? m : cap;
}
__device__ __forceinline__ WideRay wide_ray(V3 o, V3 d, V3 inv, float pmax, float mu_e, float mu_l, float mu_v, float cert = 1.0f) {      // (mu_*: the scene's WideMu)
  WideRay w;
  const float extra = wide_ray_margin(o, d, mu_e, mu_l, mu_v, cert);
  auto one = [pmax, extra](float oa, float ia, float& ic, float& on, float& of) {
    ic = __builtin_fminf(__builtin_fmaxf(ia, -0x1p60f), 0x1p60f);                    // NaN -> -2^60, and the margin below is NaN
    const float k = __builtin_fmaf(pmax + __builtin_fabsf(oa), 0x1p-21f, 0x1p-40f) + extra;
    const float ai = __builtin_fabsf(ic);
    const float m = (ia == ia && ai > 0x1p-60f && __builtin_fabsf(oa) < 0x1p60f) ? ai * k : __builtin_nanf("");
    const float p = oa * ic;
    on = p + m; of = p - m;
  };
  one(o.x, inv.x, w.inv.x, w.on.x, w.of.x); one(o.y, inv.y, w.inv.y, w.on.y, w.of.y); one(o.z, inv.z, w.inv.z, w.on.z, w.of.z);
  return w;
}

template <class Sign>
__device__ __forceinline__ unsigned wide_node_test(u32x4 A, u32x4 B, u32x4 C, const WideRay& wr, const Sign& sg, float best_t, unsigned& near_key) {
  const float ox = __uint_as_float(A.x), oy = __uint_as_float(A.y), oz = __uint_as_float(A.z);
  const float sx24 = __uint_as_float(C.z << 16), sy24 = __uint_as_float(C.z & 0xffff0000u), sz24 = __uint_as_float(C.w);      // scale * 2^24 (x, y: upper halves of their floats)
  const V3 inv = wr.inv;
  // the plane entered first is `hi` for a negative direction (slab(): same rule, so the comparison stays plane by plane)
  // (sg holds the signs of the plain 1/direction; the clamped one differs for a NaN only, and a NaN axis has NaN planes whichever word is read)
  const unsigned nxw = sg.sel(0, B.x, B.w), fxw = sg.sel(0, B.w, B.x);
  const unsigned nyw = sg.sel(1, B.y, C.x), fyw = sg.sel(1, C.x, B.y);
  const unsigned nzw = sg.sel(2, B.z, C.y), fzw = sg.sel(2, C.y, B.z);
  unsigned fail[4], kk[4];
  const float tcap = best_t;
  const float ax = sx24 * inv.x, ay = sy24 * inv.y, az = sz24 * inv.z;
  const float bxn = __builtin_fmaf(ox, inv.x, -wr.on.x), bxf = __builtin_fmaf(ox, inv.x, -wr.of.x);
  const float byn = __builtin_fmaf(oy, inv.y, -wr.on.y), byf = __builtin_fmaf(oy, inv.y, -wr.of.y);
  const float bzn = __builtin_fmaf(oz, inv.z, -wr.on.z), bzf = __builtin_fmaf(oz, inv.z, -wr.of.z);
  const PlanePairs pnx = plane_pairs(nxw), pfx = plane_pairs(fxw), pny = plane_pairs(nyw), pfy = plane_pairs(fyw), pnz = plane_pairs(nzw), pfz = plane_pairs(fzw);
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const float t0x = plane_t(pnx, k, ax, bxn), t1x = plane_t(pfx, k, ax, bxf);
    const float t0y = plane_t(pny, k, ay, byn), t1y = plane_t(pfy, k, ay, byf);
    const float t0z = plane_t(pnz, k, az, bzn), t1z = plane_t(pfz, k, az, bzf);
    const float t_min = __builtin_fmaxf(__builtin_fmaxf(__builtin_fmaxf(t0x, t0y), t0z), 0.0f);
    const float t_max = __builtin_fminf(__builtin_fminf(__builtin_fminf(t1x, t1y), t1z), tcap);
    // A child is entered when t_max >= t_min (>= where slab() has > and <=: a superset, which is all an internal node needs).  Taken from the SIGN
    // of t_max - t_min: neither is ever NaN (max / min ignore NaNs; 0 and the cap are numbers), t_max is finite or -inf, so the difference is a
    // number, +0 when they are equal.  (It is -0 only for t_max = -0, t_min = +0, where slab()'s own t_max > t_min fails anyway: still a superset.)
    // The sign, spread over a word, goes into the key (a failed child's key is all ones) and into the mask with fast bit operations instead of
    // compares and selects (tools/valu_rate.hip: 2.4 against 4.2 SIMD cycles each).
    fail[k] = (unsigned)((int)__float_as_uint(t_max - t_min) >> 31);
    kk[k] = bit_and_or(__float_as_uint(t_min), ~3u, fail[k]) | (unsigned)k;      // t_min >= 0: its bits order like the value
  }
  const unsigned k01 = kk[0] < kk[1] ? kk[0] : kk[1], k23 = kk[2] < kk[3] ? kk[2] : kk[3];
  near_key = k01 < k23 ? k01 : k23;
  // bit k of z = child k failed (the bits above are child 3's): three bitwise selects, then ~z & valid mask in one more
  const unsigned z = bit_select(bit_select(fail[3], fail[2], 4u), bit_select(fail[1], fail[0], 1u), 3u);      // bits 0-1 from the second, the rest from the first
  return bit_andn(z, A.w >> 24, 15u);
}

__device__ __forceinline__ unsigned wide_node_test(u32x4 A, u32x4 B, u32x4 C, V3 inv_plain, const WideRay& wr, float best_t, unsigned& near_key) {
  SignCmp sg; sg.inv = inv_plain;      // the planes chosen by comparing, as the reference does (per-tile kernel, host studies)
  return wide_node_test(A, B, C, wr, sg, best_t, near_key);
}

// (t, slot) as one 64-bit key whose unsigned order is the lexicographic order of the pair (t is positive, or the 10000 of
// "no hit yet" with slot -1 = the largest unsigned): what lanes that share one ray agree on with ds_min_u64
__device__ __forceinline__ unsigned long long hit_key(float t, int slot) { return ((unsigned long long)__float_as_uint(t) << 32) | (unsigned)slot; }

// next record of this lane: the lowest pending child of the newest stack word, or -1 when nothing is left
__device__ __forceinline__ void wide_pop(Trav& tr, WideStack& ws, const int* __restrict__ stack) {
  if (ws.top == 0u) {
    if (ws.sp == ws.sb) { tr.node = LANE_DONE; return; }
    ws.sp--;
    ws.top = (unsigned)stack[ws.sp * 64];
  }
  const int j = __builtin_ctz(ws.top);                       // the pending mask is never empty in a stored word
  tr.node = (int)((((ws.top >> 8) + (unsigned)j) << 1) | ((ws.top >> (4 + j)) & 1u));
  ws.top &= ws.top - 1u;
  ws.top = (ws.top & 15u) ? ws.top : 0u;
}

// wide_pop for the lean persistent build's six-wave kernel (kernels_render.hip; the same next record, remaining word and stack pointer:
// tests/test_lean_pop_host.py) on ONE straight path.  wide_pop compiles there to three nested exec regions, two compares and five register copies around
// some eleven instructions of work, in every leaf step and nearly every node step of the wave (profiles/pop_phase_trim.txt); here
//  * only the LDS read is conditional, and its condition is one compare: the lean build hands no words over (sb == 0 throughout), and a stored word is
//    at least 256 -- record 0 is the root and nobody's child (wide_builder.cpp), so a word's first child is 1 or more -- while sp <= WIDE_STACK: top < sp
//    says "top is 0 and the stack is not empty";
//  * the word popped from (w: top, or the stack's) is 0 exactly when nothing is left, and the record falls out of the same instructions then:
//    lowest_bit(0) = -1 gives (0 - 1) << 1 | 0 = -2, which the max turns into LANE_DONE (-1) and leaves every record (>= 0) alone; the remaining word of 0 is 0.
// A function of its own so that every other caller of wide_pop compiles as before.
static_assert(WIDE_STACK < 256 && LANE_DONE == -1, "wide_pop_lean: top < sp, and the max");
__device__ __forceinline__ void wide_pop_lean(Trav& tr, WideStack& ws, const int* __restrict__ stack) {
  unsigned w = ws.top;
  if (w < (unsigned)ws.sp) { ws.sp--; w = (unsigned)stack[ws.sp * 64]; }
  const int j = lowest_bit(w);
  const int rec = (int)((((w >> 8) + (unsigned)j) << 1) | ((w >> (4 + j)) & 1u));
  tr.node = at_least_minus_one(rec);
  const unsigned rest = w & (w - 1u);
  ws.top = (rest & 15u) ? rest : 0u;
}

// One record = four 16-byte units; a node is its first three (device_layout.h), a leaf all four: the fourth is fetched by the lanes at a leaf only (a
// lane knows from the parent's leaf mask which it is) -- every load instruction of a step costs about 1 % of the frame (profiles/r4_o_node_three_units.txt).
// The empty asm pins the loads in front of the first use: without it hipcc sinks the leaf's primitive units behind the box test, a second dependent round trip.
struct WideRec { u32x4 A, B, C, D; };
__device__ __forceinline__ WideRec wide_fetch(WalkRsrc wide, int node) {
  const unsigned off = (unsigned)(node >> 1) << 6;
  WideRec r;
  r.A = ld_unit_raw(wide, off); r.B = ld_unit_raw(wide, off + 16); r.C = ld_unit_raw(wide, off + 32);
  no_value(r.D);      // (a node lane's fourth unit is never read: no value, no instruction)
  if (node & 1) r.D = ld_unit_raw(wide, off + 48);
  pin_loads(r.A, r.B, r.C, r.D);
  return r;
}
// wide_fetch for a caller that knows already whether the lane stands at a leaf (the six-wave lean build: the lane's bit of a wave mask, device_prims.hpp
// lane_bit), so that `node & 1` is not formed and compared again; the same loads, pinned the same way.  A function of its own so that every other caller
// of wide_fetch compiles as before.  The record's offset is ONE register (one_register), the units at immediate offsets 16, 32, 48 of it: left to itself
// the compiler folds the cleared bit 5 into the constants and forms (node << 5) | 32 and (node << 5) | 48 in registers of their own, an instruction each.
__device__ __forceinline__ WideRec wide_fetch(WalkRsrc wide, int node, bool at_leaf) {
  const unsigned off = one_register((unsigned)(node >> 1) << 6);
  WideRec r;
  r.A = ld_unit_raw(wide, off); r.B = ld_unit_raw(wide, off + 16); r.C = ld_unit_raw(wide, off + 32);
  no_value(r.D);
  if (at_leaf) r.D = ld_unit_raw(wide, off + 48);
  pin_loads(r.A, r.B, r.C, r.D);
  return r;
}

// (POP_LEAN: the lean six-wave build's pop, wide_pop_lean above)
template <bool COUNT, bool POP_LEAN = false, class Sign>
__device__ __forceinline__ void wide_node_compute(const WideRec& r, const WideRay& wr, const Sign& sg, Trav& tr, WideStack& ws, int* __restrict__ stack, Ctr& c) {
  DR_MARK("node_begin");
  if (COUNT) c.V++;
  unsigned key;
  const unsigned mask = wide_node_test(r.A, r.B, r.C, wr, sg, tr.best_t, key);
  if (mask != 0u) {
    // nearest entered child next; the others wait as one stack word.  An unused child slot (inverted box, valid bit
    // clear) can only pass on a degenerate grid or ray; if it even has the smallest key, take the lowest valid one.
    int near = (int)(key & 3u);
    near = ((mask >> near) & 1u) ? near : __builtin_ctz(mask);
    const unsigned base = r.A.w & 0xffffffu, leafmask = r.A.w >> 28;
    const unsigned rest = mask & ~(1u << near);
    if (rest != 0u) {
      if (ws.top != 0u) { if (ws.sp < WIDE_STACK) { stack[ws.sp * 64] = (int)ws.top; ws.sp++; } }   // the host bounds the depth; the guard only protects LDS
      ws.top = (base << 8) | (leafmask << 4) | rest;
    }
    tr.node = (int)(((base + (unsigned)near) << 1) | ((leafmask >> near) & 1u));
  } else {
    if (POP_LEAN) wide_pop_lean(tr, ws, stack);
    else wide_pop(tr, ws, stack);
  }
  DR_MARK("node_end");
}

template <bool COUNT, class Sign>
__device__ __forceinline__ void wide_leaf_compute(const WideRec& r, V3 o, V3 d, V3 inv, const Sign& sg, Trav& tr, WideStack& ws, const int* __restrict__ stack, Ctr& c) {
  auto f = [](unsigned v) { return __uint_as_float(v); };
  DR_MARK("leaf_begin");
  if (COUNT) c.V++;
  float mn[3] = {f(r.A.x), f(r.A.y), f(r.A.z)}, mx[3] = {f(r.B.x), f(r.B.y), f(r.B.z)};
  float dist;
  if (LEAF_PRIM_FIRST && !COUNT) {
    // The candidate is accepted when its primitive is hit AND the leaf's box is entered no farther than the best t (hit() K:484-488: box, then primitive):
    // a conjunction of pure tests, so the order is free.  The primitive first, for every lane (98 % of the lanes pass the box anyway); the box only for the
    // lanes whose primitive is a candidate -- 5 % of them --, and not at all when no lane of the wave has one: 0.5721 against 0.5777 ms/frame
    // (profiles/r4_phase_budget.txt).  The counting build and the host build keep the reference's order: L counts primitives tested behind a passed box.
    const int info = (int)r.A.w;
    const float t = prim_hit_kind((info >> WALK_SLOT_BITS) & 3, mk(f(r.B.w), f(r.C.x), f(r.C.y)), mk(f(r.C.z), f(r.C.w), f(r.D.x)), mk(f(r.D.y), f(r.D.z), f(r.D.w)), o, d);
    const int slot = info & ((1 << WALK_SLOT_BITS) - 1);
    const bool cand = t > 0.0f && (t < tr.best_t || (t == tr.best_t && (unsigned)slot < (unsigned)tr.best_slot));
    if (DR_WAVE_ANY(cand)) {
      if (cand && slab_sel(o, inv, sg, mn, mx, dist) && leaf_entry_admits(dist, slot, tr.best_t, tr.best_slot)) { tr.best_t = t; tr.best_slot = slot; }
    }
  } else if (slab_sel(o, inv, sg, mn, mx, dist) && dist <= tr.best_t) {      // <=: a box entered exactly at the best t may hold a tie with a lower slot
    if (COUNT) c.L++;
    const int info = (int)r.A.w;
    const float t = prim_hit_kind((info >> WALK_SLOT_BITS) & 3, mk(f(r.B.w), f(r.C.x), f(r.C.y)), mk(f(r.C.z), f(r.C.w), f(r.D.x)), mk(f(r.D.y), f(r.D.z), f(r.D.w)), o, d);
    const int slot = info & ((1 << WALK_SLOT_BITS) - 1);
    if (t > 0.0f && leaf_entry_admits(dist, slot, tr.best_t, tr.best_slot) && (t < tr.best_t || (t == tr.best_t && (unsigned)slot < (unsigned)tr.best_slot))) { tr.best_t = t; tr.best_slot = slot; }
  }
  wide_pop(tr, ws, stack);
  DR_MARK("leaf_end");
}

// The primitive-first leaf step above for the lean persistent build with HIT_UV_CARRIED (kernels_render.hip): the lane that accepts the candidate -- every
// acceptance, ties included -- leaves the barycentrics tri_hit formed in its two stash words u_word, v_word, so that they are those of the best hit when
// the walk ends (a sphere leaves what is there: nobody reads them for one).  The two LDS writes sit in the candidate branch, which 5 % of the lanes take.
// A function of its own so that every other caller of wide_leaf_compute compiles as before.
template <bool POP_LEAN, class Sign>
__device__ __forceinline__ void wide_leaf_compute_uv(const WideRec& r, V3 o, V3 d, V3 inv, const Sign& sg, Trav& tr, WideStack& ws, const int* __restrict__ stack,
                                                     float* u_word, float* v_word) {
  auto f = [](unsigned v) { return __uint_as_float(v); };
  DR_MARK("leaf_begin");
  float mn[3] = {f(r.A.x), f(r.A.y), f(r.A.z)}, mx[3] = {f(r.B.x), f(r.B.y), f(r.B.z)};
  float dist;
  const int info = (int)r.A.w;
  float hit_u, hit_v;      // written by every test that can return t > 0, read by a lane that accepts; no value on the other paths: no select, no copy
  const float t = prim_hit_kind((info >> WALK_SLOT_BITS) & 3, mk(f(r.B.w), f(r.C.x), f(r.C.y)), mk(f(r.C.z), f(r.C.w), f(r.D.x)), mk(f(r.D.y), f(r.D.z), f(r.D.w)), o, d, hit_u, hit_v);
  const int slot = info & ((1 << WALK_SLOT_BITS) - 1);
  // (POP_LEAN: the wave is asked about the one compare `pos`, right where it is formed: its mask is the compare's own result.  `cand` is formed under
  // branches, and its mask takes a select and a compare more to rebuild.  The gate only spares the wave the box: a wave it lets in without a candidate finds
  // the lanes' own test closed.)
  const bool pos = t > 0.0f;
  const bool any_pos = POP_LEAN && DR_WAVE_ANY(pos);
  const bool cand = pos && (t < tr.best_t || (t == tr.best_t && (unsigned)slot < (unsigned)tr.best_slot));
  if (POP_LEAN ? any_pos : DR_WAVE_ANY(cand)) {
    if (cand && slab_sel(o, inv, sg, mn, mx, dist) && leaf_entry_admits(dist, slot, tr.best_t, tr.best_slot)) {
      tr.best_t = t; tr.best_slot = slot;
      *u_word = hit_u; *v_word = hit_v;
    }
  }
  if (POP_LEAN) wide_pop_lean(tr, ws, stack);
  else wide_pop(tr, ws, stack);
  DR_MARK("leaf_end");
}

template <bool COUNT>
__device__ __forceinline__ void wide_node_compute(const WideRec& r, V3 inv, const WideRay& wr, Trav& tr, WideStack& ws, int* __restrict__ stack, Ctr& c) {
  SignCmp sg; sg.inv = inv;
  wide_node_compute<COUNT>(r, wr, sg, tr, ws, stack, c);
}
template <bool COUNT>
__device__ __forceinline__ void wide_leaf_compute(const WideRec& r, V3 o, V3 d, V3 inv, Trav& tr, WideStack& ws, const int* __restrict__ stack, Ctr& c) {
  SignCmp sg; sg.inv = inv;
  wide_leaf_compute<COUNT>(r, o, d, inv, sg, tr, ws, stack, c);
}
template <bool COUNT>
__device__ __forceinline__ Hit closest_hit_wide(WalkRsrc wide, float pmax, float mu_e, float mu_l, float mu_v, V3 o, V3 d, Ctr& c, int* __restrict__ stack /* [word * 64] */,
                                                float cert = 1.0f /* wide_ray_margin's */, int entry = 0 /* a camera ray's: its tile's entry code */) {
  Trav tr;
  trav_begin(tr);
  tr.node = entry;
  WideStack ws; ws.top = 0u; ws.sp = 0; ws.sb = 0;
  const V3 inv = mk(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
  const WideRay wr = wide_ray(o, d, inv, pmax, mu_e, mu_l, mu_v, cert);
  if (COUNT) c.rays++;
  while (tr.node >= 0) {
    const WideRec r = wide_fetch(wide, tr.node);
    if (tr.node & 1) wide_leaf_compute<COUNT>(r, o, d, inv, tr, ws, stack, c);
    else wide_node_compute<COUNT>(r, inv, wr, tr, ws, stack, c);
  }
  Hit best; best.t = tr.best_slot < 0 ? -1.0f : tr.best_t; best.slot = tr.best_slot;
  return best;
}

}  // namespace dr
