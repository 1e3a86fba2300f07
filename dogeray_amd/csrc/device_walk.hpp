// The walks over the binary tree: the threaded walk (one step at a time, with or without parked leaves) and the ordered, near-first walk.
#pragma once
#include "device_intersect.hpp"

namespace dr {

// hit() K:468-512 in the reference's order, over the walk array (device_layout.h): a node that
// is entered continues with its hit link (its first child), a node that is skipped, and every
// leaf, with its miss link.  The link says whether its target is a leaf, so a leaf's box and
// primitive are fetched together and the triangle test costs no second memory round trip.
// The loop body is its own function so that the persistent kernel can interleave node steps of
// different rays (lanes re-armed while their neighbours are still walking).
struct Trav { int node; float best_t; int best_slot; };   // node: link to visit next, < 0 = walk finished
// ... and what a kernel that keeps its lanes as a pool of ray slots (render_persistent_kernel, trace_probe_kernel) tells apart below 0
constexpr int LANE_DONE = -1;        // walk finished (what the walks leave behind): the hit waits to be shaded / written
constexpr int LANE_REFILL = -2;      // needs a new ray: the next sample, or a new pixel
constexpr int LANE_RETIRED = -3;     // nothing left to take

// Which lanes of a wave take one step of the wide walk (render_persistent_kernel's rule, as a function of masks alone: tests/test_step_masks_host.py).
// leaves / nodes: the walking lanes that stand at a leaf / at a node.  The leaf lanes wait until `leaf_min` of them stand at one, nobody can take a node
// step, or the wave drains; with exclusive steps the node lanes sit out a leaf step unless the wave drains.  A lane in neither mask never steps.
struct StepMasks { unsigned long long step, leaf; };      // the lanes that step, and those of them that step as leaves
__device__ __forceinline__ StepMasks step_masks(unsigned long long leaves, unsigned long long nodes, bool draining, int leaf_min, bool exclusive) {
  const bool do_leaves = leaves != 0ull && (wave_count(leaves) >= leaf_min || nodes == 0ull || draining);
  const bool do_nodes = !exclusive || !do_leaves || draining;
  StepMasks m;
  m.leaf = do_leaves ? leaves : 0ull;
  m.step = m.leaf | (do_nodes ? nodes : 0ull);
  return m;
}

// "No hit yet" is t = 10000: singlehit only returns distances below 10000 (K:449) and aabb2's exit distance starts at 10000 (K:246), so every
// comparison against the running best (box entry < best, t < best) comes out as with the 1e7 of hit() K:470 -- and the wide walk's node
// test needs no min(best, 10000) of its own.
__device__ __forceinline__ void trav_begin(Trav& tr) { tr.node = 0; tr.best_t = 10000.0f; tr.best_slot = -1; }

// The walk array is read through a buffer descriptor with 128-bit buffer loads: the compiler may
// not re-slice those into narrower / unaligned pieces (it does so with plain float4 loads: the box
// came in as dwordx2 + unaligned dwordx4 + dwordx3), so a node costs exactly two 16-byte requests
// and a leaf four, all issued before the first wait.
// (WalkRsrc, make_rsrc and the raw load ld_unit_raw: device_prims.hpp)
__device__ __forceinline__ WalkRsrc walk_rsrc(const RenderParams& P) { return make_rsrc(P.walk, P.walk_bytes); }
__device__ __forceinline__ WalkRsrc wide_rsrc(const RenderParams& P) { return make_rsrc(P.wide, P.wide_bytes); }
__device__ __forceinline__ float4 ld_unit(WalkRsrc r, unsigned byte_off) {
  u32x4 v = ld_unit_raw(r, byte_off);
  return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
}

template <bool COUNT>
__device__ __forceinline__ void trav_step(WalkRsrc walk, V3 o, V3 d, V3 inv, Trav& tr, Ctr& c) {
  const bool leaf = tr.node & 1;
  const unsigned off = (unsigned)(tr.node >> 1) << 4;
  float4 A = ld_unit(walk, off), B = ld_unit(walk, off + 16);
  float4 C = A, D = A;
  if (leaf) { C = ld_unit(walk, off + 32); D = ld_unit(walk, off + 48); }
  float mn[3] = {A.x, A.y, A.z}, mx[3] = {B.x, B.y, B.z};
  const int w0 = __float_as_int(A.w);
  const int next_miss = leaf ? leaf_successor<COUNT>(tr.node, w0) : __float_as_int(B.w);
  float dist;
  if (COUNT) c.V++;
  bool h = slab(o, inv, mn, mx, dist);
  if (h && dist < tr.best_t) {
    if (leaf) {
      if (COUNT) c.L++;
      float t = prim_hit_kind((w0 >> WALK_SLOT_BITS) & 3, mk(B.w, C.x, C.y), mk(C.z, C.w, D.x), mk(D.y, D.z, D.w), o, d);
      if (t > -0.01f && t < tr.best_t) { tr.best_t = t; tr.best_slot = w0 & ((1 << WALK_SLOT_BITS) - 1); }   // K:488 (t is -1 or > 0)
      tr.node = next_miss;
    } else {
      tr.node = w0;
    }
  } else {
    tr.node = next_miss;
  }
}

// Same step, but a leaf whose box passes is not tested on the spot: the lane keeps the primitive
// it has just fetched and waits ("parks") until enough lanes of the wave have one, so the
// ~90-instruction triangle test runs once for many lanes instead of on nearly every iteration for
// one or two.  The per-lane sequence of tests and updates is unchanged.
// C and D stay 128-bit register tuples from the load to the test (as scalars the allocator scattered them and
// copied all eight back and forth on every step).
struct ParkedLeaf { float v0x; u32x4 C, D; int info; bool parked; };

template <bool COUNT>
__device__ __forceinline__ void trav_step_park(WalkRsrc walk, V3 o, V3 inv, Trav& tr, ParkedLeaf& pk, Ctr& c) {
  const bool leaf = tr.node & 1;
  const unsigned off = (unsigned)(tr.node >> 1) << 4;
  float4 A = ld_unit(walk, off), B = ld_unit(walk, off + 16);
  // a stepping lane is not parked, so its parked record is free: the leaf's primitive lands there directly
  if (leaf) { pk.C = ld_unit_raw(walk, off + 32); pk.D = ld_unit_raw(walk, off + 48); }
  float mn[3] = {A.x, A.y, A.z}, mx[3] = {B.x, B.y, B.z};
  const int w0 = __float_as_int(A.w);
  // selects, not branches: both sides are two or three instructions, a divergent branch costs more than that
  const int succ = leaf_successor<COUNT>(tr.node, w0);
  const int next_miss = leaf ? succ : __float_as_int(B.w);
  float dist;
  if (COUNT) c.V++;
  bool h = slab(o, inv, mn, mx, dist) && dist < tr.best_t;
  pk.info = leaf ? w0 : pk.info;
  pk.v0x = leaf ? B.w : pk.v0x;
  pk.parked = h && leaf;
  tr.node = (h && !leaf) ? w0 : next_miss;
}
template <bool COUNT>
__device__ __forceinline__ void parked_test(V3 o, V3 d, Trav& tr, ParkedLeaf& pk, Ctr& c) {
  if (COUNT) c.L++;
  auto f = [](unsigned v) { return __uint_as_float(v); };
  float t = prim_hit_kind((pk.info >> WALK_SLOT_BITS) & 3, mk(pk.v0x, f(pk.C.x), f(pk.C.y)), mk(f(pk.C.z), f(pk.C.w), f(pk.D.x)), mk(f(pk.D.y), f(pk.D.z), f(pk.D.w)), o, d);
  if (t > -0.01f && t < tr.best_t) { tr.best_t = t; tr.best_slot = pk.info & ((1 << WALK_SLOT_BITS) - 1); }   // K:488
  pk.parked = false;
}

template <bool COUNT>
__device__ __forceinline__ Hit closest_hit_threaded(WalkRsrc walk, V3 o, V3 d, Ctr& c) {
  Trav tr;
  trav_begin(tr);
  V3 inv = mk(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
  if (COUNT) { c.rays++; if (first_active_lane()) c.ray_slots += 64; }
  while (tr.node >= 0) {
    if (COUNT) { if (first_active_lane()) c.trav_slots += 64; }
    trav_step<COUNT>(walk, o, d, inv, tr, c);
  }
  Hit best; best.t = tr.best_slot < 0 ? -1.0f : tr.best_t; best.slot = tr.best_slot;
  return best;
}

// hit() K:468-512 with the children visited near-first instead of child-0-first.
//
// What the reference returns is the primitive with the smallest t among all leaves whose
// boxes (and ancestors' boxes) the ray enters, and, among equal t, the one its child-0-first
// walk reaches first -- which is the one with the lowest leaf rank = slot (device_layout.h).
// So any visiting order gives the same answer as long as (1) a subtree is skipped only when
// its box is missed or entered no nearer than the best t so far (the reference's own pruning
// test, K:484) and (2) ties on t go to the lower slot.  One 64-byte record holds both child
// boxes; the far child waits on a per-lane stack in LDS (one dword per level, lane-major, so
// a wave's pushes and pops never bank-conflict).  The tree is a median split, so its depth is
// ceil(log2 N) <= 24 for N <= 2^24 (the host refuses deeper trees for this mode).
//
// (1) and (2) assume that a leaf's computed entry distance does not exceed the computed t of its primitive.  Where it does (coordinates of 2^20: floats step
// by more than the 0.01 of padding) hit() decides between two leaves by its ORDER: the one it reaches later (higher slot) wins only if its box entry AND its t
// are both < the earlier one's t (K:484, K:488).  This walk keeps m = max(entry, t) of its best leaf and decides every pair that way, whichever of the two
// it met first; it prunes at m, not at t, so that an earlier leaf whose t lies between the best's t and the best's entry is still looked at.  With entry <= t
// everywhere m is t and all of this is the lexicographic minimum above, bit for bit.
template <bool COUNT>
__device__ __forceinline__ Hit closest_hit_ordered(const DevPair* __restrict__ pairs, const DevPrim* __restrict__ prims,
                                                   V3 o, V3 d, Ctr& c, int* __restrict__ stack /* [level * 64] */) {
  Hit best; best.t = 10000000.0f; best.slot = 0x7fffffff;
  float best_m = 10000000.0f;
  auto offer = [&best, &best_m](float t, int slot, float entry) {
    if (!(t > 0.0f)) return;
    const float m = __builtin_fmaxf(entry, t);
    const bool take = slot > best.slot ? m < best.t : !(best_m < t);      // the later of the two wins only if it is nearer in both respects
    if (take) { best.t = t; best.slot = slot; best_m = m; }
  };
  V3 inv = mk(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
  int sp = 0;
  int cur = 0;
  if (COUNT) c.rays++;
  for (;;) {
    const float4* pp = reinterpret_cast<const float4*>(pairs + cur);
    float4 A = pp[0], B = pp[1], C = pp[2], D = pp[3];
    int c0 = __float_as_int(A.w), c1 = __float_as_int(B.w);
    float mn0[3] = {A.x, A.y, A.z}, mx0[3] = {B.x, B.y, B.z};
    float mn1[3] = {C.x, C.y, C.z}, mx1[3] = {D.x, D.y, D.z};
    float d0, d1;
    if (COUNT) c.V += 2;
    bool h0 = slab(o, inv, mn0, mx0, d0) && d0 <= best_m;     // <=: a box entered exactly at the best t may hold a tie with a lower slot
    bool h1 = slab(o, inv, mn1, mx1, d1) && d1 <= best_m;
    if (h0 && c0 < 0) {
      int slot = ~c0;
      if (COUNT) c.L++;
      offer(prim_hit(prims, slot, o, d), slot, d0);
      h0 = false;
    }
    if (h1 && c1 < 0) {
      if (d1 <= best_m) {
        int slot = ~c1;
        if (COUNT) c.L++;
        offer(prim_hit(prims, slot, o, d), slot, d1);
      }
      h1 = false;
    }
    h0 = h0 && d0 <= best_m;
    h1 = h1 && d1 <= best_m;
    if (h0 && h1) {
      bool first0 = d0 <= d1;
      int far_c = first0 ? c1 : c0;
      cur = first0 ? c0 : c1;
      if (sp < ORDERED_STACK) { stack[sp * 64] = far_c; sp++; }
    } else if (h0) {
      cur = c0;
    } else if (h1) {
      cur = c1;
    } else {
      if (sp == 0) break;
      sp--;
      cur = stack[sp * 64];
    }
  }
  if (best.slot == 0x7fffffff) { best.t = -1.0f; best.slot = -1; }
  return best;
}

}  // namespace dr
