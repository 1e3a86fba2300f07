// The wave loop of the persistent kernels that walk a LIST of caller rays (trace_persistent_kernel, allhits_persistent_kernel, radiance_persistent_kernel,
// trace_probe_kernel): a wave's lanes are a pool of ray slots.  Two pieces, each written once here: how a wave takes rays from the list (ListFeed), and the
// round of node and leaf steps between two looks at the list (list_walk_round).  A kernel keeps what is its own: what a finished lane stores, what a new ray
// initialises, what a leaf step does (radiance: its shade phase too).  Device only.  (render_persistent_kernel is not of this family: its lanes refill from
// a queue of tiles, kernels_render.hip.)
#pragma once
#include "device_wide.hpp"

namespace dr {

// What a lane that asked for a ray got: the ray's index (ok), or the state it is in now -- LANE_RETIRED: the list is used up; LANE_REFILL: the wave's
// chunk ran out in the middle of the wave's request, ask again at the next refill
struct ListItem { unsigned index; bool ok; int state; };

// A wave's share of the list: rays [chunk_next, chunk_end) of the chunk it took last, and whether the list has nothing more for this wave.  All three are
// the same in every lane -- they come from ballots, a readfirstlane and the kernel's arguments only --, so they live in scalar registers; keep it so.
struct ListFeed {
  unsigned chunk_next = 0, chunk_end = 0;
  bool exhausted = false;
  // The lanes of `mask` -- a ballot, not empty -- each ask for a ray of the n; call it with the whole wave.  Rays come in chunks of CHUNK per wave, one
  // atomicAdd on the launch's cursor per chunk (a cursor touched at every refill is the bottleneck: 0.35 Grays/s in trace_probe_kernel): the wave takes a
  // new chunk only when its last one is used up, and a request larger than the chunk's rest gets the rest -- the tail rule: lane ranks `my` past the chunk's
  // end stay LANE_REFILL, past n they retire.  The result means something in the lanes of `mask` only.
  // (`chunk_next + cnt > chunk_end && chunk_next >= chunk_end` is `chunk_next >= chunk_end` written long: cnt > 0, the mask is not empty.  The long form is
  // kept because three of the four kernels were compiled from it.)
  template <unsigned CHUNK>
  __device__ __forceinline__ ListItem take(unsigned long long mask, unsigned* cursor, unsigned n) {
    if (exhausted) return ListItem{0u, false, LANE_RETIRED};
    const int cnt = (int)__popcll(mask);
    if (chunk_next + (unsigned)cnt > chunk_end && chunk_next >= chunk_end) {
      unsigned b = 0;
      if ((threadIdx.x & 63) == 0) b = atomicAdd(cursor, CHUNK);
      chunk_next = (unsigned)__builtin_amdgcn_readfirstlane((int)b); chunk_end = chunk_next + CHUNK;
    }
    const unsigned base = chunk_next;
    const unsigned my = base + (unsigned)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
    chunk_next = base + (unsigned)cnt < chunk_end ? base + (unsigned)cnt : chunk_end;
    const ListItem it = {my, my < n && my < chunk_end, my >= n ? LANE_RETIRED : LANE_REFILL};
    exhausted = chunk_next >= n;
    return it;
  }
};

// Two steps of the wide walk for the wave's walking lanes (tr.node >= 0), node steps and leaf steps exclusive: the lanes at a leaf wait until PARK of them
// stand there (or nobody is at a node, or the list is used up: nothing is gained by waiting), then they step alone.  leaf(r): the kernel's leaf step on
// record r -- it leaves tr at the lane's next record or LANE_DONE.
template <int PARK, class Leaf>
__device__ __forceinline__ void list_walk_round(const WalkRsrc& walk, const WideRay& wr, const SignMask& sg, bool exhausted, Trav& tr, WideStack& ws,
                                                int* my_stack, Ctr& c, Leaf&& leaf) {
  for (int u = 0; u < 2; u++) {
    const bool at_leaf = tr.node >= 0 && (tr.node & 1);
    const unsigned long long leaves = __ballot(at_leaf), nodes = __ballot(tr.node >= 0 && !(tr.node & 1));
    const bool do_leaves = leaves != 0ull && ((int)__popcll(leaves) >= PARK || nodes == 0ull || exhausted);
    const bool do_nodes = !do_leaves || exhausted;
    if (tr.node >= 0 && (at_leaf ? do_leaves : do_nodes)) {
      const WideRec r = wide_fetch(walk, tr.node);
      if (at_leaf) leaf(r);
      else wide_node_compute<false>(r, wr, sg, tr, ws, my_stack, c);
    }
  }
}

}  // namespace dr
