// The walks of caller rays (dr_trace_rays): the closest hit at t <= tmax, and the any-hit walk that stops as soon as the answer is known to be a hit.
#pragma once
#include "device_wide.hpp"
#include "../../include/dogeray_amd.h"

namespace dr {

// ------------------------------------------------------------------ capped and any-hit walks
// The answer for a ray with cap = min(tmax, 10000) is hit()'s own answer H (K:468-512) if t_H <= cap, else a miss -- for EVERY ray.  Each walk below is
// its closest_hit_* sibling (device_walk.hpp, device_wide.hpp): same start value, node step, leaf step and candidate rule, so the sequence of accepted
// primitives is the sibling's, which is hit()'s answer bit for bit (tests/test_rays_host.py).
//
// Why the boxes are NOT pruned against the cap.  A walk whose running best starts at (cap, no slot) skips every box entered behind the cap (K:484).  That
// is the same answer only while no leaf's computed box entry exceeds the computed t of the primitive inside it; it does at coordinates around 2^20 (the
// leaf-entry corner of device_intersect.hpp) and for a few accepted hits of grazing rays and sliver triangles whose float t lies in front of their own
// padded box (9 of 18 000 `graze` rays of tests/ray_cases.py grid_mixed; one ray of `degenerate` with an entry beyond 2 t): such a hit at t <= tmax came
// back as a miss -- a shadow ray that leaks.  No bound on entry - t holds for every triangle a scene may contain, so the cap decides candidates at the end
// of the walk, not boxes during it.
//
// ANY: the loop is left as soon as the final answer is known to be a hit.  In the threaded and the wide walk the running best t never grows, so that is
// "a primitive is held at t <= cap".  In the ordered walk an earlier leaf may replace the best with a LARGER t, up to the best's m = max(entry, t)
// (closest_hit_ordered), so there it is m <= cap; otherwise the walk runs to its end and the final t decides.
//
// tmax NaN or <= 0: no walk, a miss (trace_cap returns 0).
__device__ __forceinline__ float trace_cap(float tmax) { return tmax > 0.0f ? __builtin_fminf(tmax, 10000.0f) : 0.0f; }

__device__ __forceinline__ Hit trace_result(float best_t, int best_slot, float cap) {
  Hit h;
  const bool hit = best_slot >= 0 && best_t <= cap;
  h.t = hit ? best_t : -1.0f; h.slot = hit ? best_slot : -1;
  return h;
}

template <bool COUNT, bool ANY>
__device__ __forceinline__ Hit trace_threaded(WalkRsrc walk, V3 o, V3 d, float cap, Ctr& c) {
  Trav tr;
  trav_begin(tr);
  const V3 inv = mk(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
  if (COUNT) c.rays++;
  while (tr.node >= 0) {
    trav_step<COUNT>(walk, o, d, inv, tr, c);
    if (ANY && tr.best_slot >= 0 && tr.best_t <= cap) break;
  }
  return trace_result(tr.best_t, tr.best_slot, cap);
}

// closest_hit_ordered, statement by statement, with ANY's exit.  A COPY, because device_walk.hpp stays byte-identical for the render kernels' sake:
// whoever changes one changes the other (tests/test_trace_host.py holds both to the oracle), and a later change should merge them through one template.
template <bool COUNT, bool ANY>
__device__ __forceinline__ Hit trace_ordered(const DevPair* __restrict__ pairs, const DevPrim* __restrict__ prims, V3 o, V3 d, float cap, Ctr& c,
                                             int* __restrict__ stack /* [level * 64] */) {
  Hit best; best.t = 10000000.0f; best.slot = 0x7fffffff;
  float best_m = 10000000.0f;
  auto offer = [&best, &best_m](float t, int slot, float entry) {
    if (!(t > 0.0f)) return;
    const float m = __builtin_fmaxf(entry, t);
    const bool take = slot > best.slot ? m < best.t : !(best_m < t);
    if (take) { best.t = t; best.slot = slot; best_m = m; }
  };
  const V3 inv = mk(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
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
    bool h0 = slab(o, inv, mn0, mx0, d0) && d0 <= best_m;
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
    if (ANY && best.slot != 0x7fffffff && best_m <= cap) break;      // whatever replaces the best from here on has t <= best_m
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
  return trace_result(best.t, best.slot == 0x7fffffff ? -1 : best.slot, cap);
}

template <bool COUNT, bool ANY>
__device__ __forceinline__ Hit trace_wide(WalkRsrc wide, float pmax, float mu_e, float mu_l, float mu_v, V3 o, V3 d, float cap, Ctr& c,
                                          int* __restrict__ stack /* [word * 64] */) {
  Trav tr;
  trav_begin(tr);
  WideStack ws; ws.top = 0u; ws.sp = 0; ws.sb = 0;
  const V3 inv = mk(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
  const WideRay wr = wide_ray(o, d, inv, pmax, mu_e, mu_l, mu_v);
  if (COUNT) c.rays++;
  while (tr.node >= 0) {
    const WideRec r = wide_fetch(wide, tr.node);
    if (tr.node & 1) {
      wide_leaf_compute<COUNT>(r, o, d, inv, tr, ws, stack, c);
      if (ANY && tr.best_slot >= 0 && tr.best_t <= cap) break;
    } else wide_node_compute<COUNT>(r, inv, wr, tr, ws, stack, c);
  }
  return trace_result(tr.best_t, tr.best_slot, cap);
}

// One caller ray by the walk of `mode` (DR_TRAVERSAL_*; the caller has mapped a scene without a wide tree to the threaded walk): a miss without a walk
// for a tmax that admits nothing.  stack: the lane's LDS words (unused by the threaded walk).
template <int MODE, bool COUNT, bool ANY>
__device__ __forceinline__ Hit trace_ray(const RenderParams& P, V3 o, V3 d, float tmax, Ctr& c, int* __restrict__ stack) {
  const float cap = trace_cap(tmax);
  Hit miss; miss.t = -1.0f; miss.slot = -1;
  if (!(cap > 0.0f)) return miss;
  if (MODE == DR_TRAVERSAL_ORDERED) return trace_ordered<COUNT, ANY>(P.pairs, P.prims, o, d, cap, c, stack);
  if (MODE == DR_TRAVERSAL_WIDE) return trace_wide<COUNT, ANY>(wide_rsrc(P), P.wide_pmax, P.wide_mu.e, P.wide_mu.l, P.wide_mu.v, o, d, cap, c, stack);
  return trace_threaded<COUNT, ANY>(walk_rsrc(P), o, d, cap, c);
}

}  // namespace dr
