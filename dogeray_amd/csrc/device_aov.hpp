// The first hit of a pixel's pinhole ray and what shading would form there (dr_render_aov).
#pragma once
#include "device_surface.hpp"

namespace dr {

// ------------------------------------------------------------------ first-hit AOVs (dr_render_aov)
// What pixel (x, y) sees through the pinhole: the ray through the pixel CENTRE (nu = (x + 0.5) / den_w as camera_prepare forms it with the
// jitter replaced by 0.5; camera_finish without the lens offset: origin = from, K:1066-1073), its closest hit (hit() K:468-512, through `closest`)
// and what shade_prepare (K:807-844) forms there before any random draw: the facing normal, the texture coordinate and ocolor.  A sibling of
// shade_prepare, not a caller of it, so that the render kernels' code stays exactly as it is.  No random number, no counter.
struct AovHit {
  V3 dir;              // the ray direction as traced (unnormalised)
  float t;             // hit()'s t: > 0 on a hit, -1 on a miss
  int slot;            // -1 on a miss
  float distance;      // t * |dir|, +inf on a miss
  float depth;         // t * focus: every pinhole direction has the focus distance as its component along -w (K:1047-1049); +inf on a miss
  int mat;             // the object's mat, -1 on a miss
  V3 normal;           // surface_normal flipped to face the ray (K:807-825), 0 on a miss
  float u, v;          // texco.x, texco.y, 0 on a miss
  V3 albedo;           // ocolor (K:826-844), 0 on a miss
};
template <class Closest>
__device__ __forceinline__ AovHit aov_first_hit(const RenderParams& P, const Closest& closest, float focus, int x, int y) {
  AovHit a;
  const float nu = (float)(((double)x + 0.5) / P.den_w), nv = (float)(((double)y + 0.5) / P.den_h);
  const V3 from = ld3(P.from);
  a.dir = ld3(P.llc) + splat(nu) * ld3(P.hor) + splat(nv) * ld3(P.ver) - from;
  Ctr c = {0, 0, 0, 0, 0, 0, 0, 0};
  const Hit h = closest(from, a.dir, c);
  a.t = h.t;
  const float inf = __builtin_inff();
  a.slot = -1; a.distance = inf; a.depth = inf; a.mat = -1;
  a.normal = mk(0, 0, 0); a.u = 0; a.v = 0; a.albedo = mk(0, 0, 0);
  if (!(h.t > 0.0f)) return a;                                    // the miss branch of raycolor (K:951)
  a.slot = h.slot;
  a.distance = h.t * length(a.dir);
  a.depth = h.t * focus;
  const V3 hitpoint = from + splat(h.t) * a.dir;                  // K:806
  const float4* pp = reinterpret_cast<const float4*>(P.prims + h.slot);
  const float4* sp = reinterpret_cast<const float4*>(P.shade + h.slot);
  const float4 pA = pp[0], pB = pp[1], pC = pp[2];
  const float4 s0 = sp[0], s1 = sp[1], s2 = sp[2], s3 = sp[3], s4 = sp[4], s5 = sp[5], s6 = sp[6];
  V3 texco;
  V3 N = surface_normal(pA, pB, pC, s0, s1, s2, s3, s4, s6, from, a.dir, hitpoint, texco);
  a.normal = dot(a.dir, N) < 0 ? N : N * splat(-1.0f);
  a.u = texco.x; a.v = texco.y;
  const V3 col = mk(s4.z, s4.w, s5.x);
  a.mat = __float_as_int(s5.w);
  const int texnum = __float_as_int(s6.x), flags = __float_as_int(s6.z);
  a.albedo = col;
  if (texnum >= 0) {
    a.albedo = rgb_of(tex_fetch<false>(P.tex, P.texels, texnum, texco.x, -texco.y + 1, c));
  } else if (flags & 2) {                                         // checker K:776-784
    const float u2 = __builtin_floorf(texco.x * 10), v2 = __builtin_floorf(texco.y * 10);
    const float yes = u2 + v2;
    a.albedo = (__builtin_fmodf(yes, 2.0f) == 0) ? splat(0.8f) : col;
  }
  return a;
}

// The same for a caller's ray (dr_trace_rays): what shade_prepare forms at the hit (t, slot) of the ray (o, d), with the meaning, the miss values and the
// arithmetic of aov_first_hit's fields of the same name; the origin is the ray's own, not the camera.  depth is a pinhole's: +inf here.  A sibling of
// aov_first_hit, which stays as it is (the AOV kernel's code does not move).
__device__ __forceinline__ AovHit ray_surface(const RenderParams& P, V3 o, V3 d, float t, int slot) {
  AovHit a;
  a.dir = d;
  a.t = t;
  const float inf = __builtin_inff();
  a.slot = -1; a.distance = inf; a.depth = inf; a.mat = -1;
  a.normal = mk(0, 0, 0); a.u = 0; a.v = 0; a.albedo = mk(0, 0, 0);
  if (!(t > 0.0f) || slot < 0) { a.t = -1.0f; return a; }
  a.slot = slot;
  a.distance = t * length(d);
  const V3 hitpoint = o + splat(t) * d;                           // K:806
  const float4* pp = reinterpret_cast<const float4*>(P.prims + slot);
  const float4* sp = reinterpret_cast<const float4*>(P.shade + slot);
  const float4 pA = pp[0], pB = pp[1], pC = pp[2];
  const float4 s0 = sp[0], s1 = sp[1], s2 = sp[2], s3 = sp[3], s4 = sp[4], s5 = sp[5], s6 = sp[6];
  V3 texco;
  V3 N = surface_normal(pA, pB, pC, s0, s1, s2, s3, s4, s6, o, d, hitpoint, texco);
  a.normal = dot(d, N) < 0 ? N : N * splat(-1.0f);
  a.u = texco.x; a.v = texco.y;
  const V3 col = mk(s4.z, s4.w, s5.x);
  a.mat = __float_as_int(s5.w);
  const int texnum = __float_as_int(s6.x), flags = __float_as_int(s6.z);
  a.albedo = col;
  Ctr c = {0, 0, 0, 0, 0, 0, 0, 0};
  if (texnum >= 0) {
    a.albedo = rgb_of(tex_fetch<false>(P.tex, P.texels, texnum, texco.x, -texco.y + 1, c));
  } else if (flags & 2) {                                         // checker K:776-784
    const float u2 = __builtin_floorf(texco.x * 10), v2 = __builtin_floorf(texco.y * 10);
    const float yes = u2 + v2;
    a.albedo = (__builtin_fmodf(yes, 2.0f) == 0) ? splat(0.8f) : col;
  }
  return a;
}

}  // namespace dr
