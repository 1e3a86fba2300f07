// What is formed at a hit before any random draw: reflection and refraction, the texture fetch and the surface normal.
#pragma once
#include "device_layout.h"
#include "device_intersect.hpp"

namespace dr {

// ------------------------------------------------------------------ shading helpers
__device__ __forceinline__ V3 reflect(V3 v, V3 n) {              // K:667 (2.0*dot narrows exactly)
  float k = 2.0f * dot(v, n);
  return v - splat(k) * n;
}
__device__ __forceinline__ V3 refract(V3 uv, V3 n, float eta) {  // K:678-683
  float cos_theta = (float)fmin((double)dot(uv * splat(-1.0f), n), 1.0);
  V3 perp = splat(eta) * (uv + splat(cos_theta) * n);
  float lp = length(perp);
  float par = (float)(-__builtin_sqrt(__builtin_fabs(1.0 - (double)(lp * lp))));
  return perp + splat(par) * n;
}
__device__ __forceinline__ float reflectance(float cosine, float ref_idx) {   // K:686-691
  float r0 = (1 - ref_idx) / (1 + ref_idx);
  r0 = r0 * r0;
  float a = 1 - cosine;
  float r = a;             // pow(float, int 5): CUDA powif = square and multiply in float
  a = a * a;
  a = a * a;
  r = r * a;
  return r0 + (1 - r0) * r;
}

// tex2D<uchar4>, point / wrap / normalised (K:830,841,962; descriptor K:1959-1964)
template <bool COUNT>
__device__ __forceinline__ uint32_t tex_fetch(const DevTex* __restrict__ tex, const uint32_t* __restrict__ texels, int id,
                                              float u, float v, Ctr& c) {
  DevTex t = tex[id];
  if (COUNT) c.T++;
  float fu = u - __builtin_floorf(u), fv = v - __builtin_floorf(v);
  int i = f2i(__builtin_floorf(fu * (float)t.w)), j = f2i(__builtin_floorf(fv * (float)t.h));
  if (i > t.w - 1) i = t.w - 1;
  if (j > t.h - 1) j = t.h - 1;
  if (i < 0) i = 0;
  if (j < 0) j = 0;
  return texels[(size_t)t.offset + (size_t)j * (size_t)t.w + (size_t)i];
}
// b / 255 for a texel byte b, as the IEEE division rounds it, in three fast instructions instead of the division's eleven: with c = RN(1 / 255),
// q0 = RN(b c), the residual b - 255 q0 is exact in an fma and q = RN(q0 + residual * c) is the correctly rounded quotient (all 256 bytes are compared
// with the division in tools/host_kernel.cpp hk_check_uniform).
__device__ __forceinline__ float byte_over_255(uint32_t b) {
  const float x = float(b), c = 0x1.010102p-8f;
  const float q0 = x * c;
  return __builtin_fmaf(__builtin_fmaf(-255.0f, q0, x), c, q0);
}
__device__ __forceinline__ V3 rgb_of(uint32_t px) {
  return mk(byte_over_255(px & 255u), byte_over_255((px >> 8) & 255u), byte_over_255((px >> 16) & 255u));
}

// getnormal K:703-773 on the device records of one primitive (prims: pA..pC, shade: s0..s4, s6): the unflipped normal and the
// interpolated texture coordinate.  Barycentrics are recomputed from the ray origin, not from the hit point (K:728-745);
// the file's face normal is used unless its z is the -20 sentinel (then the cross product), vertex normals only when the
// smooth flag is set and n1.z is not the sentinel; spheres divide by the radius, other types normalise (hit - pos).
__device__ __forceinline__ V3 surface_normal(float4 pA, float4 pB, float4 pC, float4 s0, float4 s1, float4 s2, float4 s3, float4 s4, float4 s6,
                                             V3 rayo, V3 raydir, V3 hitpoint, V3& texco) {
  int type = __float_as_int(pC.y);
  texco = mk(0, 0, 0);
  V3 N;
  if (type == 0) {
    N = (hitpoint - mk(pA.x, pA.y, pA.z)) / splat(pA.w);
  } else if (type == 2) {
    V3 v0 = mk(pA.x, pA.y, pA.z), v0v1 = mk(pA.w, pB.x, pB.y), v0v2 = mk(pB.z, pB.w, pC.x);
    N = cross(v0v1, v0v2);
    V3 pvec = cross(raydir, v0v2);
    float det = dot(v0v1, pvec);
    float invDet = 1 / det;
    V3 tvec = rayo - v0;
    float ux = dot(tvec, pvec) * invDet;
    V3 qvec = cross(tvec, v0v1);
    float uy = dot(raydir, qvec) * invDet;
    float uz = 1 - ux - uy;
    // texco = uz*t1 + ux*t2 + uy*t3 (the z components of t1..t3 are never read again)
    texco.x = uz * s3.x + ux * s3.z + uy * s4.x;
    texco.y = uz * s3.y + ux * s3.w + uy * s4.y;
    V3 fn = mk(s0.x, s0.y, s0.z);
    if (fn.z != -20) {
      N = fn;
      int flags = __float_as_int(s6.z);
      if (s1.y != -20 && (flags & 1)) {     // n1.z
        V3 n1 = mk(s0.w, s1.x, s1.y), n2 = mk(s1.z, s1.w, s2.x), n3 = mk(s2.y, s2.z, s2.w);
        N = splat(uz) * n1 + splat(ux) * n2 + splat(uy) * n3;
      }
    }
    N = normalized(N);
  } else {
    N = normalized(hitpoint - mk(pA.x, pA.y, pA.z));
  }
  return N;
}
// surface_normal in the pieces the lean persistent build puts together (device_shade.hpp shade_prepare_hit), which may know a hit's barycentrics already
// and looks at the primitive record only where a lane reads it.  The arithmetic is the block's above, operation by operation.
//  prim_normal: what the block takes from the primitive record apart from the barycentrics -- a sphere's normal, cross(e1, e2) of a triangle (used when the
//  file's face normal is the -20 sentinel), the normalised offset of any other type;
__device__ __forceinline__ V3 prim_normal(int type, float4 pA, float4 pB, float4 pC, V3 hitpoint) {
  if (type == 0) return (hitpoint - mk(pA.x, pA.y, pA.z)) / splat(pA.w);
  if (type == 2) return cross(mk(pA.w, pB.x, pB.y), mk(pB.z, pB.w, pC.x));
  return normalized(hitpoint - mk(pA.x, pA.y, pA.z));
}
//  tri_barycentrics: ux, uy of a triangle from the ray's origin (K:728-745) -- bit for bit the u, v of the tri_hit that accepted the hit;
__device__ __forceinline__ void tri_barycentrics(float4 pA, float4 pB, float4 pC, V3 rayo, V3 raydir, float& ux, float& uy) {
  V3 v0 = mk(pA.x, pA.y, pA.z), v0v1 = mk(pA.w, pB.x, pB.y), v0v2 = mk(pB.z, pB.w, pC.x);
  V3 pvec = cross(raydir, v0v2);
  float det = dot(v0v1, pvec);
  float invDet = 1 / det;
  V3 tvec = rayo - v0;
  ux = dot(tvec, pvec) * invDet;
  V3 qvec = cross(tvec, v0v1);
  uy = dot(raydir, qvec) * invDet;
}
//  texco_of: the interpolated texture coordinate (s3: t1, t2; s4.xy: t3);
__device__ __forceinline__ V3 texco_of(float ux, float uy, float4 s3, float4 s4) {
  float uz = 1 - ux - uy;
  V3 texco = mk(0, 0, 0);
  texco.x = uz * s3.x + ux * s3.z + uy * s4.x;
  texco.y = uz * s3.y + ux * s3.w + uy * s4.y;
  return texco;
}
//  shade_normal: the unflipped normal from prim_normal's Ng, a triangle's barycentrics and the normals of the shade record.
__device__ __forceinline__ V3 shade_normal(int type, V3 Ng, float ux, float uy, float4 s0, float4 s1, float4 s2, float4 s6) {
  if (type != 2) return Ng;
  V3 N = Ng;
  float uz = 1 - ux - uy;
  V3 fn = mk(s0.x, s0.y, s0.z);
  if (fn.z != -20) {
    N = fn;
    int flags = __float_as_int(s6.z);
    if (s1.y != -20 && (flags & 1)) {     // n1.z
      V3 n1 = mk(s0.w, s1.x, s1.y), n2 = mk(s1.z, s1.w, s2.x), n3 = mk(s2.y, s2.z, s2.w);
      N = splat(uz) * n1 + splat(ux) * n2 + splat(uy) * n3;
    }
  }
  return normalized(N);
}

}  // namespace dr
