// The known-answer hooks of the shading step (dr_kat_sample, dr_kat_outside, dr_kat_tex, dr_kat_bounce, dr_kat_miss, dr_kat_camera, dr_kat_store), one
// element per lane: each body calls the product's functions of device_rng.hpp, device_surface.hpp and device_shade.hpp unchanged and writes what they
// return.  kernels_kat.hip runs them on the device, tools/host_kernel.cpp (hk_kat_*) in a loop on the host.  No render kernel includes this file.
#pragma once
#include "device_shade.hpp"

namespace dr {

__device__ __forceinline__ void kat_st3(float* p, V3 v) { p[0] = v.x; p[1] = v.y; p[2] = v.z; }
__device__ __forceinline__ Xorwow kat_generator(uint64_t seed, int warm) {
  Xorwow r; r.init(seed);
  for (int k = 0; k < warm; k++) r.next();
  return r;
}

// Both forms of the rejection samplers on copies of one generator state: the plain loops (rand_in_unit_sphere kind 3, rand_in_unit_disk kind 2, nothing
// kind 0) and rand_points_merged with the lane's kind -- on the device one loop for the whole wave, its lanes' kinds mixed as a phase of the persistent
// kernel mixes them.  Per form the point and the generator's two following outputs.
__device__ __forceinline__ void kat_sample_lane(int i, const uint64_t* seed, const int32_t* warm, const int32_t* kind, float* p_plain, uint32_t* n_plain,
                                                float* p_merged, uint32_t* n_merged) {
  const Xorwow r0 = kat_generator(seed[i], warm[i]);
  const int k = kind[i];
  Xorwow a = r0, b = r0;
  V3 pa = mk(0, 0, 0);
  if (k == 3) pa = rand_in_unit_sphere(a);
  else if (k == 2) pa = rand_in_unit_disk(a);
  const V3 pb = rand_points_merged<false>(b, k);
  kat_st3(p_plain + 3 * i, pa); kat_st3(p_merged + 3 * i, pb);
  n_plain[2 * i] = a.next(); n_plain[2 * i + 1] = a.next();
  n_merged[2 * i] = b.next(); n_merged[2 * i + 1] = b.next();
}

__device__ __forceinline__ void kat_outside_lane(int i, const float* d2, int32_t* out) { out[i] = outside_unit(d2[i]) ? 1 : 0; }

__device__ __forceinline__ void kat_tex_lane(const RenderParams& P, int i, const int32_t* tex, const float* u, const float* v, uint32_t* rgba) {
  Ctr c = {0, 0, 0, 0, 0, 0, 0, 0};
  rgba[i] = tex_fetch<false>(P.tex, P.texels, tex[i], u[i], v[i], c);
}

// One bounce at a given t, both ways, each on a copy of one generator state: shade_hit<false>, and the persistent kernel's split -- shade_prepare, the
// point of rand_points_merged (kind 3 where shade_needs_sphere, else 0), shade_scatter.  Per form: alive (1: the path continues; 0: it ended at an
// emissive surface and atten holds its radiance, the ray as it came), the ray and the attenuation afterwards, the generator's two following outputs.
__device__ __forceinline__ void kat_bounce_lane(const RenderParams& P, int i, const int32_t* slot, const float* o, const float* d, const float* t,
                                                const float* atten, const uint64_t* seed, const int32_t* warm, int32_t* alive2, float* o2, float* d2,
                                                float* atten2, uint32_t* next2, int n) {
  const Xorwow r0 = kat_generator(seed[i], warm[i]);
  Path p0; p0.rayo = ld3(o + 3 * i); p0.raydir = ld3(d + 3 * i); p0.atten = ld3(atten + 3 * i);
  Ctr c = {0, 0, 0, 0, 0, 0, 0, 0};
  // form 0: shade_hit
  Path pa = p0; Xorwow a = r0; V3 ea = mk(0, 0, 0);
  const bool alive_a = shade_hit<false>(P, pa, t[i], slot[i], a, c, ea);
  // form 1: the split
  Path pb = p0; Xorwow b = r0; V3 eb = mk(0, 0, 0);
  ShadeCtx sc;
  const bool alive_b = shade_prepare<false>(P, pb, t[i], slot[i], b, c, sc, eb);
  const V3 rs = rand_points_merged<false>(b, alive_b && shade_needs_sphere(sc) ? 3 : 0);
  if (alive_b) shade_scatter(pb, sc, rs, b);
  const size_t ia = (size_t)i, ib = (size_t)n + (size_t)i;      // form f of element i at f * n + i
  alive2[ia] = alive_a; alive2[ib] = alive_b;
  kat_st3(o2 + 3 * ia, pa.rayo); kat_st3(d2 + 3 * ia, pa.raydir); kat_st3(atten2 + 3 * ia, alive_a ? pa.atten : ea);
  kat_st3(o2 + 3 * ib, pb.rayo); kat_st3(d2 + 3 * ib, pb.raydir); kat_st3(atten2 + 3 * ib, alive_b ? pb.atten : eb);
  next2[2 * ia] = a.next(); next2[2 * ia + 1] = a.next();
  next2[2 * ib] = b.next(); next2[2 * ib + 1] = b.next();
}

// shade_miss for direction d and attenuation atten (P: backtex, bgint, the textures)
__device__ __forceinline__ void kat_miss_lane(const RenderParams& P, int i, const float* d, const float* atten, float* rgb) {
  Path p; p.rayo = mk(0, 0, 0); p.raydir = ld3(d + 3 * i); p.atten = ld3(atten + 3 * i);
  Ctr c = {0, 0, 0, 0, 0, 0, 0, 0};
  kat_st3(rgb + 3 * i, shade_miss<false>(P, p, c));
}

// The camera ray of sample s of pixel (x, y) of the view in P, both ways, each on a generator seeded with sample_seed: camera_ray, and the persistent
// kernel's split -- camera_prepare, the point of rand_points_merged (kind 2), camera_finish.  Form f of element i at f * n + i.
__device__ __forceinline__ void kat_camera_lane(const RenderParams& P, int i, const int32_t* x, const int32_t* y, const int32_t* s, float* origin2,
                                                float* dir2, uint32_t* next2, int n) {
  Xorwow a; a.init(sample_seed(P, x[i], y[i], s[i]));
  Xorwow b = a;
  V3 oa, da, ob, db;
  camera_ray(P, x[i], y[i], a, oa, da);
  float nu, nv;
  camera_prepare(P, x[i], y[i], b, nu, nv);
  const V3 disk = rand_points_merged<false>(b, 2);
  camera_finish(P, nu, nv, disk, ob, db);
  const size_t ia = (size_t)i, ib = (size_t)n + (size_t)i;
  kat_st3(origin2 + 3 * ia, oa); kat_st3(dir2 + 3 * ia, da);
  kat_st3(origin2 + 3 * ib, ob); kat_st3(dir2 + 3 * ib, db);
  next2[2 * ia] = a.next(); next2[2 * ia + 1] = a.next();
  next2[2 * ib] = b.next(); next2[2 * ib + 1] = b.next();
}

// store_pixel of colour i into pixel (i, 0) of P.out (P.H = 1, P.accumulate = 0, P.scale the view's)
__device__ __forceinline__ void kat_store_lane(const RenderParams& P, int i, const float* color) { store_pixel(P, i, 0, ld3(color + 3 * i)); }

}  // namespace dr
