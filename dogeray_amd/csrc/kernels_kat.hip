// The known-answer kernels behind dr_kat_*: single device functions on caller data, one element per lane.  The intersection, optics and walk
// hooks call the product's functions directly; the bodies of the shading step's (dr_kat_sample .. dr_kat_store) are in device_kat_shade.hpp.
#include <hip/hip_runtime.h>

#include <utility>

#include "device_kat_shade.hpp"
#include "device_wide.hpp"
#include "kernels.hpp"
#include "../../include/dogeray_amd.h"

namespace dr {

__global__ void kat_rng_kernel(uint64_t seed, int n, double* out) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    Xorwow r; r.init(seed);
    for (int i = 0; i < n; i++) out[i] = r.uniform_double();
  }
}
__global__ void kat_aabb_kernel(int n, const float* o, const float* d, const float* mn, const float* mx, int32_t* hit, float* dist) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  V3 dd = ld3(d + 3 * i);
  V3 inv = mk(1.0f / dd.x, 1.0f / dd.y, 1.0f / dd.z);
  float t;
  bool h = slab(ld3(o + 3 * i), inv, mn + 3 * i, mx + 3 * i, t);
  hit[i] = h; dist[i] = h ? t : 0;
}
__global__ void kat_node_planes_kernel(int n, const uint32_t* w, const float* a, const float* b, float* t_mix, float* t_cvt) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const PlanePairs p = plane_pairs(w[i]);
  const float a24 = a[i] * 0x1p24f;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    t_mix[4 * i + k] = plane_t(p, k, a24, b[i]);                                                         // the kernel's instruction (v_fma_mix_f32 on the f16 denormal)
    t_cvt[4 * i + k] = __builtin_fmaf((float)((w[i] >> (8 * k)) & 255u), a[i], b[i]);                    // conversion + fma
  }
}
__global__ void kat_tri_kernel(int n, const float* o, const float* d, const float* v0, const float* v1, const float* v2, float* t) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  V3 a = ld3(v0 + 3 * i);
  t[i] = tri_hit(ld3(o + 3 * i), ld3(d + 3 * i), a, ld3(v1 + 3 * i) - a, ld3(v2 + 3 * i) - a);
}
__global__ void kat_sphere_kernel(int n, const float* o, const float* d, const float* c, const float* r, float* t) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  t[i] = sphere_hit(ld3(c + 3 * i), r[i], ld3(o + 3 * i), ld3(d + 3 * i));
}
__global__ void kat_optics_kernel(int n, const float* v, const float* nrm, const float* eta, float* refl, float* refr, float* sch) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  V3 a = ld3(v + 3 * i), b = ld3(nrm + 3 * i);
  V3 r1 = reflect(a, b), r2 = refract(a, b, eta[i]);
  refl[3 * i] = r1.x; refl[3 * i + 1] = r1.y; refl[3 * i + 2] = r1.z;
  refr[3 * i] = r2.x; refr[3 * i + 1] = r2.y; refr[3 * i + 2] = r2.z;
  sch[i] = reflectance(a.x, eta[i]);
}
__global__ void kat_normal_kernel(RenderParams P, int n, const int32_t* slot, const float* o, const float* d, const float* t, float* nrm, float* texco) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4* pp = reinterpret_cast<const float4*>(P.prims + slot[i]);
  const float4* sp = reinterpret_cast<const float4*>(P.shade + slot[i]);
  const V3 ro = ld3(o + 3 * i), rd = ld3(d + 3 * i);
  const V3 hitpoint = ro + splat(t[i]) * rd;                           // K:806
  V3 tc;
  const V3 N = surface_normal(pp[0], pp[1], pp[2], sp[0], sp[1], sp[2], sp[3], sp[4], sp[6], ro, rd, hitpoint, tc);
  nrm[3 * i] = N.x; nrm[3 * i + 1] = N.y; nrm[3 * i + 2] = N.z;
  texco[3 * i] = tc.x; texco[3 * i + 1] = tc.y; texco[3 * i + 2] = tc.z;
}
template <int MODE>
__global__ __launch_bounds__(256) void kat_hit_kernel(RenderParams P, int n, const float* o, const float* d, float* t, int32_t* slot, int32_t* visits) {
  __shared__ int lds_stack[MODE == DR_TRAVERSAL_ORDERED ? ORDERED_STACK * 256 : (MODE == DR_TRAVERSAL_WIDE ? WIDE_STACK * 256 : 1)];
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Ctr c = {0, 0, 0, 0, 0, 0, 0, 0};
  Hit h;
  if (MODE == DR_TRAVERSAL_ORDERED) {
    int* stack = lds_stack + (threadIdx.x >> 6) * (ORDERED_STACK * 64) + (threadIdx.x & 63);
    h = closest_hit_ordered<true>(P.pairs, P.prims, ld3(o + 3 * i), ld3(d + 3 * i), c, stack);
  } else if (MODE == DR_TRAVERSAL_WIDE) {
    int* stack = lds_stack + (threadIdx.x >> 6) * (WIDE_STACK * 64) + (threadIdx.x & 63);
    h = closest_hit_wide<true>(wide_rsrc(P), P.wide_pmax, P.wide_mu.e, P.wide_mu.l, P.wide_mu.v, ld3(o + 3 * i), ld3(d + 3 * i), c, stack);
  } else {
    h = closest_hit_threaded<true>(walk_rsrc(P), ld3(o + 3 * i), ld3(d + 3 * i), c);
  }
  t[i] = h.t; slot[i] = h.slot;
  if (visits) visits[i] = (int32_t)c.V;
}

// ---- the shading step
__global__ __launch_bounds__(256) void kat_sample_kernel(int n, const uint64_t* seed, const int32_t* warm, const int32_t* kind, float* p_plain,
                                                         uint32_t* n_plain, float* p_merged, uint32_t* n_merged) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  kat_sample_lane(i, seed, warm, kind, p_plain, n_plain, p_merged, n_merged);
}
__global__ __launch_bounds__(256) void kat_outside_kernel(int n, const float* d2, int32_t* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  kat_outside_lane(i, d2, out);
}
__global__ __launch_bounds__(256) void kat_tex_kernel(RenderParams P, int n, const int32_t* tex, const float* u, const float* v, uint32_t* rgba) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  kat_tex_lane(P, i, tex, u, v, rgba);
}
__global__ __launch_bounds__(256) void kat_bounce_kernel(RenderParams P, int n, const int32_t* slot, const float* o, const float* d, const float* t,
                                                         const float* atten, const uint64_t* seed, const int32_t* warm, int32_t* alive2, float* o2,
                                                         float* d2, float* atten2, uint32_t* next2) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  kat_bounce_lane(P, i, slot, o, d, t, atten, seed, warm, alive2, o2, d2, atten2, next2, n);
}
__global__ __launch_bounds__(256) void kat_miss_kernel(RenderParams P, int n, const float* d, const float* atten, float* rgb) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  kat_miss_lane(P, i, d, atten, rgb);
}
__global__ __launch_bounds__(256) void kat_camera_kernel(RenderParams P, int n, const int32_t* x, const int32_t* y, const int32_t* s, float* origin2,
                                                         float* dir2, uint32_t* next2) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  kat_camera_lane(P, i, x, y, s, origin2, dir2, next2, n);
}
__global__ __launch_bounds__(256) void kat_store_kernel(RenderParams P, int n, const float* color) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  kat_store_lane(P, i, color);
}

// ---- the merged stores of device_shade.hpp (dr_kat_store_merged): lane i of the call is lane i % 64 of wave i / 64, four waves to a block as in the render
// kernel, n a multiple of 64 so that every wave that stores is whole (wave_sum needs its 64 lanes).  FORM 0: store_pixel, every storing lane on its own;
// 1: store_pixels_merged; 2: store_pixels_merged_lds.  A wave owns KAT_MERGE_ROWS rows of 64 LDS words, filled from lds_in before the store and written to
// lds_out after it: rows 1 .. 5 are the five slot rows, handed over as the render kernel hands its stash (the first word of slot `lane`); rows 0 and 6 are guards.
template <int FORM>
__global__ __launch_bounds__(256) void kat_store_merged_kernel(RenderParams P, int n, const int32_t* store_me, const int32_t* key, const int32_t* x,
                                                               const int32_t* y, const float* color, const int32_t* lds_in, int32_t* lds_out) {
  __shared__ int lds[4 * KAT_MERGE_ROWS * 64];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;                                    // whole waves: n is a multiple of 64
  const int lane = threadIdx.x & 63;
  int* const rows = lds + (threadIdx.x >> 6) * (KAT_MERGE_ROWS * 64);
  const size_t first = (size_t)(i >> 6) * (KAT_MERGE_ROWS * 64);
  for (int r = 0; r < KAT_MERGE_ROWS; r++) rows[r * 64 + lane] = lds_in[first + r * 64 + lane];
  asm volatile("" ::: "memory");                         // (a wave's LDS instructions run in order: the other lanes' words are there, as at the call site)
  __builtin_amdgcn_wave_barrier();
  const bool s = store_me[i] != 0;
  const V3 c = ld3(color + 3 * (size_t)i);
  if (FORM == 2) store_pixels_merged_lds(P, rows + 64 + lane, lane, s, key[i], x[i], y[i], c);
  else if (FORM == 1) store_pixels_merged(P, s, key[i], x[i], y[i], c);
  else if (s) store_pixel(P, x[i], y[i], c);
  asm volatile("" ::: "memory");
  __builtin_amdgcn_wave_barrier();
  for (int r = 0; r < KAT_MERGE_ROWS; r++) lds_out[first + r * 64 + lane] = rows[r * 64 + lane];
}

// ------------------------------------------------------------------ launchers
// every kernel but kat_rng_kernel (one wave: a single generator's sequence): blocks of 256 lanes, lane i the element i of n
template <class Kernel, class... Args>
static void kat_launch(Kernel kernel, hipStream_t stream, int n, Args&&... args) {
  hipLaunchKernelGGL(kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, std::forward<Args>(args)...);
}

void launch_kat_rng(hipStream_t stream, uint64_t seed, int n, double* out) { hipLaunchKernelGGL(kat_rng_kernel, dim3(1), dim3(64), 0, stream, seed, n, out); }
void launch_kat_aabb(hipStream_t stream, int n, const float* o, const float* d, const float* mn, const float* mx, int32_t* hit, float* dist) {
  kat_launch(kat_aabb_kernel, stream, n, n, o, d, mn, mx, hit, dist);
}
void launch_kat_node_planes(hipStream_t stream, int n, const uint32_t* w, const float* a, const float* b, float* t_mix, float* t_cvt) {
  kat_launch(kat_node_planes_kernel, stream, n, n, w, a, b, t_mix, t_cvt);
}
void launch_kat_tri(hipStream_t stream, int n, const float* o, const float* d, const float* v0, const float* v1, const float* v2, float* t) {
  kat_launch(kat_tri_kernel, stream, n, n, o, d, v0, v1, v2, t);
}
void launch_kat_sphere(hipStream_t stream, int n, const float* o, const float* d, const float* c, const float* r, float* t) {
  kat_launch(kat_sphere_kernel, stream, n, n, o, d, c, r, t);
}
void launch_kat_optics(hipStream_t stream, int n, const float* v, const float* nrm, const float* eta, float* refl, float* refr, float* sch) {
  kat_launch(kat_optics_kernel, stream, n, n, v, nrm, eta, refl, refr, sch);
}
void launch_kat_normal(hipStream_t stream, const RenderParams& P, int n, const int32_t* slot, const float* o, const float* d, const float* t, float* nrm, float* texco) {
  kat_launch(kat_normal_kernel, stream, n, P, n, slot, o, d, t, nrm, texco);
}
void launch_kat_hit(hipStream_t stream, const RenderParams& P, int traversal, int n, const float* o, const float* d, float* t, int32_t* slot, int32_t* visits) {
  if (traversal == DR_TRAVERSAL_WIDE) kat_launch(kat_hit_kernel<DR_TRAVERSAL_WIDE>, stream, n, P, n, o, d, t, slot, visits);
  else if (traversal == DR_TRAVERSAL_ORDERED) kat_launch(kat_hit_kernel<DR_TRAVERSAL_ORDERED>, stream, n, P, n, o, d, t, slot, visits);
  else kat_launch(kat_hit_kernel<DR_TRAVERSAL_THREADED>, stream, n, P, n, o, d, t, slot, visits);
}
void launch_kat_sample(hipStream_t stream, int n, const uint64_t* seed, const int32_t* warm, const int32_t* kind, float* p_plain, uint32_t* n_plain,
                       float* p_merged, uint32_t* n_merged) {
  kat_launch(kat_sample_kernel, stream, n, n, seed, warm, kind, p_plain, n_plain, p_merged, n_merged);
}
void launch_kat_outside(hipStream_t stream, int n, const float* d2, int32_t* out) { kat_launch(kat_outside_kernel, stream, n, n, d2, out); }
void launch_kat_tex(hipStream_t stream, const RenderParams& P, int n, const int32_t* tex, const float* u, const float* v, uint32_t* rgba) {
  kat_launch(kat_tex_kernel, stream, n, P, n, tex, u, v, rgba);
}
void launch_kat_bounce(hipStream_t stream, const RenderParams& P, int n, const int32_t* slot, const float* o, const float* d, const float* t,
                       const float* atten, const uint64_t* seed, const int32_t* warm, int32_t* alive2, float* o2, float* d2, float* atten2,
                       uint32_t* next2) {
  kat_launch(kat_bounce_kernel, stream, n, P, n, slot, o, d, t, atten, seed, warm, alive2, o2, d2, atten2, next2);
}
void launch_kat_miss(hipStream_t stream, const RenderParams& P, int n, const float* d, const float* atten, float* rgb) {
  kat_launch(kat_miss_kernel, stream, n, P, n, d, atten, rgb);
}
void launch_kat_camera(hipStream_t stream, const RenderParams& P, int n, const int32_t* x, const int32_t* y, const int32_t* s, float* origin2,
                       float* dir2, uint32_t* next2) {
  kat_launch(kat_camera_kernel, stream, n, P, n, x, y, s, origin2, dir2, next2);
}
void launch_kat_store(hipStream_t stream, const RenderParams& P, int n, const float* color) { kat_launch(kat_store_kernel, stream, n, P, n, color); }
void launch_kat_store_merged(hipStream_t stream, const RenderParams& P, int form, int n, const int32_t* store_me, const int32_t* key, const int32_t* x,
                             const int32_t* y, const float* color, const int32_t* lds_in, int32_t* lds_out) {
  if (form == 2) kat_launch(kat_store_merged_kernel<2>, stream, n, P, n, store_me, key, x, y, color, lds_in, lds_out);
  else if (form == 1) kat_launch(kat_store_merged_kernel<1>, stream, n, P, n, store_me, key, x, y, color, lds_in, lds_out);
  else kat_launch(kat_store_merged_kernel<0>, stream, n, P, n, store_me, key, x, y, color, lds_in, lds_out);
}

}  // namespace dr
