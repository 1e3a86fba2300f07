// One bounce and one path: the material's scatter, the background, the camera ray of a sample and the pixel's store.
#pragma once
#include "device_rng.hpp"
#include "device_surface.hpp"

namespace dr {

// raycolor K:787-982 is split at its natural seams so that the per-pixel kernel and the
// persistent kernel run the same arithmetic: shade_hit = the "hit > 0" branch of one bounce
// (K:807-950), shade_miss = the background branch (K:951-976).
struct Path { V3 rayo, raydir, atten; };

// shade_hit in three parts, so that the persistent kernel can run ONE rejection loop per phase for the lanes that scatter and the lanes that start a
// path (rand_points_merged): everything up to the draws (shade_prepare: K:807-848 and glossy's one uniform), the point in the unit sphere, and the
// scatter itself (shade_scatter: K:848-944).  A lane's draws keep the reference's order.
struct ShadeCtx { V3 hitpoint, N, ocolor; float add_x, rough, ir, r5; int mat; bool front; };
__device__ __forceinline__ bool shade_needs_sphere(const ShadeCtx& sc) { return sc.mat == 0 || sc.mat == 3 || sc.mat == 5; }

// What shade_prepare does with the unflipped normal N and the texture coordinate of a hit (s4 .. s6: the material's units of the shade record):
// returns false when the path ends at an emissive surface, with `emitted` as its radiance (K:941-944); true: sc is filled
template <bool COUNT>
__device__ __forceinline__ bool shade_material(const RenderParams& P, const Path& path, V3 hitpoint, V3 N, V3 texco, float4 s4, float4 s5, float4 s6, Xorwow& rng, Ctr& c,
                                               ShadeCtx& sc, V3& emitted) {
  const V3 raydir = path.raydir;
  bool front = dot(raydir, N) < 0;
  N = front ? N : N * splat(-1.0f);
  // ---- material inputs K:826-844
  V3 col = mk(s4.z, s4.w, s5.x);
  float add_x = s5.y, rough = s5.z;
  int mat = __float_as_int(s5.w), texnum = __float_as_int(s6.x), rtexnum = __float_as_int(s6.y);
  int flags = __float_as_int(s6.z);
  V3 ocolor = col;
  if (texnum >= 0) {
    ocolor = rgb_of(tex_fetch<COUNT>(P.tex, P.texels, texnum, texco.x, -texco.y + 1, c));
  } else if (flags & 2) {                     // checker K:776-784
    float u2 = __builtin_floorf(texco.x * 10), v2 = __builtin_floorf(texco.y * 10);
    float yes = u2 + v2;
    ocolor = (__builtin_fmodf(yes, 2.0f) == 0) ? splat(0.8f) : col;
  }
  if (rtexnum >= 0) {
    uint32_t px = tex_fetch<COUNT>(P.tex, P.texels, rtexnum, texco.x, -texco.y + 1, c);
    rough = byte_over_255(px & 255u) / 2;
  }
  if (!(mat == 0 || mat == 2 || mat == 3 || mat == 4 || mat == 5)) { emitted = ocolor * path.atten; return false; }      // emissive (and every unknown material) K:941-944
  // ---- the random draws come first (K:848-944), ONE copy of each loop for every lane that needs it: diffuse (0), metal (3) and glossy (5) all draw
  // a point in the unit sphere, glossy after its one uniform -- the order of draws of each lane is the reference's, but a wave runs the rejection
  // loop once instead of once per material branch (the five copies of that loop were most of the shade phase)
  sc.r5 = 0.0f;
  if (mat == 5) sc.r5 = randy(rng);
  sc.hitpoint = hitpoint; sc.N = N; sc.ocolor = ocolor; sc.add_x = add_x; sc.rough = rough; sc.ir = s5.z; sc.mat = mat; sc.front = front;      // ir: b[g].addional.y itself, not the textured roughness (K:917)
  return true;
}

// Returns false when the path ends at an emissive surface, with `emitted` as its radiance (K:941-944); true: sc is filled
template <bool COUNT>
__device__ __forceinline__ bool shade_prepare(const RenderParams& P, const Path& path, float t, int slot, Xorwow& rng, Ctr& c, ShadeCtx& sc, V3& emitted) {
  const V3 rayo = path.rayo, raydir = path.raydir;
  if (COUNT) c.S++;
  V3 hitpoint = rayo + splat(t) * raydir;
  const float4* pp = reinterpret_cast<const float4*>(P.prims + slot);
  const float4* sp = reinterpret_cast<const float4*>(P.shade + slot);
  float4 pA = pp[0], pB = pp[1], pC = pp[2];
  float4 s0 = sp[0], s1 = sp[1], s2 = sp[2], s3 = sp[3], s4 = sp[4], s5 = sp[5], s6 = sp[6];
  V3 texco;
  V3 N = surface_normal(pA, pB, pC, s0, s1, s2, s3, s4, s6, rayo, raydir, hitpoint, texco);
  return shade_material<COUNT>(P, path, hitpoint, N, texco, s4, s5, s6, rng, c, sc, emitted);
}

// shade_prepare for a hit of the lean persistent build (kernels_render.hip; device_prims.hpp HIT_UV_CARRIED, HIT_FETCH_LAZY), which may know more than
// the records and fetch less of them.  The same arithmetic on the same words: tests/test_hit_inputs_host.py, tests/test_gpu_hit_inputs.py.
//  CARRIED: (hit_u, hit_v) are the barycentrics of the tri_hit that accepted this hit, taken as given (otherwise tri_barycentrics forms them again);
//  LAZY: the hit's type is the shade record's copy (linearise.cpp writes the object's type into both records); the primitive record is loaded only in a
//        wave where a lane reads it -- without CARRIED every lane does; with it a sphere, a type that is never hit and a triangle whose face normal is the
//        -20 sentinel -- and t1, t2 (sp[3]) only where a lane has a texture, a roughness texture or the checker flag: texco has no other reader.  The lazy
//        loads are a second round trip, for the waves that take the branch.
// texco_out (the host's test hook, tools/host_kernel.cpp hk_hit_inputs): where texco goes besides
template <bool CARRIED, bool LAZY>
__device__ __forceinline__ bool shade_prepare_hit(const RenderParams& P, const Path& path, float t, int slot, float hit_u, float hit_v, Xorwow& rng, Ctr& c, ShadeCtx& sc,
                                                  V3& emitted, V3* texco_out = nullptr) {
  const V3 rayo = path.rayo, raydir = path.raydir;
  V3 hitpoint = rayo + splat(t) * raydir;
  const float4* pp = reinterpret_cast<const float4*>(P.prims + slot);
  const float4* sp = reinterpret_cast<const float4*>(P.shade + slot);
  float4 s0 = sp[0], s1 = sp[1], s2 = sp[2], s4 = sp[4], s5 = sp[5], s6 = sp[6];
  const int type = LAZY ? __float_as_int(s6.w) : __float_as_int(pp[2].y);
  // ---- the primitive record: the barycentrics (unless carried) and prim_normal
  float ux = hit_u, uy = hit_v;
  V3 Ng = mk(0, 0, 0);
  const bool reads_prim = !(CARRIED && LAZY) || type != 2 || s0.z == -20;
  if (DR_WAVE_ANY(reads_prim)) {
    if (reads_prim) {
      const float4 pA = pp[0], pB = pp[1], pC = pp[2];
      if (!CARRIED && type == 2) tri_barycentrics(pA, pB, pC, rayo, raydir, ux, uy);
      Ng = prim_normal(type, pA, pB, pC, hitpoint);
    }
  }
  // ---- the texture coordinate (0 for a sphere, K:703-773; 0 where no lane of the wave reads it)
  V3 texco = mk(0, 0, 0);
  const bool reads_texco = !LAZY || __float_as_int(s6.x) >= 0 || __float_as_int(s6.y) >= 0 || (__float_as_int(s6.z) & 2) != 0;
  if (DR_WAVE_ANY(reads_texco)) {
    if (type == 2 && reads_texco) texco = texco_of(ux, uy, sp[3], s4);
  }
  V3 N = shade_normal(type, Ng, ux, uy, s0, s1, s2, s6);
  if (texco_out) *texco_out = texco;
  return shade_material<false>(P, path, hitpoint, N, texco, s4, s5, s6, rng, c, sc, emitted);
}

// the scatter of one bounce (rs: the point in the unit sphere, for the materials that draw one): rayo / raydir / atten updated
__device__ __forceinline__ void shade_scatter(Path& path, const ShadeCtx& sc, V3 rs, Xorwow& rng) {
  V3& rayo = path.rayo; V3& raydir = path.raydir; V3& atten = path.atten;
  const V3 hitpoint = sc.hitpoint, N = sc.N, ocolor = sc.ocolor;
  const int mat = sc.mat;
  const bool like_metal = mat == 3 || (mat == 5 && sc.r5 > 0.8);      // float compared with the double 0.8
  if (mat == 0 || (mat == 5 && !like_metal)) {
    V3 target = hitpoint + N;
    if (mat == 5 || sc.add_x == 0) target = target + rs;              // glossy never normalises (K:899)
    else target = target + normalized(rs);
    atten = atten * ocolor;
    rayo = hitpoint;
    raydir = normalized(target - hitpoint);
  } else if (mat == 2) {
    atten = atten * ocolor;
    rayo = hitpoint;
    raydir = reflect(normalized(raydir), N);
  } else if (like_metal) {
    V3 refl = reflect(normalized(raydir), N);
    atten = atten * ocolor;
    rayo = hitpoint;
    raydir = refl + splat(sc.rough) * rs;
  } else {      // mat == 4
    float ir = sc.ir;
    float ratio = sc.front ? (1.0f / ir) : ir;
    float cos_theta = (float)fmin((double)dot(normalized(raydir) * splat(-1.0f), N), 1.0);
    float sin_theta = (float)__builtin_sqrt(1.0 - (double)(cos_theta * cos_theta));
    bool cannot = (ratio * sin_theta) > 1.0f;
    V3 out;
    if (cannot || reflectance(cos_theta, ratio) > randy(rng)) out = reflect(normalized(raydir), N);
    else out = refract(normalized(raydir), N, ratio);
    atten = atten * ocolor;
    rayo = hitpoint;
    raydir = out;
  }
}

// Returns true when the path continues (rayo/raydir/atten updated), false when it ends at an
// emissive surface with `emitted` as its radiance (K:941-944).
template <bool COUNT>
__device__ __forceinline__ bool shade_hit(const RenderParams& P, Path& path, float t, int slot, Xorwow& rng, Ctr& c, V3& emitted) {
  ShadeCtx sc;
  if (!shade_prepare<COUNT>(P, path, t, slot, rng, c, sc, emitted)) return false;
  V3 rs = mk(0, 0, 0);
  if (shade_needs_sphere(sc)) rs = rand_in_unit_sphere(rng);
  shade_scatter(path, sc, rs, rng);
  return true;
}

template <bool COUNT>
__device__ __forceinline__ V3 shade_miss(const RenderParams& P, const Path& path, Ctr& c) {
  const V3 raydir = path.raydir, atten = path.atten;
  V3 u = normalized(raydir);
  if (P.backtex > -1) {                       // K:953-966
    double ux = (double)u.x, uy = (double)u.y, uz = (double)u.z + 1.;
    float m = (float)(2. * __builtin_sqrt(ux * ux + uy * uy + uz * uz));
    V3 tt = u / splat(m) + splat(.5f);
    tt.y = -tt.y;
    V3 colr = rgb_of(tex_fetch<COUNT>(P.tex, P.texels, P.backtex, tt.x, -tt.y + 1, c));
    return atten * colr * splat(P.bgint);
  }
  float t2 = (float)(0.5 * ((double)u.y + 1.0));   // K:971-974
  float omt = (float)(1.0 - (double)t2);
  V3 sky = splat(omt) * mk(1.0f, 1.0f, 1.0f) + splat(t2) * mk(0.5f, 0.7f, 1.0f);
  return atten * sky * splat(P.bgint);
}

// One path: raycolor K:787-982.  `closest` is the traversal functor.
template <bool COUNT, class Closest>
__device__ __forceinline__ V3 trace_path(const RenderParams& P, const Closest& closest, V3 origin, V3 dir, Xorwow& rng, Ctr& c) {
  Path path; path.rayo = origin; path.raydir = dir; path.atten = splat(1.0f);
  for (int i = 0; i < P.max_depth; i++) {
    Hit h = closest(path.rayo, path.raydir, c);
    if (h.t > 0.0f) {
      V3 emitted;
      if (!shade_hit<COUNT>(P, path, h.t, h.slot, rng, c, emitted)) return emitted;
    } else {
      return shade_miss<COUNT>(P, path, c);
    }
  }
  return mk(0, 0, 0);
}

// Camera ray of one sample: K:1065-1073 (rng must be freshly seeded), in two parts around the point in the unit disk (the persistent kernel draws
// it in the phase's one rejection loop, rand_points_merged)
__device__ __forceinline__ void camera_prepare(const RenderParams& P, int x, int y, Xorwow& rng, float& nu, float& nv) {
  nu = (float)(((double)(float)x + rng.uniform_double()) / P.den_w);
  nv = (float)(((double)(float)y + rng.uniform_double()) / P.den_h);
}
__device__ __forceinline__ void camera_finish(const RenderParams& P, float nu, float nv, V3 disk, V3& origin, V3& dir) {
  V3 from = ld3(P.from), llc = ld3(P.llc), hor = ld3(P.hor), ver = ld3(P.ver), uu = ld3(P.uu), vu = ld3(P.vu);
  V3 rd = splat(P.lens_radius) * disk;
  V3 offset = uu * splat(rd.x) + vu * splat(rd.y);
  dir = llc + splat(nu) * hor + splat(nv) * ver - from - offset;
  origin = from + offset;
}
__device__ __forceinline__ void camera_ray(const RenderParams& P, int x, int y, Xorwow& rng, V3& origin, V3& dir) {
  float nu, nv;
  camera_prepare(P, x, y, rng, nu, nv);
  camera_finish(P, nu, nv, rand_in_unit_disk(rng), origin, dir);
}
__device__ __forceinline__ uint64_t sample_seed(const RenderParams& P, int x, int y, int s, int frame = 0) {   // K:1065 with clock() := frame seed
  return P.seed + (uint64_t)frame * P.batch_seed_stride + (uint64_t)s * 0x9E3779B97F4A7C15ull +
         (uint64_t)((uint32_t)x + (uint32_t)y * P.seed_stride);
}
// (frame_offset: launches that render every frame of their batch into a buffer of its own -- the grouped present pipeline -- pass frame * P.out_frame_stride)
__device__ __forceinline__ void store_pixel(const RenderParams& P, int x, int y, V3 color, size_t frame_offset = 0) {     // K:1081-1085
  int r = f2i(color.x * 255 * P.scale), g = f2i(color.y * 255 * P.scale), b = f2i(color.z * 255 * P.scale);
  int32_t* px = P.out + frame_offset + ((size_t)x * (size_t)P.H + (size_t)y) * 3;
  if (P.accumulate == 2) {        // frames of one batch may finish the same pixel concurrently; integer adds commute
    atomicAdd(px + 0, r); atomicAdd(px + 1, g); atomicAdd(px + 2, b);
  } else if (P.accumulate) { px[0] += r; px[1] += g; px[2] += b; }
  else { px[0] = r; px[1] = g; px[2] = b; }
}

#ifndef DR_HOST_BUILD
// STORES_MERGED (the macro serves the variant libraries of tools/exp_variant.sh): with option sample_order = 1 the lanes of a wave that end a path in one
// phase are mostly frames of the same pixel and would each add their three words to the same three addresses; store_pixels_merged adds one sum per pixel
// instead.  Integer addition is exact in any grouping: the same bytes.  Only for launches that add atomically with a frame-minor order (never one frame).
#ifndef DR_STORES_MERGED
#define DR_STORES_MERGED 2
#endif
constexpr int STORES_MERGED = DR_STORES_MERGED;      // 0 every lane adds on its own; 1 store_pixels_merged; 2 store_pixels_merged_lds (the wide builds)
// the sum of v over the wave (all 64 lanes active), as a scalar: an inclusive scan within each row of 16 (row_shr 1, 2, 4, 8; lanes shifted in read 0), then
// lane 15 of rows 0 and 2 into rows 1 and 3 (row_bcast15), lane 31 into rows 2 and 3 (row_bcast31): lane 63 holds the total
__device__ __forceinline__ int wave_sum(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, true);
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, true);
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, true);
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, true);
  v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, true);
  v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, true);
  return __builtin_amdgcn_readlane(v, 63);
}
// store_pixel's atomic adds (P.accumulate == 2) for the lanes with store_me, one set per pixel: called by the whole wave; key names the lane's pixel
// (two lanes with the same key have the same x, y).  A turn per distinct pixel among the storing lanes; its lowest lane adds the group's sums.
__device__ __forceinline__ void store_pixels_merged(const RenderParams& P, bool store_me, int key, int x, int y, V3 color) {
  const int r = f2i(color.x * 255 * P.scale), g = f2i(color.y * 255 * P.scale), b = f2i(color.z * 255 * P.scale);
  unsigned long long todo = __ballot(store_me);
  while (todo != 0ull) {
    const int lead = __builtin_ctzll(todo);
    const bool mine = store_me && key == __builtin_amdgcn_readlane(key, lead);
    const int sr = wave_sum(mine ? r : 0), sg = wave_sum(mine ? g : 0), sb = wave_sum(mine ? b : 0);
    if ((int)(threadIdx.x & 63) == lead) {
      int32_t* px = P.out + ((size_t)x * (size_t)P.H + (size_t)y) * 3;
      atomicAdd(px + 0, sr); atomicAdd(px + 1, sg); atomicAdd(px + 2, sb);
    }
    todo &= ~__ballot(mine);
  }
}
// The same through five LDS words per slot that the caller has free (word w of slot s at ws[w * 64 + s - lane], s = 0 .. 63, private to the wave): a pixel's slot is
// the low six bits of its key.  The storing lanes write their key to their slot and clear its three sums; the lanes that find their own key there -- all the
// lanes of one pixel: two pixels on one slot are rare, the loser's lanes add on their own -- add into the sums with LDS atomics and write their lane number;
// the lane that finds its own number adds the sums to the pixel.  A wave's LDS instructions run in order, and the compiler barriers keep it from forwarding
// a lane's own write to its read.  The cost does not depend on how many pixels end in the phase.
// (the three integers are formed where they are used, a channel at a time: held beside the colour they cost the lean build two spilled registers)
__device__ __forceinline__ void store_pixels_merged_lds(const RenderParams& P, int* ws, int lane, bool store_me, int key, int x, int y, V3 color) {
  if (!store_me) return;
  int* const slot = ws + ((key & 63) - lane);      // words: 0 key, 1 lane, 2 .. 4 sums (ws: the first word of slot `lane`, which the caller has at hand)
  slot[0] = key; slot[2 * 64] = 0; slot[3 * 64] = 0; slot[4 * 64] = 0;
  asm volatile("" ::: "memory");
  const bool ok = slot[0] == key;
  if (ok) {
    slot[1 * 64] = lane;
    atomicAdd(slot + 2 * 64, f2i(color.x * 255 * P.scale)); atomicAdd(slot + 3 * 64, f2i(color.y * 255 * P.scale)); atomicAdd(slot + 4 * 64, f2i(color.z * 255 * P.scale));
  }
  asm volatile("" ::: "memory");
  int r, g, b;
  if (ok) {
    if (slot[1 * 64] != lane) return;
    r = slot[2 * 64]; g = slot[3 * 64]; b = slot[4 * 64];
  } else { r = f2i(color.x * 255 * P.scale); g = f2i(color.y * 255 * P.scale); b = f2i(color.z * 255 * P.scale); }
  int32_t* px = P.out + ((size_t)x * (size_t)P.H + (size_t)y) * 3;
  atomicAdd(px + 0, r); atomicAdd(px + 1, g); atomicAdd(px + 2, b);
}
#endif

// Kernel K:998-1093 for one pixel (the camera basis comes precomputed in P).
template <bool COUNT, class Closest>
__device__ __forceinline__ void render_pixel(const RenderParams& P, const Closest& closest, int x, int y, Ctr& c, bool* camera_ray_next = nullptr /* set before every path: its first ray is a camera ray */) {
  V3 color = mk(0, 0, 0);
  for (int s = 0; (float)s < P.spp_f; ++s) {
    Xorwow rng;
    rng.init(sample_seed(P, x, y, s));
    if (COUNT) c.samples++;
    V3 origin, dir;
    camera_ray(P, x, y, rng, origin, dir);
    if (camera_ray_next) *camera_ray_next = true;
    color = color + trace_path<COUNT>(P, closest, origin, dir, rng, c);
  }
  store_pixel(P, x, y, color);
}

}  // namespace dr
