// The first-hit AOVs of a pixel averaged over the renderer's own camera rays (dr_render_aov_lens): the jittered rays that leave from a point on the
// lens, folded sample by sample.  include/dogeray_amd.h has the table of channels; DESIGN.md 4.22 the kernel.
#pragma once
#include "device_shade.hpp"
#include "device_aov.hpp"

namespace dr {

// ------------------------------------------------------------------ lens-averaged AOVs (dr_render_aov_lens)
// Pixel (x, y) over its N = nframes * spp samples, frame k = 0 .. nframes - 1 outer, sample s = 0 .. spp - 1 inner: sample (k, s) seeds a fresh Xorwow
// with sample_seed(P, x, y, s, k) -- P.seed the launch's frame_seed, P.batch_seed_stride its seed_stride, P.seed_stride the unstriped view's 8 * gx -- and
// camera_ray draws the ray a render launch of these seeds traces (K:1065-1073).  Its closest hit and ray_surface there are folded into the sums below:
// every sum a plain float + in sample order from 0, every quotient one division at the end (-ffp-contract=off), no random draw beyond camera_ray's, no
// counter.  The three pieces -- the ray of a sample, the fold of its hit, the quotients -- are what the GPU kernel calls one by one from its refilling
// walk loop; aov_lens_pixel is their plain nested loop (the host build, and the kernel's second loop shape).  A lane folds its own samples strictly in
// order either way: the same bits.
struct AovLensSum {
  int hits;            // h: samples that hit
  float depth;         // sum of t * focus over the hits
  float distance;      // sum of ray_surface's distance
  V3 normal, albedo;   // sums of the facing normal and of ocolor
  int cand, cnt;       // the Boyer-Moore vote over the samples' mat (-1: a miss)
};
struct AovLens {
  float coverage;      // h / N
  float depth;         // sum / h: the lens offset lies in the uu, vu plane, so t * focus is still the distance along the view axis; +inf when h = 0
  float distance;      // sum / h, +inf when h = 0
  int mat;             // the vote's candidate: the majority where one exists; -1 implies nothing else, != -1 implies h >= 1
  V3 normal;           // sum / h, not renormalised: shorter where the samples' normals disagree; 0 when h = 0
  V3 albedo;           // sum / N: premultiplied by coverage
};

__device__ __forceinline__ AovLensSum aov_lens_begin() {
  AovLensSum a;
  a.hits = 0; a.depth = 0; a.distance = 0;
  a.normal = mk(0, 0, 0); a.albedo = mk(0, 0, 0);
  a.cand = -1; a.cnt = 0;
  return a;
}

// The camera ray of sample s of frame k
__device__ __forceinline__ void aov_lens_ray(const RenderParams& P, int x, int y, int k, int s, V3& o, V3& d) {
  Xorwow rng;
  rng.init(sample_seed(P, x, y, s, k));
  camera_ray(P, x, y, rng, o, d);
}

// One sample: the closest hit (t, slot) of its ray (o, d) as a walk left it (a miss: t <= 0)
__device__ __forceinline__ void aov_lens_fold(const RenderParams& P, float focus, V3 o, V3 d, float t, int slot, AovLensSum& a) {
  const AovHit r = ray_surface(P, o, d, t, t > 0.0f ? slot : -1);
  int v = -1;
  if (r.t > 0.0f) {
    a.hits++;
    a.depth = a.depth + t * focus;
    a.distance = a.distance + r.distance;
    a.normal = a.normal + r.normal;
    a.albedo = a.albedo + r.albedo;
    v = r.mat;
  }
  if (a.cnt == 0) { a.cand = v; a.cnt = 1; }
  else if (v == a.cand) a.cnt++;
  else a.cnt--;
}

// The quotients over N >= 1 samples.  as_guides (trace_guides only): a pixel whose vote is a miss is a miss in every channel, and the albedo is the
// guide albedo a + (1 - coverage), a missed sample counting as albedo 1 so that demodulation leaves the sky's share alone.
__device__ __forceinline__ AovLens aov_lens_finish(const AovLensSum& a, int N, bool as_guides) {
  AovLens r;
  const float inf = __builtin_inff();
  const float h = (float)a.hits, n = (float)N;
  r.coverage = h / n;
  r.depth = inf; r.distance = inf; r.normal = mk(0, 0, 0);
  if (a.hits > 0) {
    r.depth = a.depth / h;
    r.distance = a.distance / h;
    r.normal = a.normal / splat(h);
  }
  r.albedo = a.albedo / splat(n);
  r.mat = a.cand;
  if (as_guides) {
    if (r.mat == -1) { r.coverage = 0; r.depth = inf; r.distance = inf; r.normal = mk(0, 0, 0); r.albedo = mk(0, 0, 0); }
    else r.albedo = r.albedo + splat(1.0f - r.coverage);
  }
  return r;
}

// The whole pixel by the nested loop; `closest` is the traversal functor of aov_first_hit
template <class Closest>
__device__ __forceinline__ AovLens aov_lens_pixel(const RenderParams& P, const Closest& closest, float focus, int x, int y, int nframes, int spp /* (int)settings13[10] */,
                                                  bool as_guides = false) {
  AovLensSum a = aov_lens_begin();
  Ctr c = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int k = 0; k < nframes; k++)
    for (int s = 0; s < spp; s++) {
      V3 o, d;
      aov_lens_ray(P, x, y, k, s, o, d);
      const Hit h = closest(o, d, c);
      aov_lens_fold(P, focus, o, d, h.t, h.slot, a);
    }
  return aov_lens_finish(a, nframes * spp, as_guides);
}

}  // namespace dr
