// The caller-ray queries on the host: dr_kat_hit, dr_trace_rays with its surface pass, dr_trace_radiance and dr_trace_all_hits (with its brute-force
// yardstick), each the product's per-ray body in a loop over the image of a tree.  Part of host_kernel.cpp.
extern "C" {
// dr_kat_hit on the host: the closest hit of n caller rays (o[3n], d[3n]) by the walks of device_core.hpp -- traversal 0 closest_hit_threaded, 1
// closest_hit_ordered, 2 closest_hit_wide<true> over the image of `tree` (1: the reference's leaf boxes; 2: the product's default, small triangles with
// their own bounds, built on first use); a scene without a wide tree takes the threaded walk for traversal 2, as the product does.  Results in
// dr_kat_hit's convention: t (-1: miss), the ORIGINAL object index (0 on a miss), visits (may be NULL): boxes tested.  Returns 0, or -1 with hk_last_error.
int hk_hit(void* hv, int traversal, int tree, long long n, const float* o, const float* d, float* t, int32_t* idx, int32_t* visits) {
  HkScene* h = (HkScene*)hv;
  if (!h || n < 0 || (n > 0 && (!o || !d || !t || !idx)) || traversal < 0 || traversal > 2 || (tree != 1 && tree != 2)) { hk_err = "bad argument"; return -1; }
  const DeviceImage* const im = h->image(tree);
  if (!im) return -1;
  const DeviceImage& img = *im;
  const RenderParams P = image_params(img);
  HostStack stack;
  with_closest<true>(P, traversal, stack.data(), [&](auto closest) {
    for (long long i = 0; i < n; i++) {
      Ctr c = {0, 0, 0, 0, 0, 0, 0, 0};
      const Hit hit = closest(ld3(o + 3 * i), ld3(d + 3 * i), c);
      t[i] = hit.t;
      idx[i] = hit.slot >= 0 ? img.slot_to_orig[(size_t)hit.slot] : 0;      // hit() returns index 0 on a miss (K:507)
      if (visits) visits[i] = (int32_t)c.V;
    }
  });
  return 0;
}
// dr_trace_rays on the host: the walks of device_trace.hpp (trace_threaded, trace_ordered, trace_wide through trace_ray) on n caller rays, traversal and
// tree as hk_hit's (a scene without a wide tree takes the threaded walk for traversal 2).  mode 0 (DR_TRACE_CLOSEST): t (-1: miss), idx -- the ORIGINAL
// object index, -1 on a miss: dr_trace_rays' `object` --, slot (may be NULL): the hit's slot for hk_ray_surface; mode 1 (DR_TRACE_ANY): occluded 1 / 0.
// tmax NULL: every ray 10000.  visits (may be NULL): boxes tested per ray (the counting build's V).  Returns 0, or -1 with hk_last_error.
int hk_trace(void* hv, int traversal, int tree, int mode, long long n, const float* o, const float* d, const float* tmax, float* t, int32_t* idx,
             int32_t* occluded, int32_t* slot, int32_t* visits) {
  HkScene* h = (HkScene*)hv;
  if (!h || n < 0 || traversal < 0 || traversal > 2 || (tree != 1 && tree != 2) || (mode != DR_TRACE_CLOSEST && mode != DR_TRACE_ANY) ||
      (n > 0 && (!o || !d || (mode == DR_TRACE_CLOSEST ? (!t || !idx) : !occluded)))) { hk_err = "bad argument"; return -1; }
  const DeviceImage* const im = h->image(tree);
  if (!im) return -1;
  const DeviceImage& img = *im;
  const RenderParams P = image_params(img);
  HostStack stack;
  const int walk = plan_trace(n > 0 ? n : 1, traversal, P.wide != nullptr, 1, QUERY_FORCE_PLAIN).traversal;
  // every ray through `trace`; store(i, hit) keeps what the mode returns
  auto rays = [&](auto trace, auto store) {
    for (long long i = 0; i < n; i++) {
      Ctr c = {0, 0, 0, 0, 0, 0, 0, 0};
      store(i, trace(ld3(o + 3 * i), ld3(d + 3 * i), tmax ? tmax[i] : 10000.0f, c));
      if (visits) visits[i] = (int32_t)c.V;
    }
  };
  if (mode == DR_TRACE_ANY)
    with_trace<true>(P, walk, stack.data(), [&](auto trace) { rays(trace, [&](long long i, const Hit& hit) { occluded[i] = hit.slot >= 0 ? 1 : 0; }); });
  else
    with_trace<false>(P, walk, stack.data(), [&](auto trace) {
      rays(trace, [&](long long i, const Hit& hit) {
        t[i] = hit.t;
        idx[i] = hit.slot >= 0 ? img.slot_to_orig[(size_t)hit.slot] : -1;
        if (slot) slot[i] = hit.slot;
      });
    });
  return 0;
}
// dr_trace_rays' surface pass on the host: device_aov.hpp ray_surface on n rays and their hits (t, slot: hk_trace's, of the same tree); the channels
// (null: not written) as dr_trace_rays writes them.  Returns 0, or -1 with hk_last_error.
int hk_ray_surface(void* hv, int tree, long long n, const float* o, const float* d, const float* t, const int32_t* slot, int32_t* material, float* distance,
                   float* normal, float* uv, float* albedo) {
  HkScene* h = (HkScene*)hv;
  if (!h || n < 0 || (tree != 1 && tree != 2) || (n > 0 && (!o || !d || !t || !slot))) { hk_err = "bad argument"; return -1; }
  const DeviceImage* const im = h->image(tree);
  if (!im) return -1;
  const RenderParams P = image_params(*im);
  for (long long i = 0; i < n; i++) {
    if (slot[i] >= (int32_t)im->prims.size()) { hk_err = "slot outside the scene"; return -1; }
    write_aov_channels(ray_surface(P, ld3(o + 3 * i), ld3(d + 3 * i), t[i], slot[i]), (size_t)i, material, distance, normal, uv, albedo);
  }
  return 0;
}
// dr_trace_radiance on the host: device_radiance.hpp radiance_ray on n caller rays over the walks of device_core.hpp, traversal and tree as hk_hit's
// (a scene without a wide tree takes the threaded walk for traversal 2).  seed / skip NULL as in dr_radiance_rays; radiance (3n) / bounces (n): NULL not
// written, one of them at least.  The refusals are dr_trace_radiance's.  Returns 0, or -1 with hk_last_error.
int hk_radiance(void* hv, int traversal, int tree, long long n, const float* o, const float* d, const uint64_t* seed, const int32_t* skip, int spp,
                int max_depth, float background, int backtex, uint64_t base_seed, float* radiance, int32_t* bounces) {
  HkScene* h = (HkScene*)hv;
  if (!h || traversal < 0 || traversal > 2 || (tree != 1 && tree != 2)) { hk_err = "bad argument"; return -1; }
  if (n < 0 || n >= (long long)1 << 31) { hk_err = "radiance: the ray count must be in [0, 2^31)"; return -1; }
  if (!o || !d) { hk_err = "radiance: null origin or dir"; return -1; }
  if (!radiance && !bounces) { hk_err = "radiance: no output"; return -1; }
  if (spp < 1 || max_depth < 1) { hk_err = "radiance: spp and max_depth must be >= 1"; return -1; }
  if (backtex >= (int)h->img.tex.size()) { hk_err = "backtex refers to a texture that is not loaded"; return -1; }
  if (skip) for (long long i = 0; i < n; i++) if (skip[i] < 0) { hk_err = "radiance: a skip is negative"; return -1; }
  const DeviceImage* const im = h->image(tree);
  if (!im) return -1;
  RenderParams P = image_params(*im);
  P.max_depth = max_depth; P.bgint = background; P.backtex = backtex;
  RadianceLaunch R;
  memset(&R, 0, sizeof(R));
  R.origin = o; R.dir = d; R.seed = seed; R.skip = skip; R.n = (unsigned)n; R.spp = spp; R.base_seed = base_seed; R.radiance = radiance; R.bounces = bounces;
  HostStack stack;
  const int walk = plan_radiance(n > 0 ? n : 1, traversal, P.wide != nullptr, 1, QUERY_FORCE_PLAIN).traversal;
  with_closest<false>(P, walk, stack.data(), [&](auto closest) { for (long long i = 0; i < n; i++) radiance_ray(P, R, (unsigned)i, closest); });
  return 0;
}
// dr_trace_all_hits on the host: the per-ray bodies of device_allhits.hpp (allhits_wide or allhits_threaded, allhits_store, allhits_surface) on n caller
// rays with list length max_hits and kind_mask.  walk 2: the 4-way records of the image of `tree` (1 / 2, as hk_hit's), 0: the threaded links; a scene
// without a wide tree takes the threaded walk for walk 2, as the product does.  zero_margin (a switch for tests/test_allhits_host.py): the wide node
// step runs with the ray's margins forced to zero -- fl(o * inv) on both sides --, which the reachability argument does not cover.  The channels as
// dr_trace_all_hits writes them (NULL: not written); visits (may be NULL): records visited per ray.  Returns 0, or -1 with hk_last_error.
int hk_allhits(void* hv, int walk, int tree, long long n, const float* o, const float* d, const float* tmax, int max_hits, int kind_mask, int zero_margin,
               int32_t* count, float* t, int32_t* object, int32_t* material, float* distance, float* normal, float* uv, float* albedo, int32_t* visits, int nthreads) {
  HkScene* h = (HkScene*)hv;
  if (!h || n < 0 || n >= (long long)1 << 31 || (walk != 0 && walk != 2) || (tree != 1 && tree != 2) || (n > 0 && (!o || !d)) || nthreads < 1 || max_hits < 0 ||
      max_hits > ALLHITS_MAX || kind_mask <= 0 || kind_mask > 3) { hk_err = "bad argument"; return -1; }
  if (max_hits == 0 && (t || object || material || distance || normal || uv || albedo)) { hk_err = "max_hits 0 returns the count only"; return -1; }
  const DeviceImage* const im = h->image(tree);
  if (!im) return -1;
  const DeviceImage& img = *im;
  const RenderParams P = image_params(img);
  const bool wide = plan_allhits(n > 0 ? n : 1, walk == 2 && P.wide != nullptr, 1, QUERY_FORCE_PLAIN).wide;
  const int K = max_hits;
  const bool surface = material || distance || normal || uv || albedo;
  std::vector<uint32_t> hit(surface ? 2 * (size_t)n * (size_t)K : 0);
  const AllHitsSurface S = {distance, material, normal, uv, albedo};
  host_rows(nthreads, nthreads, [&](int k) {
    HostStack stack;
    std::vector<unsigned> list((size_t)ALLHITS_LIST_WORDS * 64);
    for (long long i = k; i < n; i += nthreads) {
      const V3 ro = ld3(o + 3 * i), rd = ld3(d + 3 * i);
      const float tm = tmax ? tmax[i] : 10000.0f;
      Ctr c = {0, 0, 0, 0, 0, 0, 0, 0};
      int cnt = 0;
      if (wide && zero_margin) {
        const float cap = trace_cap(tm);
        if (cap > 0.0f) {
          const V3 inv = mk(1.0f / rd.x, 1.0f / rd.y, 1.0f / rd.z);
          WideRay wr = wide_ray(ro, rd, inv, P.wide_pmax, P.wide_mu.e, P.wide_mu.l, P.wide_mu.v);
          wr.on = wr.of = mk(ro.x * wr.inv.x, ro.y * wr.inv.y, ro.z * wr.inv.z);
          allhits_wide<true>(wide_rsrc(P), wr, ro, rd, inv, cap, kind_mask, K, cnt, list.data(), c, stack.data());
        }
      } else if (wide) cnt = allhits_ray<true, true>(P, ro, rd, tm, kind_mask, K, list.data(), c, stack.data());
      else cnt = allhits_ray<false, true>(P, ro, rd, tm, kind_mask, K, list.data(), c, stack.data());
      allhits_store((size_t)i, cnt, K, list.data(), img.slot_to_orig.data(), count, t, object, surface ? hit.data() : nullptr);
      if (surface) for (int e = 0; e < K; e++) allhits_surface(P, o, d, hit.data(), K, (size_t)i * (size_t)K + (size_t)e, S);
      if (visits) visits[i] = (int32_t)c.V;
    }
  });
  return 0;
}
// The answer of dr_trace_all_hits by its definition, with no walk: every leaf record of the pre-order array in storage order (a record's successor is
// known from the record before it: an inner node's hit link, a leaf's next-is-leaf bit), slab() on the record's box, prim_hit_kind on its primitive,
// 0 < t <= cap, the kind mask; the crossings sorted by (bits of t, slot).  count, t, object as hk_allhits'.  The yardstick of tests/test_allhits_host.py.
int hk_allhits_brute(void* hv, long long n, const float* o, const float* d, const float* tmax, int max_hits, int kind_mask, int32_t* count, float* t, int32_t* object,
                     int nthreads) {
  HkScene* h = (HkScene*)hv;
  if (!h || n < 0 || (n > 0 && (!o || !d)) || nthreads < 1 || max_hits < 0 || kind_mask <= 0 || kind_mask > 3) { hk_err = "bad argument"; return -1; }
  const DeviceImage& img = h->img;
  const std::vector<DevUnit>& w = img.walk;
  auto word = [&w](size_t unit, int k) { int32_t v; memcpy(&v, &w[unit].f[k], 4); return v; };
  std::vector<size_t> leaves;
  {
    size_t u = 0;
    bool leaf = false;      // (the root of a scene of two objects or more is an inner node)
    while (u + (leaf ? WALK_UNITS_LEAF : WALK_UNITS_INTERNAL) <= w.size()) {
      if (leaf) {
        leaves.push_back(u);
        const int info = word(u, 3);
        if ((info >> 29) & 1) break;
        leaf = (info >> 28) & 1; u += WALK_UNITS_LEAF;
      } else {
        const int link = word(u, 3);
        if (link < 0) break;
        leaf = link & 1; u += WALK_UNITS_INTERNAL;
      }
    }
  }
  if (leaves.size() != img.prims.size()) { hk_err = "the walk array's leaves do not match the primitives"; return -1; }
  const int K = max_hits;
  host_rows(nthreads, nthreads, [&](int k) {
    std::vector<unsigned long long> keys;
    for (long long i = k; i < n; i += nthreads) {
      const V3 ro = ld3(o + 3 * i), rd = ld3(d + 3 * i);
      const float tm = tmax ? tmax[i] : 10000.0f;
      const float cap = tm > 0.0f ? fminf(tm, 10000.0f) : 0.0f;
      keys.clear();
      if (cap > 0.0f) {
        const V3 inv = mk(1.0f / rd.x, 1.0f / rd.y, 1.0f / rd.z);
        for (const size_t u : leaves) {
          const float mn[3] = {w[u].f[0], w[u].f[1], w[u].f[2]}, mx[3] = {w[u + 1].f[0], w[u + 1].f[1], w[u + 1].f[2]};
          const int info = word(u, 3), kind = (info >> WALK_SLOT_BITS) & 3, slot = info & ((1 << WALK_SLOT_BITS) - 1);
          if (!((kind == WALK_KIND_TRIANGLE && (kind_mask & 1)) || (kind == WALK_KIND_SPHERE && (kind_mask & 2)))) continue;
          float dist;
          if (!slab(ro, inv, mn, mx, dist)) continue;
          const float th = prim_hit_kind(kind, mk(w[u + 1].f[3], w[u + 2].f[0], w[u + 2].f[1]), mk(w[u + 2].f[2], w[u + 2].f[3], w[u + 3].f[0]),
                                         mk(w[u + 3].f[1], w[u + 3].f[2], w[u + 3].f[3]), ro, rd);
          if (th > 0.0f && th <= cap) keys.push_back(hit_key(th, slot));
        }
        std::sort(keys.begin(), keys.end());
      }
      if (count) count[i] = (int32_t)keys.size();
      for (int e = 0; e < K; e++) {
        const bool have = (size_t)e < keys.size();
        if (t) t[i * K + e] = have ? __uint_as_float((uint32_t)(keys[(size_t)e] >> 32)) : -1.0f;
        if (object) object[i * K + e] = have ? img.slot_to_orig[(size_t)(uint32_t)keys[(size_t)e]] : -1;
      }
    }
  });
  return 0;
}
}  // extern "C"
