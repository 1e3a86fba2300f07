// The point queries on the host: dr_query_nearest over the image of a tree, its brute-force definition, nearest_prim pair by pair and the records both
// read.  Part of host_kernel.cpp.
extern "C" {
// dr_query_nearest on the host: the per-query bodies of device_nearest.hpp (nearest_query over nearest_wide or nearest_threaded, then nearest_finish)
// on n points p[3n] with radii rmax (NULL: unbounded).  walk 2: the 4-way records of the image of `tree` (1 / 2, as hk_hit's), 0: the threaded links; a
// scene without a wide tree takes the threaded walk for walk 2, as the product does.  The channels as dr_query_nearest writes them (NULL: not written);
// visits (may be NULL): records visited per query.  Returns 0, or -1 with hk_last_error.
int hk_nearest(void* hv, int walk, int tree, long long n, const float* p, const float* rmax, float* distance, float* d2, int32_t* object, int32_t* material,
               float* point, float* uv, int32_t* visits, int nthreads) {
  HkScene* h = (HkScene*)hv;
  if (!h || n < 0 || n >= (long long)1 << 31 || (walk != 0 && walk != 2) || (tree != 1 && tree != 2) || (n > 0 && !p) || nthreads < 1) { hk_err = "bad argument"; return -1; }
  const DeviceImage* const im = h->image(tree);
  if (!im) return -1;
  const DeviceImage& img = *im;
  const RenderParams P = image_params(img);
  std::vector<uint32_t> key(2 * (size_t)n + 2);
  NearestLaunch N;
  memset(&N, 0, sizeof(N));
  N.point = p; N.rmax = rmax; N.n = (unsigned)n; N.lmax = img.near_lmax; N.slot_to_orig = img.slot_to_orig.data(); N.key = key.data();
  N.distance = distance; N.d2 = d2; N.object = object; N.material = material; N.qpoint = point; N.uv = uv;
  const bool wide = plan_nearest(n > 0 ? n : 1, walk == 2 && P.wide != nullptr).wide;
  host_rows(nthreads, nthreads, [&](int k) {
    HostStack stack;
    for (long long i = k; i < n; i += nthreads) {
      Ctr c = {0, 0, 0, 0, 0, 0, 0, 0};
      if (wide) nearest_query<true, true>(P, N, (unsigned)i, c, stack.data());
      else nearest_query<false, true>(P, N, (unsigned)i, c, stack.data());
      if (material || point || uv) nearest_finish(P, N, (unsigned)i);
      if (visits) visits[i] = (int32_t)c.V;
    }
  });
  return 0;
}
// The answer of dr_query_nearest by its definition, with no tree: the minimum of (bits(d2), slot) of nearest_prim over every primitive record of the
// scene, d2 <= fl(rmax rmax).  Channels as hk_nearest's.  The baseline of tools/nearest_rate.py and the reference of tests/test_nearest_host.py.
int hk_nearest_brute(void* hv, long long n, const float* p, const float* rmax, float* distance, float* d2, int32_t* object, int32_t* material, float* point,
                     float* uv, int nthreads) {
  HkScene* h = (HkScene*)hv;
  if (!h || n < 0 || (n > 0 && !p) || nthreads < 1) { hk_err = "bad argument"; return -1; }
  const DeviceImage& img = h->img;
  const int np = (int)img.prims.size();
  host_rows(nthreads, nthreads, [&](int k) {
    for (long long i = k; i < n; i += nthreads) {
      const V3 q = mk(p[3 * i], p[3 * i + 1], p[3 * i + 2]);
      const float r = rmax ? rmax[i] : INFINITY;
      float best = r * r; int slot = -1;
      Nearest bn; bn.q = mk(0, 0, 0); bn.u = bn.v = 0.0f;
      if (r >= 0.0f && std::isfinite(q.x) && std::isfinite(q.y) && std::isfinite(q.z))
        for (int s = 0; s < np; s++) {
          const DevPrim& pr = img.prims[(size_t)s];
          if (pr.type != 0 && pr.type != 2) continue;
          const Nearest a = nearest_prim(pr.type == 0 ? WALK_KIND_SPHERE : WALK_KIND_TRIANGLE, mk(pr.v0[0], pr.v0[1], pr.v0[2]), mk(pr.e1x, pr.e1y, pr.e1z),
                                         mk(pr.e2x, pr.e2y, pr.e2z), q);
          if (!a.cand) continue;
          const uint32_t ka = __float_as_uint(a.d2), kb = __float_as_uint(best);
          if (ka < kb || (ka == kb && slot < 0)) { best = a.d2; slot = s; bn = a; }      // slots ascend: a tie keeps the lower one
        }
      const bool hit = slot >= 0;
      if (!hit) { bn.q = mk(0, 0, 0); bn.u = bn.v = 0.0f; }
      if (d2) d2[i] = hit ? best : 0.0f;
      if (distance) distance[i] = hit ? sqrtf(best) : -1.0f;
      if (object) object[i] = hit ? img.slot_to_orig[(size_t)slot] : -1;
      if (material) material[i] = hit ? img.shade[(size_t)slot].mat : -1;
      if (point) { point[3 * i] = bn.q.x; point[3 * i + 1] = bn.q.y; point[3 * i + 2] = bn.q.z; }
      if (uv) { uv[2 * i] = bn.u; uv[2 * i + 1] = bn.v; }
    }
  });
  return 0;
}
// nearest_prim (device_nearest.hpp) on n point / primitive pairs: kind[n] (WALK_KIND_*), a, b, c[3n] as the records store them -> d2[n] (+inf: never a
// candidate), q[3n], uv[2n]
void hk_nearest_prim(long long n, const int32_t* kind, const float* a, const float* b, const float* c, const float* p, float* d2, float* q, float* uv) {
  for (long long i = 0; i < n; i++) {
    const Nearest r = nearest_prim(kind[i], mk(a[3 * i], a[3 * i + 1], a[3 * i + 2]), mk(b[3 * i], b[3 * i + 1], b[3 * i + 2]), mk(c[3 * i], c[3 * i + 1], c[3 * i + 2]),
                                   mk(p[3 * i], p[3 * i + 1], p[3 * i + 2]));
    d2[i] = r.d2; q[3 * i] = r.q.x; q[3 * i + 1] = r.q.y; q[3 * i + 2] = r.q.z; uv[2 * i] = r.u; uv[2 * i + 1] = r.v;
  }
}
// the scene's primitive records in slot order (both trees share them): kind[n], a, b, c[3n], the original object index and the material; and the
// pruning slack's scene constant.  Returns the number of records (arrays NULL: only that).
long long hk_nearest_prims(void* hv, int32_t* kind, float* a, float* b, float* c, int32_t* orig, int32_t* material, float* lmax) {
  HkScene* h = (HkScene*)hv;
  if (!h) { hk_err = "bad argument"; return -1; }
  const DeviceImage& img = h->img;
  if (lmax) *lmax = img.near_lmax;
  if (kind)
    for (size_t s = 0; s < img.prims.size(); s++) {
      const DevPrim& pr = img.prims[s];
      kind[s] = pr.type == 0 ? WALK_KIND_SPHERE : (pr.type == 2 ? WALK_KIND_TRIANGLE : WALK_KIND_NONE);
      a[3 * s] = pr.v0[0]; a[3 * s + 1] = pr.v0[1]; a[3 * s + 2] = pr.v0[2];
      b[3 * s] = pr.e1x; b[3 * s + 1] = pr.e1y; b[3 * s + 2] = pr.e1z;
      c[3 * s] = pr.e2x; c[3 * s + 1] = pr.e2y; c[3 * s + 2] = pr.e2z;
      orig[s] = img.slot_to_orig[s]; material[s] = img.shade[s].mat;
    }
  return (long long)img.prims.size();
}
int hk_nearest_k() { return NEAREST_K; }
// the records of the walk hk_nearest takes: 4-way records (walk 2, scenes that have them), else the nodes and leaves of the threaded walk
long long hk_nearest_records(void* hv, int walk, int tree) {
  HkScene* h = (HkScene*)hv;
  if (!h) { hk_err = "bad argument"; return -1; }
  const DeviceImage* const im = h->image(tree);
  if (!im) return -1;
  const DeviceImage& img = *im;
  if (walk == 2 && !img.wide.empty()) return (long long)(img.wide.size() / WIDE_UNITS);
  return (long long)(2 * img.prims.size() - 1);
}
}  // extern "C"
