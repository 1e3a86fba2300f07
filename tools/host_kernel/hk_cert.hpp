// The camera rays' grazing certificate and entry table of one view (device_cert.hpp) as kernels_aux.hip builds them, each with the
// brute-force check of what it promises against the kernel's own camera rays; and the default tree's side arrays for the tests.  Part of host_kernel.cpp.
namespace {
// The sampling loop of hk_cert_check and hk_cert_levels.  n_samples times: a triangle of the ones entered with their own bounds (|e1| |e2| <= cv.e_own;
// every second pick, when there are any, from those that constrained(i) names), a random point X of its padded box (own bounds + 0.01), the pixel X
// projects to through the pinhole (+-1), a random sample seed, and the kernel's camera ray of that sample (camera_ray: camera_prepare, the lens disk,
// camera_finish).  A ray that enters the box (slab(), entry > -0.01, as K:484-488) is handed to on_ray(i, x, y, a), a = |d . (e1 x e2)|.
template <class C, class F>
void cert_sample_rays(const RenderParams& P, const CertView& cv, const std::vector<DevPrim>& prims, const C& constrained, long long n_samples, uint64_t seed,
                      const F& on_ray) {
  uint64_t st = seed * 0x9E3779B97F4A7C15ull + 1;
  auto rnd = [&st]() { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return (double)(st >> 11) * 0x1p-53; };
  std::vector<size_t> tri, low;
  for (size_t i = 0; i < prims.size(); i++) {
    const DevPrim& p = prims[i];
    const double n1 = std::sqrt((double)p.e1x * p.e1x + (double)p.e1y * p.e1y + (double)p.e1z * p.e1z), n2 = std::sqrt((double)p.e2x * p.e2x + (double)p.e2y * p.e2y + (double)p.e2z * p.e2z);
    if (p.type == 2 && n1 * n2 <= cv.e_own) { tri.push_back(i); if (constrained(i)) low.push_back(i); }
  }
  if (tri.empty()) return;
  for (long long s = 0; s < n_samples; s++) {
    const bool pick_low = !low.empty() && (s & 1);
    const size_t i = pick_low ? low[(size_t)(rnd() * (double)low.size()) % low.size()] : tri[(size_t)(rnd() * (double)tri.size()) % tri.size()];
    const DevPrim& p = prims[i];
    const double v0[3] = {p.v0[0], p.v0[1], p.v0[2]}, e1[3] = {p.e1x, p.e1y, p.e1z}, e2[3] = {p.e2x, p.e2y, p.e2z};
    float mn[3], mx[3];
    double X[3];
    for (int a = 0; a < 3; a++) {
      const double lo = std::min(v0[a], std::min(v0[a] + e1[a], v0[a] + e2[a])) - 0.01, hi = std::max(v0[a], std::max(v0[a] + e1[a], v0[a] + e2[a])) + 0.01;
      mn[a] = (float)lo; mx[a] = (float)hi;
      X[a] = lo + (hi - lo) * rnd();
    }
    double rel[3], z = 0;                      // the pixel X projects to through the pinhole
    for (int a = 0; a < 3; a++) { rel[a] = X[a] - cv.from[a]; z += rel[a] * cv.w[a]; }
    if (!(z > 0)) continue;
    double pl[3];
    for (int a = 0; a < 3; a++) pl[a] = cv.from[a] + rel[a] * (cv.D / z) - cv.llc[a];
    const double nu = cv.du[0] * pl[0] + cv.du[1] * pl[1] + cv.du[2] * pl[2], nv = cv.dv[0] * pl[0] + cv.dv[1] * pl[1] + cv.dv[2] * pl[2];
    const double fx = std::floor(nu * cv.den_w) + (double)((int)(rnd() * 3.0) - 1), fy = std::floor(nv * cv.den_h) + (double)((int)(rnd() * 3.0) - 1);
    if (!(fx >= 0 && fy >= 0 && fx < cv.nx && fy < cv.ny)) continue;
    const int x = (int)fx, y = (int)fy;
    Xorwow rng;
    rng.init(sample_seed(P, x, y, 0, (int)(rnd() * 1000.0)));
    V3 o, d;
    camera_ray(P, x, y, rng, o, d);
    const V3 inv = mk(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
    float dist = 0;
    if (!slab(o, inv, mn, mx, dist) || !(dist > -0.01f)) continue;
    const double dd[3] = {d.x, d.y, d.z};
    const double nx = e1[1] * e2[2] - e1[2] * e2[1], ny = e1[2] * e2[0] - e1[0] * e2[2], nz = e1[0] * e2[1] - e1[1] * e2[0];
    on_ray(i, x, y, std::fabs(dd[0] * nx + dd[1] * ny + dd[2] * nz));
  }
}
}  // namespace

extern "C" {
// The camera rays' grazing certificate (device_cert.hpp cert_leaf) of the scene's triangles for one view, as kernels_aux.hip
// cert_mask_kernel builds it, and a check of what it promises against the kernel's own camera rays (cert_sample_rays, half the picks from the flagged
// triangles): a ray that enters a triangle's padded box must have |d . (e1 x e2)| >= a_star if the triangle is certified, and lie in a flagged tile
// if it is not.  e_own: triangles with |e1| |e2| above it are skipped (as never entered with their own bounds).
// out[0..7]: rays through certified boxes, of them below a_star (must be 0), rays through flagged boxes, of them in unflagged tiles (must be 0),
// flagged tiles, tiles, triangles flagged, "every tile" set.  Returns 0, or -1 with hk_last_error.
int hk_cert_check(void* hv, const float* settings13, int W, int H, double a_star, float e_own, long long n_samples, uint64_t seed, long long* out, uint32_t* mask_out) {
  HkScene* h = (HkScene*)hv;
  if (!h || !settings13 || !out) { hk_err = "bad argument"; return -1; }
  RenderParams P;
  if (const char* why = host_view(settings13, W, H, 0.0f, 1, 1, 0, P)) { hk_err = why; return -1; }
  CertView cv;
  if (!fill_cert_view(P, a_star, e_own, cv)) { hk_err = "the view gives no certificate"; return -1; }
  const std::vector<DevPrim>& prims = h->img.prims;
  const int tiles = P.ncols * P.gy, nwords = (tiles + 31) / 32;
  std::vector<uint32_t> mask((size_t)nwords + 2, 0u);
  std::vector<int> kind(prims.size(), 0);
  for (size_t i = 0; i < prims.size(); i++) {
    const DevPrim& p = prims[i];
    if (p.type != 2) continue;
    const float e1[3] = {p.e1x, p.e1y, p.e1z}, e2[3] = {p.e2x, p.e2y, p.e2z};
    int rect[4] = {0, -1, 0, -1};
    const int k = cert_leaf(cv, p.v0, e1, e2, rect);
    kind[i] = k;
    if (k == 2) mask[(size_t)nwords] = 1u;
    if (k == 1)
      for (int col = rect[0]; col <= rect[1]; col++)
        for (int r = rect[2]; r <= rect[3]; r++) { const int b = col * cv.gy + r; mask[(size_t)(b >> 5)] |= 1u << (b & 31); }
  }
  auto flagged_tile = [&](int b) { return mask[(size_t)nwords] || ((mask[(size_t)(b >> 5)] >> (b & 31)) & 1u); };
  long long flagged = 0, flagged_prims = 0;
  for (int b = 0; b < tiles; b++) flagged += flagged_tile(b) ? 1 : 0;
  for (int k : kind) flagged_prims += k != 0;
  if (mask_out) memcpy(mask_out, mask.data(), (size_t)(nwords + 2) * sizeof(uint32_t));
  for (int k = 0; k < 8; k++) out[k] = 0;
  out[4] = flagged; out[5] = tiles; out[6] = flagged_prims; out[7] = mask[(size_t)nwords];
  cert_sample_rays(P, cv, prims, [&](size_t i) { return kind[i] != 0; }, n_samples, seed, [&](size_t i, int x, int y, double a) {
    if (kind[i] == 0) {
      out[0]++;
      if (!(a >= a_star)) out[1]++;
    } else {
      out[2]++;
      if (!flagged_tile((x >> 3) * cv.gy + (y >> 3))) out[3]++;
    }
  });
  return 0;
}
// The graded certificate of one view (option cert_levels): the grades of its tiles as kernels_aux.hip builds them -- the same cert_leaf
// against the ladder of cert_factor (params_host.hpp cert_ladder; graded = 0: the single step) -- and hk_cert_check's sampling check per step (half the
// picks from the triangles that constrain a tile): a camera ray that enters the padded box of a triangle of grade g must have |d . (e1 x e2)| >= the
// ladder's step g - 1 (g >= 1), and lie in a tile whose grade is <= g (g < n_levels).  out[0..3]: rays through boxes of grade >= 1, of them below their step (must be 0), rays through boxes of grade
// < n_levels, of them in tiles of a higher grade (must be 0); out[4] n_levels, out[5] tiles, out[6] "every tile", out[7] base; out[8 + g] tiles of
// grade g, out[16 + g] rays through boxes of grade g (g = 0 .. 7).  plane_out (may be NULL): the grades, a byte per tile.  Returns 0, or -1.
int hk_cert_levels(void* hv, const float* settings13, int W, int H, int cert_factor, int graded, float e_own, long long n_samples, uint64_t seed, long long* out,
                   uint8_t* plane_out) {
  HkScene* h = (HkScene*)hv;
  if (!h || !settings13 || !out || cert_factor < 1) { hk_err = "bad argument"; return -1; }
  RenderParams P;
  if (const char* why = host_view(settings13, W, H, 0.0f, 1, 1, 0, P)) { hk_err = why; return -1; }
  CertView cv;
  if (!fill_cert_view(P, 1e-4 * (double)cert_factor, e_own, cv)) { hk_err = "the view gives no certificate"; return -1; }
  cert_ladder(cert_factor, graded != 0, cv);
  const std::vector<DevPrim>& prims = h->img.prims;
  const int tiles = P.ncols * P.gy, nl = cv.n_levels;
  std::vector<uint8_t> plane((size_t)tiles, (uint8_t)nl);
  std::vector<int> grade(prims.size(), nl);
  bool every = false;
  for (size_t i = 0; i < prims.size(); i++) {
    const DevPrim& p = prims[i];
    if (p.type != 2) continue;
    const float e1[3] = {p.e1x, p.e1y, p.e1z}, e2[3] = {p.e2x, p.e2y, p.e2z};
    int rect[4] = {0, -1, 0, -1};
    int g = nl;
    const int k = cert_leaf(cv, p.v0, e1, e2, rect, &g);
    if (k == 2) { every = true; g = 0; }
    grade[i] = k == 0 ? nl : g;
    if (k == 1)
      for (int col = rect[0]; col <= rect[1]; col++)
        for (int r = rect[2]; r <= rect[3]; r++) { uint8_t& b = plane[(size_t)col * cv.gy + r]; if (g < b) b = (uint8_t)g; }
  }
  if (every) std::fill(plane.begin(), plane.end(), (uint8_t)0);
  if (plane_out) memcpy(plane_out, plane.data(), plane.size());
  for (int k = 0; k < 24; k++) out[k] = 0;
  out[4] = nl; out[5] = tiles; out[6] = every; out[7] = cv.base;
  for (uint8_t b : plane) out[8 + b]++;
  cert_sample_rays(P, cv, prims, [&](size_t i) { return grade[i] < nl; }, n_samples, seed, [&](size_t i, int x, int y, double a) {
    const int g = grade[i];
    out[16 + g]++;
    if (g >= 1) {
      out[0]++;
      if (!(a >= cv.level_a[g - 1])) out[1]++;
    }
    if (g < nl) {
      out[2]++;
      if (plane[(size_t)(x >> 3) * cv.gy + (size_t)(y >> 3)] > g) out[3]++;
    }
  });
  return 0;
}
// The camera rays' entry table of one view (option camera_entry) over the product's default tree, as kernels_aux.hip builds it -- the same
// entry_leaf over the leaves in depth-first order, the same entry_tile per tile -- for the block columns bx % col_mod == col_rem.  codes_out (may be NULL):
// the entry codes, a word per tile (local column * tile rows + row).  mutant: 0, or one of device_cert.hpp's ENTRY_MUTANTs (a wrong rule on purpose).
// out[0] tiles, out[1] tiles without a leaf (ENTRY_NONE), out[2] tiles at the root, out[3] tiles at a leaf record, out[4] "every tile at the root",
// out[5] leaves, out[8 + d] tiles whose entry lies d records below the root (d = 0 .. 17; ENTRY_NONE not counted).  Returns 0, -1 with hk_last_error,
// or 1 when the view gives no table (fill_cert_view: a degenerate camera, a lens too wide for the focus plane) or the scene has no wide tree.
int hk_camera_entry(void* hv, const float* settings13, int W, int H, int col_mod, int col_rem, int mutant, int32_t* codes_out, long long* out) {
  HkScene* h = (HkScene*)hv;
  if (!h || !settings13 || !out || col_mod < 1 || col_rem < 0 || col_rem >= col_mod) { hk_err = "bad argument"; return -1; }
  const DeviceImage* const im = h->image(2);
  if (!im) return -1;
  const DeviceImage& img = *im;
  RenderParams P;
  if (const char* why = host_view(settings13, W, H, 0.0f, 1, col_mod, col_rem, P)) { hk_err = why; return -1; }
  CertView cv;
  // (the table asks nothing of the certificate's a_star or of the scene's own-bounds E: any valid pair)
  if (img.wide.empty() || !fill_cert_view(P, 40e-4, img.wide_mu.e > 0.0f ? img.wide_mu.e : 1.0f, cv)) return 1;
  const int tiles = P.ncols * P.gy;
  std::vector<uint32_t> mm(2 * (size_t)tiles + 1, 0xffffffffu);
  entry_mutant = mutant;
  for (size_t rank = 0; rank < img.wide_leaf_rec.size(); rank++) {
    const DevUnit* rec = &img.wide[(size_t)img.wide_leaf_rec[rank] * WIDE_UNITS];
    entry_leaf(cv, rec[0].f, rec[1].f, (uint32_t)rank, mm.data(), tiles);
  }
  for (int k = 0; k < 32; k++) out[k] = 0;
  out[0] = tiles; out[4] = mm[2 * (size_t)tiles] == 0u; out[5] = (long long)img.wide_leaf_rec.size();
  for (int t = 0; t < tiles; t++) {
    const int code = entry_tile(img.wide.data(), img.wide_range.data(), mm[2 * (size_t)t], mm[2 * (size_t)t + 1], mm[2 * (size_t)tiles] == 0u);
    if (codes_out) codes_out[t] = code;
    if (code == ENTRY_NONE) { out[1]++; continue; }
    if (code == 0) out[2]++;
    if (code & 1) out[3]++;
    // its depth: down from the root along the records whose ranges hold the entry's
    const uint32_t lo = img.wide_range[2 * (size_t)(code >> 1)], hi = img.wide_range[2 * (size_t)(code >> 1) + 1];
    uint32_t cur = 0u;
    int d = 0;
    while (cur != (uint32_t)(code >> 1) && d < 17) {
      const uint32_t* w = reinterpret_cast<const uint32_t*>(&img.wide[(size_t)cur * WIDE_UNITS]);
      uint32_t next = cur;
      for (uint32_t k = 0; k < 4; k++) {
        const uint32_t ch = wide_node_first_child(w) + k;
        if (((wide_node_valid(w) >> k) & 1u) && img.wide_range[2 * (size_t)ch] <= lo && hi <= img.wide_range[2 * (size_t)ch + 1]) next = ch;
      }
      if (next == cur) break;
      cur = next; d++;
    }
    out[8 + d]++;
  }
  entry_mutant = 0;
  return 0;
}
// What the table promises, by brute force: for every pixel of the stripe and `frames` frames (seeds seed + stride f) the kernel's own camera rays (camera_ray
// with the real sample seeds, settings13's samples per pixel) against EVERY leaf of the default tree -- a leaf whose record's box the ray enters (slab(), the
// reference's test) must lie under the entry of the ray's tile (codes: hk_camera_entry's).  out[0] rays, out[1] (ray, leaf) pairs entered, out[2] of them
// not under the tile's entry (must be 0), out[3] pairs entered in tiles whose entry is below the root.  Returns 0, or -1.
int hk_camera_entry_check(void* hv, const float* settings13, int W, int H, int col_mod, int col_rem, uint64_t seed, uint64_t stride, int frames, int nthreads,
                          const int32_t* codes, long long* out) {
  HkScene* h = (HkScene*)hv;
  if (!h || !settings13 || !codes || !out || !h->has_own || h->own.wide.empty() || frames < 1) { hk_err = "bad argument (hk_camera_entry first)"; return -1; }
  const DeviceImage& img = h->own;
  RenderParams P;
  if (const char* why = host_view(settings13, W, H, 0.0f, seed, col_mod, col_rem, P)) { hk_err = why; return -1; }
  if (nthreads < 1) nthreads = 1;
  std::vector<long long> part((size_t)nthreads * 4, 0);
  const size_t nleaves = img.wide_leaf_rec.size();
  host_rows(nthreads, P.ncols, [&](int col) {
    long long* acc = &part[(size_t)(col % nthreads) * 4];
    const int bx = P.stripe_rem + col * P.stripe_mod;
    for (int by = 0; by < P.gy; by++) {
      const int code = codes[(size_t)col * (size_t)P.gy + (size_t)by];
      const uint32_t lo = code == ENTRY_NONE ? 1u : img.wide_range[2 * (size_t)(code >> 1)], hi = code == ENTRY_NONE ? 0u : img.wide_range[2 * (size_t)(code >> 1) + 1];
      for (int lane = 0; lane < 64; lane++) {
        const int x = bx * 8 + (lane >> 3), y = by * 8 + (lane & 7);
        for (int f = 0; f < frames; f++)
          for (int s = 0; (float)s < P.spp_f; s++) {
            RenderParams Q = P;
            Q.seed = seed + stride * (uint64_t)f;
            Xorwow rng;
            rng.init(sample_seed(Q, x, y, s));
            V3 o, d;
            camera_ray(Q, x, y, rng, o, d);
            const V3 inv = mk(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
            acc[0]++;
            for (size_t rank = 0; rank < nleaves; rank++) {
              const DevUnit* rec = &img.wide[(size_t)img.wide_leaf_rec[rank] * WIDE_UNITS];
              float dist = 0;
              if (!slab(o, inv, rec[0].f, rec[1].f, dist)) continue;
              acc[1]++;
              if (!(lo <= rank && rank <= hi)) acc[2]++;
              if (code != 0) acc[3]++;
            }
          }
      }
    }
  });
  for (int k = 0; k < 4; k++) { out[k] = 0; for (int t = 0; t < nthreads; t++) out[k] += part[(size_t)t * 4 + k]; }
  return 0;
}
// the default tree's side arrays and leaf boxes, for the tests: leaves, then per rank the record and its box (mn, mx: 6 floats); range2 (may be NULL): two words per record
long long hk_wide_leaves(void* hv, uint32_t* leaf_rec, float* boxes, uint32_t* range2, long long room_leaves, long long room_records) {
  HkScene* h = (HkScene*)hv;
  if (!h) { hk_err = "bad argument"; return -1; }
  const DeviceImage* const im = h->image(2);
  if (!im) return -1;
  const DeviceImage& img = *im;
  const long long n =(long long)img.wide_leaf_rec.size(), nrec = (long long)(img.wide.size() / WIDE_UNITS);
  for (long long r = 0; r < n && r < room_leaves; r++) {
    if (leaf_rec) leaf_rec[r] = img.wide_leaf_rec[(size_t)r];
    if (boxes) { const DevUnit* rec = &img.wide[(size_t)img.wide_leaf_rec[(size_t)r] * WIDE_UNITS]; memcpy(boxes + 6 * r, rec[0].f, 12); memcpy(boxes + 6 * r + 3, rec[1].f, 12); }
  }
  if (range2) memcpy(range2, img.wide_range.data(), (size_t)(nrec < room_records ? nrec : room_records) * 8);
  return n;
}
// the scene's WideMu (e, l, v) as the product computes it (wide_tree = 2), for the certificate's own-bounds test (CertView e_own)
int hk_wide_mu(void* hv, float* out3) {
  HkScene* h = (HkScene*)hv;
  if (!h || !out3) { hk_err = "bad argument"; return -1; }
  DeviceImage img;
  if (linearise(h->scene->host, img, 2) != DR_OK) { hk_err = "scene could not be linearised"; return -1; }
  out3[0] = img.wide_mu.e; out3[1] = img.wide_mu.l; out3[2] = img.wide_mu.v;
  return img.wide_own_bounds;
}
}  // extern "C"
