// Frames and first-hit buffers on the host: render_pixel and aov_first_hit (the product's per-pixel bodies) over the tiles of a view, one "lane" at a
// time, threads over 8-pixel block columns or rows.  hk_render is the measured cpu_baseline.same_source of bench.py.  Part of host_kernel.cpp.
namespace {
// The block columns first, first + step, ... of P's stripe.
// plane / ktab (null: none): the grades of the view's grazing certificate, a byte per tile, and the margin's factor per grade -- the camera ray of
// every path of a tile carries its tile's factor, as the lean build's do (kernels_render.hip; there for a pixel's first sample)
// eplane (null: none): the entry codes of the view's camera rays, a word per tile (hk_camera_entry) -- the camera ray of every path starts its walk there
template <bool COUNT>
void render_columns(const RenderParams& P, int traversal, int first, int step, Ctr& total, const uint8_t* plane, const float* ktab, const int32_t* eplane) {
  HostStack stack;
  Ctr c = {0, 0, 0, 0, 0, 0, 0, 0};
  auto pixels = [&](auto pixel) {                                   // pixel(tile, x, y) for every pixel of the columns, tile by tile
    for (int col = first; col < P.ncols; col += step) {
      const int bx = P.stripe_rem + col * P.stripe_mod;
      for (int by = 0; by < P.gy; by++)
        for (int lane = 0; lane < 64; lane++)                       // lane l of a tile is pixel (l >> 3, l & 7), as in the kernels
          pixel((size_t)col * (size_t)P.gy + (size_t)by, bx * 8 + (lane >> 3), by * 8 + (lane & 7));
    }
  };
  if (traversal == DR_TRAVERSAL_WIDE && P.wide) {                   // the wide walk, the camera ray with its tile's margin and entry
    const WalkRsrc wide = wide_rsrc(P);
    pixels([&](size_t tile, int x, int y) {
      bool camera = false;
      const float kt = plane ? ktab[plane[tile] & CERT_MAX_LEVELS] : 1.0f;
      const int entry = eplane ? eplane[tile] : 0;
      auto closest = [&](V3 o, V3 d, Ctr& cc) {
        const float k = camera ? kt : 1.0f;
        const int e = camera ? entry : 0;
        camera = false;
        return closest_hit_wide<COUNT>(wide, P.wide_pmax, P.wide_mu.e, P.wide_mu.l, P.wide_mu.v, o, d, cc, stack.data(), k, e);
      };
      render_pixel<COUNT>(P, closest, x, y, c, plane || eplane ? &camera : nullptr);
    });
  } else
    with_closest<COUNT>(P, traversal, stack.data(), [&](auto closest) { pixels([&](size_t, int x, int y) { render_pixel<COUNT>(P, closest, x, y, c); }); });
  total = c;
}
}  // namespace

extern "C" {
// One frame (dr_render_frame's arguments): int32[W * H * 3], pixel (x, y) at (x * H + y) * 3, unrendered margins 0; only the block
// columns bx % col_mod == col_rem are rendered (a bounded sample for the bench).  counters: rays, V, L, S, T, samples (6 words).
// level_plane (may be NULL): the grades of the view's graded certificate (hk_cert_levels' plane_out for cert_factor / graded, whole frame: col_mod 1) --
// the frame is then rendered as the device renders it: the wide walk over the product's default tree (wide_tree = 2), the camera rays with their
// tile's margin.  entry_plane (may be NULL): the entry codes of the view's camera rays for this very stripe (hk_camera_entry's codes_out): the camera rays
// start there, over the default tree as well.
int hk_render(void* hv, const float* settings13, int W, int H, float background, uint64_t frame_seed, int traversal, int nthreads, int col_mod, int col_rem,
              int32_t* out, uint64_t* counters, const uint8_t* level_plane, int cert_factor, int graded, const int32_t* entry_plane) {
  HkScene* h = (HkScene*)hv;
  if (!h || !settings13 || !out || col_mod < 1 || col_rem < 0 || col_rem >= col_mod) { hk_err = "bad argument"; return -1; }
  float ktab[CERT_MAX_LEVELS + 1];
  for (float& k : ktab) k = 1.0f;
  if (level_plane) {
    if (col_mod != 1 || cert_factor < 1 || traversal != DR_TRAVERSAL_WIDE) { hk_err = "a level plane needs the whole frame, its cert_factor and the wide walk"; return -1; }
  }
  const bool own = level_plane || entry_plane;
  if (own && traversal != DR_TRAVERSAL_WIDE) { hk_err = "an entry plane needs the wide walk"; return -1; }
  const DeviceImage* const im = h->image(own ? 2 : 1);
  if (!im) return -1;
  const DeviceImage& img = *im;
  if (level_plane) {
    CertView cv;
    cert_ladder(cert_factor, graded != 0, cv);
    for (int g = 1; g <= cv.n_levels; g++) ktab[g] = cert_factor_k(cv.level_a[g - 1]);
  }
  RenderParams P;
  if (const char* why = host_view(img, settings13, W, H, background, frame_seed, col_mod, col_rem, P)) { hk_err = why; return -1; }
  if (own && img.wide.empty()) { hk_err = "the scene has no wide tree"; return -1; }
  fill_image(img, P);
  P.out = out;
  P.accumulate = 0;
  memset(out, 0, (size_t)W * H * 3 * sizeof(int32_t));
  if (nthreads < 1) nthreads = 1;
  std::vector<Ctr> part((size_t)nthreads);
  host_rows(nthreads, nthreads, [&](int t) {
    if (counters) render_columns<true>(P, traversal, t, nthreads, part[(size_t)t], level_plane, ktab, entry_plane);
    else render_columns<false>(P, traversal, t, nthreads, part[(size_t)t], level_plane, ktab, entry_plane);
  });
  if (counters) {
    for (int k = 0; k < 6; k++) counters[k] = 0;
    for (const Ctr& c : part) { counters[0] += c.rays; counters[1] += c.V; counters[2] += c.L; counters[3] += c.S; counters[4] += c.T; counters[5] += c.samples; }
  }
  return 0;
}

// dr_render_aov on the host: device_aov.hpp aov_first_hit for every pixel of the window (x0, y0, w, h) of the pixel grid, with the given traversal;
// the channels (null: not written) in dr_render_aov's layout.  Returns 0, or -1 with hk_last_error.
int hk_aov(void* hv, const float* settings13, int W, int H, int x0, int y0, int w, int h, int traversal, int nthreads, float* t, float* distance,
           float* depth, int32_t* object, int32_t* material, float* normal, float* uv, float* albedo, float* dir) {
  HkScene* h_ = (HkScene*)hv;
  if (!h_ || !settings13) { hk_err = "bad argument"; return -1; }
  const DeviceImage& img = h_->img;
  RenderParams P;
  if (const char* why = host_view(img, settings13, W, H, 0.0f, 0, 1, 0, P)) { hk_err = why; return -1; }
  if (w <= 0 || h <= 0 || x0 < 0 || y0 < 0 || x0 > P.gx * 8 - w || y0 > P.gy * 8 - h) { hk_err = "window is empty or not inside the pixel grid"; return -1; }
  fill_image(img, P);
  const float focus = settings13[7];
  if (nthreads < 1) nthreads = 1;
  host_rows(nthreads, nthreads, [&](int k) {
    HostStack stack;
    with_closest<false>(P, traversal, stack.data(), [&](auto closest) {
      for (int wy = k; wy < h; wy += nthreads)
        for (int wx = 0; wx < w; wx++) {
          const AovHit a = aov_first_hit(P, closest, focus, x0 + wx, y0 + wy);
          const size_t i = (size_t)wy * (size_t)w + (size_t)wx;
          if (t) t[i] = a.t;
          if (depth) depth[i] = a.depth;
          if (object) object[i] = a.slot >= 0 ? img.slot_to_orig[(size_t)a.slot] : -1;
          if (dir) st3(dir + 3 * i, a.dir);
          write_aov_channels(a, i, material, distance, normal, uv, albedo);
        }
    });
  });
  return 0;
}

// dr_render_aov_lens on the host: device_aov_lens.hpp aov_lens_pixel -- the plain nested loop over the pixel's nframes * spp camera rays -- for every pixel
// of the window, with the given traversal; the channels (null: not written) in dr_render_aov_lens's layout.  as_guides: trace_guides' form (option
// guide_frames: frame_seed DR_GUIDE_SEED, seed_stride 1).  Returns 0, or -1 with hk_last_error.
int hk_aov_lens(void* hv, const float* settings13, int W, int H, int x0, int y0, int w, int h, uint64_t frame_seed, uint64_t seed_stride, int nframes,
                int as_guides, int traversal, int nthreads, float* coverage, float* depth, float* distance, int32_t* material, float* normal, float* albedo) {
  HkScene* h_ = (HkScene*)hv;
  if (!h_ || !settings13) { hk_err = "bad argument"; return -1; }
  const DeviceImage& img = h_->img;
  RenderParams P;
  if (const char* why = host_view(img, settings13, W, H, 0.0f, frame_seed, 1, 0, P)) { hk_err = why; return -1; }
  if (w <= 0 || h <= 0 || x0 < 0 || y0 < 0 || x0 > P.gx * 8 - w || y0 > P.gy * 8 - h) { hk_err = "window is empty or not inside the pixel grid"; return -1; }
  const int spp = hf2i(settings13[10]);
  if (nframes < 1 || spp < 1 || (long long)nframes * spp > 256) { hk_err = "a lens pass takes 1 .. 256 samples"; return -1; }
  fill_image(img, P);
  P.batch_seed_stride = seed_stride;
  const float focus = settings13[7];
  if (nthreads < 1) nthreads = 1;
  host_rows(nthreads, nthreads, [&](int k) {
    HostStack stack;
    with_closest<false>(P, traversal, stack.data(), [&](auto closest) {
      for (int wy = k; wy < h; wy += nthreads)
        for (int wx = 0; wx < w; wx++) {
          const AovLens a = aov_lens_pixel(P, closest, focus, x0 + wx, y0 + wy, nframes, spp, as_guides != 0);
          const size_t i = (size_t)wy * (size_t)w + (size_t)wx;
          if (coverage) coverage[i] = a.coverage;
          if (depth) depth[i] = a.depth;
          if (distance) distance[i] = a.distance;
          if (material) material[i] = a.mat;
          if (normal) st3(normal + 3 * i, a.normal);
          if (albedo) st3(albedo + 3 * i, a.albedo);
        }
    });
  });
  return 0;
}
}  // extern "C"
