// The accumulator stages on the host (hk_denoise, hk_upscale, hk_reproject, hk_moments_add, hk_error, hk_adaptive_select / _add): the launch structs of device_launch.h filled with
// host pointers and a loop over the pixels; no stage's arithmetic or indexing is written here.  A call is judged, and its launch struct's grid,
// sizes and parameters filled, by params_host.hpp's judge_* -- the judges the library runs; an entry here adds the pointers.  Part of host_kernel.cpp.
namespace {
// a parameter set handed over as words (null: the defaults): a dr_denoise_params, dr_upscale_params or dr_reproject_params
template <class T>
struct ParamWords {
  T p{};
  bool given;
  explicit ParamWords(const int32_t* words) : given(words != nullptr) { if (given) memcpy(&p, words, sizeof(T)); }
  const T* get() const { return given ? &p : nullptr; }
};

// The low side of hk_denoise and hk_upscale over the L.gw x L.gh pixel grid (L.D, L.acc, L.hist, L.m2 and the AOV planes L.normal, L.depth,
// L.albedo, L.mat set by the caller), stage by stage as denoise_low_side (context_accum.cpp) launches it: the guide prepare, colour stage 0 and
// -- filter -- the variance pre-pass and the L.D.iterations a-trous passes.  The planes live in `planes`; on return L.src is the plane of the
// result, (e, l) after stage 0, (e, var) after the last pass, and L.guide, L.gz are the guides.
struct HostLow {
  std::vector<float> guide, gz, pa, pb;      // float4 (n, z) | depth gradient | colour planes A, B (float4)
};
void host_denoise_low(DnLaunch& L, bool filter, int nthreads, HostLow& planes) {
  const size_t n = (size_t)L.gw * L.gh;
  planes.guide.resize(4 * n); planes.gz.resize(n); planes.pa.resize(4 * n); planes.pb.resize(4 * n);
  L.guide = planes.guide.data(); L.gz = planes.gz.data();
  host_grid(nthreads, L.gw, L.gh, [&](int x, int y) { dn_guide_pixel(L, x, y); });
  L.dst = planes.pa.data();
  host_grid(nthreads, L.gw, L.gh, [&](int x, int y) { dn_colour_pixel(L, x, y); });            // acc -> (e, l) in A
  L.src = planes.pa.data(); L.dst = planes.pb.data();
  if (!filter) return;
  host_grid(nthreads, L.gw, L.gh, [&](int x, int y) { dn_variance_pixel(L, x, y); });          // (e, l) -> (e, var) in B
  L.src = planes.pb.data(); L.dst = planes.pa.data();                                          // the passes: B -> A -> B ...
  for (int it = 0; it < L.D.iterations; it++) {
    host_grid(nthreads, L.gw, L.gh, [&](int x, int y) { dn_pass_pixel(L, 1 << it, x, y); });
    float* const t = const_cast<float*>(L.src);
    L.src = L.dst; L.dst = t;
  }
}
}  // namespace
extern "C" {
// dr_accum_denoise on the host: the stage bodies of device_denoise.hpp over the pixel grid of settings13 (host_denoise_low, then the finish), from guides given
// as arrays in dr_render_aov's layout (normal / albedo gw x gh x 3, depth / material gw x gh) -- hk_aov's, hk_aov_lens's guide form (option guide_frames) or the GPU's own.  acc: the column-major
// W x H x 3 accumulator; params: a dr_denoise_params (NULL: the defaults); out_f32 / out_rgb8 (either may be NULL): row-major W x H x 3.
// hist (may be NULL): the accumulator's history plane, W x H at x * H + y -- pixel p's divisor is hist[p] + divide_by.
// m2 (may be NULL): the second-moment plane, W x H at x * H + y -- option "denoise_variance" = 1: the variance pre-pass takes the temporal variance
// of pixels with four samples or more from it.  Returns 0, or -1 with hk_last_error.
int hk_denoise(const int32_t* acc, int W, int H, int divide_by, const float* settings13, const float* normal, const float* albedo, const float* depth,
               const int32_t* material, const int32_t* params, float* out_f32, uint8_t* out_rgb8, int nthreads, const int32_t* hist,
               const unsigned long long* m2) {
  if (!acc || !settings13 || !normal || !albedo || !depth || !material) { hk_err = "bad argument"; return -1; }
  RenderParams P;
  if (const char* why = host_view(settings13, W, H, 0.0f, 0, 1, 0, P)) { hk_err = why; return -1; }
  DnLaunch L;
  hk_err = judge_denoise(P, divide_by, ParamWords<dr_denoise_params>(params).get(), L);
  if (!hk_err.empty()) return -1;
  L.acc = acc; L.hist = hist; L.m2 = m2;
  L.normal = normal; L.depth = depth; L.albedo = albedo; L.mat = material;
  HostLow planes;
  if (L.D.iterations > 0) host_denoise_low(L, true, nthreads, planes);
  L.out_f32 = out_f32; L.out_rgb8 = out_rgb8;
  host_grid(nthreads, W, H, [&](int x, int y) { dn_finish_pixel(L, x, y); });
  return 0;
}

// dr_accum_upscale on the host: device_upscale.hpp over the output grid of settings13, from the low guides (the grid of settings13) and the full
// guides (settings13 with element 11 = 1) given as arrays in dr_render_aov's layout -- normal, albedo, depth, material each.  params: a
// dr_upscale_params (NULL: the defaults); prefilter: a dr_denoise_params or NULL -- the denoiser's host passes then run on the low grid first.
// out_f32 / out_rgb8 (either may be NULL): row-major W x H x 3; out_notap (may be NULL): W x H bytes, 1 where a guided pixel found no usable tap.
// hist / m2 as hk_denoise.  Returns 0, or -1 with hk_last_error.
int hk_upscale(const int32_t* acc, int W, int H, int divide_by, const float* settings13, const float* normal, const float* albedo, const float* depth,
               const int32_t* material, const float* fnormal, const float* falbedo, const float* fdepth, const int32_t* fmaterial, const int32_t* params,
               const int32_t* prefilter, float* out_f32, uint8_t* out_rgb8, uint8_t* out_notap, int nthreads, const int32_t* hist,
               const unsigned long long* m2) {
  if (!acc || !settings13) { hk_err = "bad argument"; return -1; }
  RenderParams P, PF;
  if (const char* why = host_view(settings13, W, H, 0.0f, 0, 1, 0, P)) { hk_err = why; return -1; }
  float full13[13];
  full_view13(settings13, full13);
  if (const char* why = host_view(full13, W, H, 0.0f, 0, 1, 0, PF)) { hk_err = why; return -1; }
  UpLaunch U;
  DnLaunch L;                                                               // the low side: the denoiser's planes
  hk_err = judge_upscale(P, PF, settings13, divide_by, ParamWords<dr_upscale_params>(params).get(), ParamWords<dr_denoise_params>(prefilter).get(), U, L);
  if (!hk_err.empty()) return -1;
  U.acc = acc; U.hist = hist;
  HostLow low;
  std::vector<float> fguide, fgz;
  if (U.U.mode == UP_GUIDED && U.gw > 0 && U.gh > 0) {
    if (!normal || !albedo || !depth || !material || !fnormal || !falbedo || !fdepth || !fmaterial) { hk_err = "bad argument"; return -1; }
    L.acc = acc; L.hist = hist; L.m2 = m2;
    L.normal = normal; L.depth = depth; L.albedo = albedo; L.mat = material;
    host_denoise_low(L, prefilter != nullptr, nthreads, low);
    U.e = L.src; U.guide = L.guide; U.mat = L.mat;
    DnLaunch G;                                                             // the full side: the guide prepare over the full grid
    memset(&G, 0, sizeof(G));
    G.gw = U.FW; G.gh = U.FH;
    fguide.resize((size_t)4 * U.FW * U.FH); fgz.resize((size_t)U.FW * U.FH);
    G.normal = fnormal; G.depth = fdepth; G.mat = fmaterial; G.guide = fguide.data(); G.gz = fgz.data();
    host_grid(nthreads, G.gw, G.gh, [&](int x, int y) { dn_guide_pixel(G, x, y); });
    U.Fguide = G.guide; U.Falbedo = falbedo; U.Fmat = fmaterial; U.Fgz = G.gz;
  }
  U.out_f32 = out_f32; U.out_rgb8 = out_rgb8;
  host_grid(nthreads, W, H, [&](int X, int Y) {
    bool notap = false;
    up_pixel(U, X, Y, &notap);
    if (out_notap) out_notap[(size_t)Y * W + X] = notap ? 1 : 0;
  });
  return 0;
}

// The float camera block of a view as fill_view_params forms it (what dr_accum_reproject's definition starts from): out12 = from, llc, hor, ver;
// den2 = den_w, den_h; grid2 = gw, gh.  Returns 0, or -1 with hk_last_error.
int hk_camera_block(const float* settings13, int W, int H, float* out12, double* den2, int* grid2) {
  RenderParams P;
  if (const char* why = host_view(settings13, W, H, 0.0f, 0, 1, 0, P)) { hk_err = why; return -1; }
  memcpy(out12, P.from, 12); memcpy(out12 + 3, P.llc, 12); memcpy(out12 + 6, P.hor, 12); memcpy(out12 + 9, P.ver, 12);
  den2[0] = P.den_w; den2[1] = P.den_h;
  grid2[0] = P.gx * 8; grid2[1] = P.gy * 8;
  return 0;
}

// dr_accum_reproject on the host: device_reproject.hpp over the pixel grid, from guides given as arrays in dr_render_aov's layout (t / material
// gw x gh, normal gw x gh x 3) for both views -- hk_aov's or the GPU's own.  acc_from / acc_to: column-major W x H x 3; hist_from (may be NULL) /
// hist_to: W x H at x * H + y; params: a dr_reproject_params (NULL: the defaults); counts[5]: pixels, valid, masked, offscreen, rejected.
// m2_from / m2_to (both or neither NULL): the second-moment planes, W x H at x * H + y, carried with the sums (device_moments.hpp mo_carry).
// Returns 0, or -1 with hk_last_error.
int hk_reproject(const int32_t* acc_from, const int32_t* hist_from, int W, int H, int frames, const float* from_settings13, const float* to_settings13,
                 const float* t_from, const float* normal_from, const int32_t* mat_from, const float* t_to, const float* normal_to, const int32_t* mat_to,
                 const int32_t* params, int32_t* acc_to, int32_t* hist_to, long long* counts, int nthreads, const unsigned long long* m2_from,
                 unsigned long long* m2_to) {
  if ((m2_from == nullptr) != (m2_to == nullptr)) { hk_err = "bad argument"; return -1; }
  if (!acc_from || !from_settings13 || !to_settings13 || !t_from || !normal_from || !mat_from || !t_to || !normal_to || !mat_to || !acc_to || !hist_to || !counts) { hk_err = "bad argument"; return -1; }
  RenderParams Pf, Pt;
  if (const char* why = host_view(from_settings13, W, H, 0.0f, 0, 1, 0, Pf)) { hk_err = why; return -1; }
  if (const char* why = host_view(to_settings13, W, H, 0.0f, 0, 1, 0, Pt)) { hk_err = why; return -1; }
  RpLaunch L;
  hk_err = judge_reproject(Pf, Pt, frames, ParamWords<dr_reproject_params>(params).get(), L);
  if (!hk_err.empty()) return -1;
  L.t_to = t_to; L.normal_to = normal_to; L.mat_to = mat_to;
  L.t_from = t_from; L.normal_from = normal_from; L.mat_from = mat_from;
  L.acc_from = acc_from; L.hist_from = hist_from; L.acc_to = acc_to; L.hist_to = hist_to;
  L.m2_from = m2_from; L.m2_to = m2_to;
  memset(acc_to, 0, (size_t)W * H * 3 * sizeof(int32_t));                   // (pixels outside the grid: the body writes every pixel of the grid)
  memset(hist_to, 0, (size_t)W * H * sizeof(int32_t));
  if (m2_to) memset(m2_to, 0, (size_t)W * H * sizeof(unsigned long long));
  std::vector<long long> part((size_t)L.gh * 4, 0);                         // the classes of every row
  host_rows(nthreads, L.gh, [&](int y) {
    long long row[4] = {0, 0, 0, 0};
    for (int x = 0; x < L.gw; x++) row[rp_pixel(L, x, y)]++;
    memcpy(&part[(size_t)y * 4], row, sizeof(row));
  });
  counts[0] = (long long)L.gw * L.gh;
  for (int c = 0; c < 4; c++) { counts[1 + c] = 0; for (int y = 0; y < L.gh; y++) counts[1 + c] += part[(size_t)y * 4 + (size_t)c]; }
  return 0;
}

// The fused add of the second-moment plane on the host (device_moments.hpp, as kernels_moments.hip runs it): acc += frame and m2 += the frame's capped
// luma squared, for npix pixels, in place.
int hk_moments_add(int32_t* acc, const int32_t* frame, unsigned long long* m2, long long npix) {
  if (!acc || !frame || !m2 || npix < 0) { hk_err = "bad argument"; return -1; }
  for (long long p = 0; p < npix; p++) mo_add_pixel(acc, frame, m2, (size_t)p);
  return 0;
}

// dr_accum_error on the host: device_moments.hpp over the pixel grid of settings13.  acc: column-major W x H x 3; hist (may be NULL) / m2: W x H at
// x * H + y; out_sigma (may be NULL): row-major W x H, 0 outside the grid; result (may be NULL): 19 words -- estimated, above, sum_var_q16, bins[16]
// (pixels = grid2[0] * grid2[1], returned in grid2).  Returns 0, or -1 with hk_last_error.
int hk_error(const int32_t* acc, const int32_t* hist, const unsigned long long* m2, int W, int H, int divide_by, float tolerance, const float* settings13,
             float* out_sigma, unsigned long long* result, int* grid2, int nthreads) {
  if (!acc || !m2 || !settings13 || (!out_sigma && !result)) { hk_err = "bad argument"; return -1; }
  RenderParams P;
  if (const char* why = host_view(settings13, W, H, 0.0f, 0, 1, 0, P)) { hk_err = why; return -1; }
  MoLaunch L;
  hk_err = judge_error(P, divide_by, tolerance, L);
  if (!hk_err.empty()) return -1;
  L.acc = acc; L.hist = hist; L.m2 = m2; L.out_sigma = out_sigma;
  if (grid2) { grid2[0] = L.gw; grid2[1] = L.gh; }
  if (out_sigma) memset(out_sigma, 0, (size_t)W * H * sizeof(float));
  std::vector<unsigned long long> part((size_t)L.gh * MO_WORDS, 0);         // the counts of every row
  host_rows(nthreads, L.gh, [&](int y) {
    unsigned long long cnt[MO_WORDS] = {0};
    for (int x = 0; x < L.gw; x++) {
      double var;
      float sigma;
      if (!mo_error_pixel(L, x, y, var, sigma)) continue;
      cnt[MO_ESTIMATED]++;
      if (sigma > L.tolerance) cnt[MO_ABOVE]++;
      cnt[MO_SUM_VAR] += mo_var_q16(var);
      cnt[MO_BIN0 + mo_bin(sigma)]++;
    }
    memcpy(&part[(size_t)y * MO_WORDS], cnt, sizeof(cnt));
  });
  if (result)
    for (int w = 0; w < MO_WORDS; w++) { result[w] = 0; for (int y = 0; y < L.gh; y++) result[w] += part[(size_t)y * MO_WORDS + (size_t)w]; }
  return 0;
}

// dr_render_adaptive's selection on the host: device_adaptive.hpp over the tiles of settings13's pixel grid.  Planes as hk_error's (hist may be NULL);
// params: a dr_adaptive_params (NULL: the defaults); flags: a byte per tile; counts[2]: active tiles, asking pixels; grid2: gx, gy.
// Returns 0, or -1 with hk_last_error (the library's refusals of nframes -- pass 1 --, divide_by and the parameters).
int hk_adaptive_select(const int32_t* acc, const int32_t* hist, const unsigned long long* m2, int W, int H, int divide_by, const float* settings13,
                       const int32_t* params, uint8_t* flags, long long* counts, int* grid2) {
  if (!acc || !m2 || !settings13 || !flags || !counts) { hk_err = "bad argument"; return -1; }
  RenderParams P;
  if (const char* why = host_view(settings13, W, H, 0.0f, 0, 1, 0, P)) { hk_err = why; return -1; }
  AdLaunch L;
  hk_err = judge_adaptive(P, 1, divide_by, ParamWords<dr_adaptive_params>(params).get(), L);
  if (!hk_err.empty()) return -1;
  L.acc = const_cast<int32_t*>(acc); L.hist = const_cast<int32_t*>(hist); L.m2 = const_cast<unsigned long long*>(m2);
  if (grid2) { grid2[0] = L.gx; grid2[1] = L.gy; }
  counts[AD_ACTIVE] = counts[AD_ASKING] = 0;
  for (int t = 0; t < L.gx * L.gy; t++) {
    int asking = 0;
    for (int lane = 0; lane < 64; lane++) asking += ad_asks(L, t, lane) ? 1 : 0;
    flags[t] = ad_tile_active(L, asking) ? 1 : 0;
    counts[AD_ACTIVE] += flags[t]; counts[AD_ASKING] += asking;
  }
  return 0;
}

// device_split.hpp order_split_plain by FlagKeep: order may be NULL (identity); launch_region_start 2 * MAX_REGIONS + 1 ints; returns the number of flagged tiles
int hk_subset_split(const int* order, const int* region_start, const uint8_t* flag, int tiles, int regions, int* launch_order, int* launch_region_start) {
  return order_split_plain(order, region_start, FlagKeep{flag}, tiles, regions, launch_order, launch_region_start, nullptr).kept;
}

// dr_render_adaptive's fold on the host: ad_fold_pixel over the n tiles of list (tile = block column * gy + row of settings13's grid), IN PLACE --
// nframes frames in the accumulator's layout, frame f at frames + f * W * H * 3.  Returns 0, or -1 with hk_last_error.
int hk_adaptive_add(int32_t* acc, int32_t* hist, unsigned long long* m2, int W, int H, const float* settings13, const int32_t* frames, int nframes,
                    const int* list, int n) {
  if (!acc || !hist || !m2 || !settings13 || !frames || (n > 0 && !list)) { hk_err = "bad argument"; return -1; }
  RenderParams P;
  if (const char* why = host_view(settings13, W, H, 0.0f, 0, 1, 0, P)) { hk_err = why; return -1; }
  AdLaunch L;
  hk_err = judge_adaptive(P, nframes, 0, nullptr, L);
  if (!hk_err.empty()) return -1;
  L.acc = acc; L.hist = hist; L.m2 = m2; L.frames = frames; L.frame_stride = (size_t)W * H * 3;
  for (int i = 0; i < n; i++) {
    if (list[i] < 0 || list[i] >= L.gx * L.gy) { hk_err = "adaptive: a listed tile is outside the grid"; return -1; }
    for (int lane = 0; lane < 64; lane++) ad_fold_pixel(L, list[i], lane);
  }
  return 0;
}
}  // extern "C"
