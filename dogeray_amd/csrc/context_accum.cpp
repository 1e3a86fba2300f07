// The accumulator and what is computed from it on the device: reset, first-hit AOVs, the denoiser, the upscaler, temporal reprojection, the noise
// estimate, present, the stripe copies of the multi-GPU gather, reads and device pointers.
#include <utility>

#include "context.hpp"

using namespace dr;

namespace {

// The view of a first-hit AOV pass (dr_render_aov, dr_accum_*): the context's device made current, the scene present, the settings judged as
// dr_render_frame judges them (make_params) without touching the context's state, and the resident scene's buffers
int aov_view(dr_context* c, const float settings13[13], int W, int H, RenderParams& P, int& traversal) {
  HIP_TRY(hipSetDevice(c->device));
  if (!c->walk) { set_error("no scene uploaded"); return DR_ERR_INVALID; }
  memset(&P, 0, sizeof(P));
  if (const char* why = fill_view_params(settings13, W, H, 0.0f, 0, 1, 0, P)) { set_error(why); return DR_ERR_INVALID; }
  if (P.backtex >= c->n_tex) { set_error("backtex refers to a texture that is not loaded"); return DR_ERR_INVALID; }
  traversal = traversal_of(c);
  if (traversal == DR_TRAVERSAL_ORDERED && c->tree_depth > ORDERED_STACK) { set_error("tree too deep for ordered traversal"); return DR_ERR_SCENE; }
  fill_scene(c, P);
  return DR_OK;
}

// The W x H a dr_accum_* call (`who`: the word its messages start with) was given is the accumulator's
int accum_matches(const dr_context* c, const char* who, int W, int H) {
  if (!c->accum) { set_error("no accumulator: call dr_accum_reset(W, H) first"); return DR_ERR_INVALID; }
  if (W != c->accW || H != c->accH) {
    set_error(std::string(who) + ": " + std::to_string(W) + " x " + std::to_string(H) + " is not the accumulator's " + std::to_string(c->accW) + " x " + std::to_string(c->accH));
    return DR_ERR_INVALID;
  }
  return DR_OK;
}

// Traces the guides of view P over its gw x gh pixel grid: launch_aov writes normal and depth into `scratch` (3n + n floats), albedo and
// material into their planes; the guide prepare packs (n, z) into `guide` and forms gz from them
int trace_guides(dr_context* c, const RenderParams& P, int traversal, float focus, int gw, int gh, float* scratch, float* albedo, int32_t* mat,
                 float* guide, float* gz) {
  const size_t n = (size_t)gw * (size_t)gh;
  AovLaunch A;
  memset(&A, 0, sizeof(A));
  A.x0 = 0; A.y0 = 0; A.w = gw; A.h = gh;
  A.focus = focus;
  A.slot_to_orig = c->slot_to_orig_dev;
  A.normal = scratch; A.depth = scratch + 3 * n; A.albedo = albedo; A.material = mat;
  launch_aov(c->stream, P, traversal, A);
  HIP_TRY(hipGetLastError());
  DnLaunch G;
  memset(&G, 0, sizeof(G));
  G.gw = gw; G.gh = gh;
  G.normal = scratch; G.depth = scratch + 3 * n; G.mat = mat; G.guide = guide; G.gz = gz;
  launch_denoise_guides(c->stream, G);
  HIP_TRY(hipGetLastError());
  return DR_OK;
}

// The low side of dr_accum_denoise and dr_accum_upscale over the pixel grid of settings13 (L.gw x L.gh > 0; L.D, L.acc, L.hist, L.m2 set by the
// caller): the planes (allocated by the first call), the cached guides (traced when the key differs; *aov_passes counts that pass), colour stage 0
// and -- filter -- the variance pre-pass and the L.D.iterations a-trous passes.  On return L.src is the plane of the result: (e, l) after stage 0,
// (e, var) after the last pass; L.guide, L.albedo, L.mat and L.gz are the guides.
int denoise_low_side(dr_context* c, const float settings13[13], int W, int H, const RenderParams& P, int traversal, DnLaunch& L, bool filter, int* aov_passes) {
  const size_t n = (size_t)L.gw * (size_t)L.gh;
  // planes, in floats: guide 4n | colour A 4n | colour B 4n | albedo 3n | material n | gz n (the float4 planes first: 16-byte aligned, n % 8 == 0)
  if (17 * n > c->dn_planes.n) c->dn_key.valid = false;
  DR_TRY(c->dn_planes.grow(17 * n, c->stream));
  float* const guide = c->dn_planes;
  float* const pa = guide + 4 * n;
  float* const pb = pa + 4 * n;
  float* const albedo = pb + 4 * n;
  int32_t* const mat = reinterpret_cast<int32_t*>(albedo + 3 * n);
  float* const gz = reinterpret_cast<float*>(mat + n);
  L.albedo = albedo; L.mat = mat; L.guide = guide; L.gz = gz;
  if (!c->dn_key.matches(settings13, W, H, c->scene_gen)) {
    DR_TRY(trace_guides(c, P, traversal, settings13[7], L.gw, L.gh, pa, albedo, mat, guide, gz));      // (colour plane A is the scratch)
    c->dn_key.store(settings13, W, H, c->scene_gen);
    if (aov_passes) ++*aov_passes;
  }
  L.dst = pa;
  launch_denoise_colour(c->stream, L, 0);                 // acc -> (e, l) in A
  L.src = pa; L.dst = pb;
  if (filter) {
    launch_denoise_colour(c->stream, L, 1);               // (e, l) -> (e, var) in B
    L.src = pb; L.dst = pa;                               // the passes: B -> A -> B ...
    for (int it = 0; it < L.D.iterations; it++) {
      launch_denoise_pass(c->stream, L, 1 << it, c->denoise_tiles);
      float* const t = const_cast<float*>(L.src);
      L.src = L.dst; L.dst = t;
    }
  }
  HIP_TRY(hipGetLastError());
  return DR_OK;
}

// Where the W x H outputs of dr_accum_denoise / dr_accum_upscale are written: the caller's device buffers, or the staging they are downloaded from
int output_staging(dr_context* c, size_t npix, float* out_f32, uint8_t* out_rgb8, int device_pointers, float*& f32_dev, uint8_t*& rgb_dev) {
  f32_dev = out_f32;
  rgb_dev = out_rgb8;
  if (device_pointers) return DR_OK;
  DR_TRY(c->dn_staging.grow((out_f32 ? npix * 3 * sizeof(float) : 0) + (out_rgb8 ? npix * 3 : 0), c->stream));
  f32_dev = out_f32 ? reinterpret_cast<float*>(c->dn_staging.p) : nullptr;
  rgb_dev = out_rgb8 ? c->dn_staging + (out_f32 ? npix * 3 * sizeof(float) : 0) : nullptr;
  return DR_OK;
}
int output_download(dr_context* c, size_t npix, float* out_f32, uint8_t* out_rgb8, const float* f32_dev, const uint8_t* rgb_dev) {
  if (out_f32) HIP_TRY(hipMemcpyAsync(out_f32, f32_dev, npix * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  if (out_rgb8) HIP_TRY(hipMemcpyAsync(out_rgb8, rgb_dev, npix * 3, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return DR_OK;
}

}  // namespace

extern "C" {

int dr_accum_reset(dr_context* c, int W, int H) {
  if (!c || W <= 0 || H <= 0) { set_error("bad argument"); return DR_ERR_INVALID; }
  HIP_TRY(hipSetDevice(c->device));
  DR_TRY(join_pipeline(c));
  size_t elems = (size_t)W * H * 3;
  DR_TRY(c->accum.grow(elems, c->stream));
  c->accW = W; c->accH = H;
  c->hist = nullptr;               // the history plane goes with the sums it counted
  HIP_TRY(hipMemsetAsync(c->accum, 0, elems * sizeof(int32_t), c->stream));
  if (c->moments_opt) {            // a zeroed second-moment plane (the allocation is kept across resets of the same size: the preview ladder resets four times)
    c->m2 = nullptr;
    DR_TRY(c->m2_buf[0].grow((size_t)W * H, c->stream));
    c->m2 = c->m2_buf[0]; c->m2_cur = 0;
    HIP_TRY(hipMemsetAsync(c->m2, 0, (size_t)W * H * sizeof(unsigned long long), c->stream));
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (!c->moments_opt) {           // the plane is dropped (nothing uses it any more: the stream has drained)
    c->m2 = nullptr;
    c->m2_buf[0].release(); c->m2_buf[1].release();
  }
  return DR_OK;
}

int dr_render_aov(dr_context* c, const float settings13[13], int W, int H, int x0, int y0, int w, int h, const dr_aov_buffers* buffers,
                  int device_pointers) {
  if (!c || !settings13 || !buffers) { set_error("null argument"); return DR_ERR_INVALID; }
  RenderParams P;
  int traversal = 0;
  DR_TRY(aov_view(c, settings13, W, H, P, traversal));
  const int gw = P.gx * 8, gh = P.gy * 8;
  if (w <= 0 || h <= 0) { set_error("empty AOV window"); return DR_ERR_INVALID; }
  if (x0 < 0 || y0 < 0 || x0 > gw - w || y0 > gh - h) {
    set_error("AOV window (" + std::to_string(x0) + ", " + std::to_string(y0) + ", " + std::to_string(w) + ", " + std::to_string(h) +
              ") is not inside the " + std::to_string(gw) + " x " + std::to_string(gh) + " pixel grid");
    return DR_ERR_INVALID;
  }
  DR_TRY(join_pipeline(c));      // ordered behind the frames submitted before
  DR_TRY(ensure_slot_to_orig(c));
  AovLaunch A;
  A.x0 = x0; A.y0 = y0; A.w = w; A.h = h;
  A.focus = settings13[7];
  A.slot_to_orig = c->slot_to_orig_dev;
  // channel k: where the caller wants it, the device buffer it is written to, its words per pixel
  void* const want[9] = {buffers->t, buffers->distance, buffers->depth, buffers->object, buffers->material, buffers->normal, buffers->uv, buffers->albedo, buffers->dir};
  const int words[9] = {1, 1, 1, 1, 1, 3, 2, 3, 3};
  void* dev[9] = {nullptr};
  const size_t npix = (size_t)w * (size_t)h;
  bool any = false;
  if (device_pointers) {
    for (int k = 0; k < 9; k++) { dev[k] = want[k]; any = any || want[k]; }
  } else {
    size_t bytes = 0;
    for (int k = 0; k < 9; k++) if (want[k]) bytes += npix * (size_t)words[k] * 4;
    if (bytes > 0) DR_TRY(c->aov_staging.grow(bytes, c->stream));
    size_t off = 0;
    for (int k = 0; k < 9; k++) if (want[k]) { dev[k] = c->aov_staging + off; off += npix * (size_t)words[k] * 4; any = true; }
  }
  if (!any) return DR_OK;
  A.t = (float*)dev[0]; A.distance = (float*)dev[1]; A.depth = (float*)dev[2]; A.object = (int32_t*)dev[3]; A.material = (int32_t*)dev[4];
  A.normal = (float*)dev[5]; A.uv = (float*)dev[6]; A.albedo = (float*)dev[7]; A.dir = (float*)dev[8];
  launch_aov(c->stream, P, traversal, A);
  HIP_TRY(hipGetLastError());
  if (device_pointers) return DR_OK;
  for (int k = 0; k < 9; k++)
    if (want[k]) HIP_TRY(hipMemcpyAsync(want[k], dev[k], npix * (size_t)words[k] * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return DR_OK;
}

int dr_denoise_defaults(dr_denoise_params* p) {
  if (!p) { set_error("null argument"); return DR_ERR_INVALID; }
  const DnParams& D = DN_DEFAULTS;
  p->iterations = D.iterations; p->sigma_luminance = D.sigma_luminance; p->normal_power_log2 = D.normal_power_log2;
  p->sigma_depth = D.sigma_depth; p->demodulate = D.demodulate; p->material_stop = D.material_stop;
  return DR_OK;
}

int dr_accum_denoise(dr_context* c, const float settings13[13], int W, int H, int divide_by, const dr_denoise_params* params, float* out_f32,
                     uint8_t* out_rgb8, int device_pointers) {
  if (!c || !settings13) { set_error("null argument"); return DR_ERR_INVALID; }
  RenderParams P;
  int traversal = 0;
  DR_TRY(aov_view(c, settings13, W, H, P, traversal));
  DR_TRY(accum_matches(c, "denoise", W, H));
  if (divide_by < 1) { set_error("denoise: divide_by must be >= 1"); return DR_ERR_INVALID; }
  const DnParams D = params ? dn_params(*params) : DN_DEFAULTS;
  if (const char* why = check_denoise_params(D)) { set_error(std::string("denoise: ") + why); return DR_ERR_INVALID; }
  if (!out_f32 && !out_rgb8) { set_error("denoise: no output (both out_f32 and out_rgb8 are NULL)"); return DR_ERR_INVALID; }
  DR_TRY(join_pipeline(c));      // ordered behind the frames submitted before

  const int gw = P.gx * 8, gh = P.gy * 8;
  const size_t n = (size_t)gw * (size_t)gh, npix = (size_t)W * (size_t)H;
  DnLaunch L;
  memset(&L, 0, sizeof(L));
  L.gw = gw; L.gh = gh; L.W = W; L.H = H; L.divide_by = divide_by;
  L.D = D;
  L.acc = c->accum; L.hist = c->hist;
  L.m2 = c->denoise_variance ? c->m2 : nullptr;
  if (D.iterations > 0 && n > 0) DR_TRY(denoise_low_side(c, settings13, W, H, P, traversal, L, true, nullptr));
  float* f32_dev;
  uint8_t* rgb_dev;
  DR_TRY(output_staging(c, npix, out_f32, out_rgb8, device_pointers, f32_dev, rgb_dev));
  L.out_f32 = f32_dev; L.out_rgb8 = rgb_dev;
  launch_denoise_finish(c->stream, L);
  HIP_TRY(hipGetLastError());
  if (device_pointers) return DR_OK;
  return output_download(c, npix, out_f32, out_rgb8, f32_dev, rgb_dev);
}

int dr_upscale_defaults(dr_upscale_params* p) {
  if (!p) { set_error("null argument"); return DR_ERR_INVALID; }
  const UpParams& U = UP_DEFAULTS;
  p->mode = U.mode; p->normal_power_log2 = U.normal_power_log2; p->sigma_depth = U.sigma_depth; p->demodulate = U.demodulate; p->material_stop = U.material_stop;
  return DR_OK;
}

int dr_accum_upscale(dr_context* c, const float settings13[13], int W, int H, int divide_by, const dr_upscale_params* params,
                     const dr_denoise_params* prefilter, float* out_f32, uint8_t* out_rgb8, int device_pointers) {
  if (!c || !settings13) { set_error("null argument"); return DR_ERR_INVALID; }
  RenderParams P, PF;
  int traversal = 0;
  DR_TRY(aov_view(c, settings13, W, H, P, traversal));
  float full13[13];                                        // the same view at full resolution
  memcpy(full13, settings13, sizeof(full13));
  full13[11] = 1.0f;
  DR_TRY(aov_view(c, full13, W, H, PF, traversal));
  DR_TRY(accum_matches(c, "upscale", W, H));
  if (divide_by < 1) { set_error("upscale: divide_by must be >= 1"); return DR_ERR_INVALID; }
  const UpParams UP = params ? up_params(*params) : UP_DEFAULTS;
  const DnParams PRE = prefilter ? dn_params(*prefilter) : DnParams{};
  const DnParams* const pre = prefilter ? &PRE : nullptr;
  const std::string why = check_upscale_params(UP, pre);
  if (!why.empty()) { set_error(why); return DR_ERR_INVALID; }
  if (!out_f32 && !out_rgb8) { set_error("upscale: no output (both out_f32 and out_rgb8 are NULL)"); return DR_ERR_INVALID; }
  DR_TRY(join_pipeline(c));      // ordered behind the frames submitted before

  const int gw = P.gx * 8, gh = P.gy * 8, FW = PF.gx * 8, FH = PF.gy * 8;
  const size_t n = (size_t)gw * (size_t)gh, nf = (size_t)FW * (size_t)FH, npix = (size_t)W * (size_t)H;
  UpLaunch U;
  memset(&U, 0, sizeof(U));
  U.gw = gw; U.gh = gh; U.FW = FW; U.FH = FH; U.W = W; U.H = H; U.div = n > 0 ? (int)settings13[11] : 1; U.divide_by = divide_by;
  U.U = UP;
  U.acc = c->accum; U.hist = c->hist;
  c->up_passes = 0;
  if (UP.mode == UP_GUIDED && n > 0) {
    // the low side: the denoiser's planes; without a prefilter only the demodulated colour of stage 0
    DnLaunch L;
    memset(&L, 0, sizeof(L));
    L.gw = gw; L.gh = gh; L.W = W; L.H = H; L.divide_by = divide_by;
    L.D = up_low_params(UP, pre);
    L.acc = c->accum; L.hist = c->hist;
    L.m2 = c->denoise_variance ? c->m2 : nullptr;
    DR_TRY(denoise_low_side(c, settings13, W, H, P, traversal, L, pre != nullptr, &c->up_passes));
    U.e = L.src; U.guide = L.guide; U.mat = L.mat;
    // the full side: planes of its own (guide 4nf | scratch 4nf | albedo 3nf | material nf | gz nf floats), traced once per view
    if (13 * nf > c->up_planes.n) c->up_key.valid = false;
    DR_TRY(c->up_planes.grow(13 * nf, c->stream));
    float* const fguide = c->up_planes;
    float* const scratch = fguide + 4 * nf;
    float* const falbedo = scratch + 4 * nf;
    int32_t* const fmat = reinterpret_cast<int32_t*>(falbedo + 3 * nf);
    float* const fgz = reinterpret_cast<float*>(fmat + nf);
    if (!c->up_key.matches(full13, W, H, c->scene_gen)) {
      DR_TRY(trace_guides(c, PF, traversal, full13[7], FW, FH, scratch, falbedo, fmat, fguide, fgz));
      c->up_key.store(full13, W, H, c->scene_gen);
      c->up_passes++;
    }
    U.Fguide = fguide; U.Falbedo = falbedo; U.Fmat = fmat; U.Fgz = fgz;
  }
  float* f32_dev;
  uint8_t* rgb_dev;
  DR_TRY(output_staging(c, npix, out_f32, out_rgb8, device_pointers, f32_dev, rgb_dev));
  U.out_f32 = f32_dev; U.out_rgb8 = rgb_dev;
  launch_upscale(c->stream, U);
  HIP_TRY(hipGetLastError());
  if (device_pointers) return DR_OK;
  return output_download(c, npix, out_f32, out_rgb8, f32_dev, rgb_dev);
}

int dr_reproject_defaults(dr_reproject_params* p) {
  if (!p) { set_error("null argument"); return DR_ERR_INVALID; }
  const RpParams& R = RP_DEFAULTS;
  p->max_history = R.max_history; p->normal_cos = R.normal_cos; p->plane_tolerance = R.plane_tolerance; p->material_mask = R.material_mask; p->sky = R.sky;
  return DR_OK;
}

int dr_accum_reproject(dr_context* c, const float from_settings13[13], const float to_settings13[13], int W, int H, int frames,
                       const dr_reproject_params* params, dr_reproject_result* result) {
  if (!c || !from_settings13 || !to_settings13) { set_error("null argument"); return DR_ERR_INVALID; }
  RenderParams Pf, Pt;
  int traversal = 0;
  DR_TRY(aov_view(c, from_settings13, W, H, Pf, traversal));
  DR_TRY(aov_view(c, to_settings13, W, H, Pt, traversal));
  if (Pf.gx != Pt.gx || Pf.gy != Pt.gy || Pf.den_w != Pt.den_w || Pf.den_h != Pt.den_h) { set_error("reproject: the two views have different divisors"); return DR_ERR_INVALID; }
  if (c->stripe_mod != 1 || c->stripe_rem != 0) { set_error("reproject: the context renders a stripe (dr_context_set_stripe); only (1, 0) is supported"); return DR_ERR_INVALID; }
  DR_TRY(accum_matches(c, "reproject", W, H));
  if (frames < 1) { set_error("reproject: frames must be >= 1"); return DR_ERR_INVALID; }
  RpLaunch L;
  memset(&L, 0, sizeof(L));
  L.R = params ? rp_params(*params) : RP_DEFAULTS;
  if (const char* why = check_reproject_params(L.R)) { set_error(why); return DR_ERR_INVALID; }
  fill_reproject_camera(Pt, L.to);
  fill_reproject_camera(Pf, L.from);
  if (!fill_reproject_proj(L.from, L.J)) { set_error("reproject: the `from` view is degenerate (its focus plane has no normal facing the camera)"); return DR_ERR_INVALID; }
  DR_TRY(join_pipeline(c));      // ordered behind the frames submitted before

  const int gw = Pt.gx * 8, gh = Pt.gy * 8;
  const size_t n = (size_t)gw * (size_t)gh, npix = (size_t)W * (size_t)H;
  DR_TRY(c->accum2.grow(npix * 3, c->stream));
  const int hto = c->hist ? 1 - c->hist_cur : 0;
  DR_TRY(c->hist_buf[hto].grow(npix, c->stream));
  const int mto = 1 - c->m2_cur;                               // (a second-moment plane is carried into the other buffer of its pair)
  if (c->m2) DR_TRY(c->m2_buf[mto].grow(npix, c->stream));
  DR_TRY(c->rp_counts.grow(4, c->stream));
  // the guides: the cached planes serve as `from` when their key matches; the `to` view is traced into the other set (into none when it is
  // the `from` view itself) and becomes the cache
  const bool warm = c->rp_key.matches(from_settings13, W, H, c->scene_gen);
  const bool same_view = memcmp(from_settings13, to_settings13, 13 * sizeof(float)) == 0;
  const int sf = warm ? c->rp_cur : 0, st = same_view ? sf : 1 - sf;
  c->rp_key.valid = false;
  c->rp_passes = 0;
  // (t, normal and material only, no guide prepare: not trace_guides)
  auto trace = [&](int set, const RenderParams& P, const float* st13) -> int {
    if (n == 0) return DR_OK;
    DR_TRY(c->rp_planes[set].grow(5 * n, c->stream));
    AovLaunch A;
    memset(&A, 0, sizeof(A));
    A.x0 = 0; A.y0 = 0; A.w = gw; A.h = gh;
    A.focus = st13[7];
    A.t = c->rp_planes[set]; A.normal = c->rp_planes[set] + n; A.material = reinterpret_cast<int32_t*>(c->rp_planes[set] + 4 * n);
    launch_aov(c->stream, P, traversal, A);
    HIP_TRY(hipGetLastError());
    c->rp_passes++;
    return DR_OK;
  };
  if (!warm) DR_TRY(trace(sf, Pf, from_settings13));
  if (!same_view) DR_TRY(trace(st, Pt, to_settings13));
  L.gw = gw; L.gh = gh; L.W = W; L.H = H; L.frames = frames;
  if (n > 0) {
    L.t_from = c->rp_planes[sf]; L.normal_from = c->rp_planes[sf] + n; L.mat_from = reinterpret_cast<const int32_t*>(c->rp_planes[sf] + 4 * n);
    L.t_to = c->rp_planes[st]; L.normal_to = c->rp_planes[st] + n; L.mat_to = reinterpret_cast<const int32_t*>(c->rp_planes[st] + 4 * n);
  }
  L.acc_from = c->accum; L.hist_from = c->hist;
  L.acc_to = c->accum2; L.hist_to = c->hist_buf[hto];
  L.m2_from = c->m2; L.m2_to = c->m2 ? c->m2_buf[mto].p : nullptr;
  L.counts = c->rp_counts;
  HIP_TRY(hipMemsetAsync(c->rp_counts, 0, 4 * sizeof(unsigned long long), c->stream));
  if (gw < W || gh < H) {                                     // pixels outside the grid are 0
    HIP_TRY(hipMemsetAsync(c->accum2, 0, npix * 3 * sizeof(int32_t), c->stream));
    HIP_TRY(hipMemsetAsync(c->hist_buf[hto], 0, npix * sizeof(int32_t), c->stream));
    if (L.m2_to) HIP_TRY(hipMemsetAsync(L.m2_to, 0, npix * sizeof(unsigned long long), c->stream));
  }
  launch_reproject(c->stream, L);
  HIP_TRY(hipGetLastError());
  unsigned long long counts[4] = {0, 0, 0, 0};
  HIP_TRY(hipMemcpyAsync(counts, c->rp_counts, sizeof(counts), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  // the pair of the `to` view is the current one from here on
  c->accum.swap(c->accum2);
  c->hist = c->hist_buf[hto]; c->hist_cur = hto;
  if (c->m2) { c->m2 = c->m2_buf[mto]; c->m2_cur = mto; }
  c->rp_key.store(to_settings13, W, H, c->scene_gen);
  c->rp_cur = st; c->rp_key.valid = n > 0;
  if (result) {
    result->pixels = (int64_t)n;
    result->valid = (int64_t)counts[RP_VALID]; result->masked = (int64_t)counts[RP_MASKED];
    result->offscreen = (int64_t)counts[RP_OFFSCREEN]; result->rejected = (int64_t)counts[RP_REJECTED];
  }
  return DR_OK;
}

int dr_accum_reserve_pack(dr_context* c, int slot) {
  if (!c || !c->accum || (slot != 0 && slot != 1)) { set_error("pack: no accumulator, or slot not 0/1"); return DR_ERR_INVALID; }
  HIP_TRY(hipSetDevice(c->device));
  DR_TRY(join_pipeline(c));
  const int gx = c->accW / 8;
  const size_t run = (size_t)8 * (size_t)c->accH * 3;                 // int32 per block column
  // sized for the largest stripe of this partition (rank 0's), so that every rank's buffer can take part in one
  // equal-sized gather
  const size_t need = (size_t)((gx + c->stripe_mod - 1) / c->stripe_mod > 0 ? (gx + c->stripe_mod - 1) / c->stripe_mod : 1) * run;
  return c->packed[slot].grow(need, c->stream);
}

int dr_accum_pack_stripe(dr_context* c, int slot, void** dev_ptr, uint64_t* bytes) {
  if (!c || !c->accum || (slot != 0 && slot != 1)) { set_error("pack: no accumulator, or slot not 0/1"); return DR_ERR_INVALID; }
  HIP_TRY(hipSetDevice(c->device));
  DR_TRY(join_pipeline(c));
  const int gx = c->accW / 8;
  const int ncols = gx > c->stripe_rem ? (gx - c->stripe_rem + c->stripe_mod - 1) / c->stripe_mod : 0;
  const size_t run = (size_t)8 * (size_t)c->accH * 3;                 // int32 per block column
  DR_TRY(dr_accum_reserve_pack(c, slot));
  if (ncols > 0) {
    const int run4 = (int)(run / 4);
    launch_stripe_copy(c->stream, c->packed[slot], c->accum, ncols, run4, 0ll, (long long)run4, (long long)c->stripe_rem * run4, (long long)c->stripe_mod * run4);
    HIP_TRY(hipGetLastError());
  }
  if (dev_ptr) *dev_ptr = c->packed[slot];
  if (bytes) *bytes = (uint64_t)ncols * run * sizeof(int32_t);
  return DR_OK;
}

int dr_accum_unpack_stripes(dr_context* c, const void* packed_dev, uint64_t rank_stride_bytes, int world, int first_rank, void* hip_stream) {
  if (!c || !c->accum || !packed_dev || world < 1 || first_rank < 0 || first_rank > world || (rank_stride_bytes & 15ull)) { set_error("unpack: bad argument"); return DR_ERR_INVALID; }
  HIP_TRY(hipSetDevice(c->device));
  DR_TRY(join_pipeline(c));      // the frames submitted before are added before the stripes are written over the sums (a stream of the caller's is ordered by the caller)
  hipStream_t stream = hip_stream ? (hipStream_t)hip_stream : c->stream;
  const int gx = c->accW / 8;
  const size_t run = (size_t)8 * (size_t)c->accH * 3;
  const int run4 = (int)(run / 4);
  for (int r = first_rank; r < world; r++) {
    const int ncols = gx > r ? (gx - r + world - 1) / world : 0;
    if (ncols == 0) continue;
    if ((uint64_t)ncols * run * sizeof(int32_t) > rank_stride_bytes) { set_error("unpack: a rank's stripe is larger than rank_stride_bytes"); return DR_ERR_INVALID; }
    launch_stripe_copy(stream, c->accum, reinterpret_cast<const int32_t*>(packed_dev), ncols, run4, (long long)r * run4, (long long)world * run4,
                       (long long)((uint64_t)r * rank_stride_bytes / 16), (long long)run4);
  }
  HIP_TRY(hipGetLastError());
  return DR_OK;
}

int dr_accum_read(dr_context* c, int32_t* out_int3) {
  if (!c || !out_int3 || !c->accum) { set_error("no accumulator"); return DR_ERR_INVALID; }
  HIP_TRY(hipSetDevice(c->device));
  DR_TRY(join_pipeline(c));
  HIP_TRY(hipMemcpyAsync(out_int3, c->accum, (size_t)c->accW * c->accH * 3 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return DR_OK;
}

int dr_accum_history_read(dr_context* c, int32_t* out) {
  if (!c || !out || !c->accum) { set_error("no accumulator"); return DR_ERR_INVALID; }
  HIP_TRY(hipSetDevice(c->device));
  DR_TRY(join_pipeline(c));
  const size_t n = (size_t)c->accW * c->accH;
  if (!c->hist) { memset(out, 0, n * sizeof(int32_t)); return DR_OK; }
  HIP_TRY(hipMemcpyAsync(out, c->hist, n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return DR_OK;
}

int dr_accum_history_device_ptr(dr_context* c, void** dev_ptr, uint64_t* bytes) {
  if (!c || !dev_ptr || !c->accum) { set_error("no accumulator"); return DR_ERR_INVALID; }
  HIP_TRY(hipSetDevice(c->device));
  DR_TRY(join_pipeline(c));      // as dr_accum_device_ptr
  *dev_ptr = c->hist;
  if (bytes) *bytes = c->hist ? (uint64_t)c->accW * c->accH * sizeof(int32_t) : 0;
  return DR_OK;
}

int dr_accum_moments_read(dr_context* c, uint64_t* out) {
  if (!c || !out || !c->accum) { set_error("no accumulator"); return DR_ERR_INVALID; }
  HIP_TRY(hipSetDevice(c->device));
  DR_TRY(join_pipeline(c));
  const size_t n = (size_t)c->accW * c->accH;
  if (!c->m2) { memset(out, 0, n * sizeof(uint64_t)); return DR_OK; }
  HIP_TRY(hipMemcpyAsync(out, c->m2, n * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return DR_OK;
}

int dr_accum_moments_device_ptr(dr_context* c, void** dev_ptr, uint64_t* bytes) {
  if (!c || !dev_ptr || !c->accum) { set_error("no accumulator"); return DR_ERR_INVALID; }
  HIP_TRY(hipSetDevice(c->device));
  DR_TRY(join_pipeline(c));      // as dr_accum_device_ptr
  *dev_ptr = c->m2;
  if (bytes) *bytes = c->m2 ? (uint64_t)c->accW * c->accH * sizeof(uint64_t) : 0;
  return DR_OK;
}

int dr_accum_error(dr_context* c, const float settings13[13], int W, int H, int divide_by, float tolerance, float* out_sigma, dr_error_result* result,
                   int device_pointers) {
  if (!c || !settings13) { set_error("null argument"); return DR_ERR_INVALID; }
  RenderParams P;
  int traversal = 0;
  DR_TRY(aov_view(c, settings13, W, H, P, traversal));
  DR_TRY(accum_matches(c, "error", W, H));
  if (!c->m2) { set_error("error: no moments plane (set option moments = 1 before dr_accum_reset)"); return DR_ERR_INVALID; }
  if (divide_by < 0) { set_error("error: divide_by must be >= 0"); return DR_ERR_INVALID; }
  if (!(tolerance >= 0.0f)) { set_error("error: tolerance must be >= 0"); return DR_ERR_INVALID; }
  if (!out_sigma && !result) { set_error("error: no output (both out_sigma and result are NULL)"); return DR_ERR_INVALID; }
  DR_TRY(join_pipeline(c));      // ordered behind the frames submitted before

  const size_t npix = (size_t)W * (size_t)H;
  MoLaunch L;
  memset(&L, 0, sizeof(L));
  L.gw = P.gx * 8; L.gh = P.gy * 8; L.W = W; L.H = H; L.divide_by = divide_by; L.tolerance = tolerance;
  L.acc = c->accum; L.hist = c->hist; L.m2 = c->m2;
  float* sigma_dev = out_sigma;
  if (out_sigma && !device_pointers) {
    DR_TRY(c->err_staging.grow(npix, c->stream));
    sigma_dev = c->err_staging;
  }
  L.out_sigma = sigma_dev;
  if (sigma_dev && (L.gw < W || L.gh < H)) HIP_TRY(hipMemsetAsync(sigma_dev, 0, npix * sizeof(float), c->stream));      // pixels outside the grid are 0
  if (result) {
    DR_TRY(c->err_counts.grow(MO_WORDS, c->stream));
    HIP_TRY(hipMemsetAsync(c->err_counts, 0, MO_WORDS * sizeof(unsigned long long), c->stream));
    L.counts = c->err_counts;
  }
  launch_moments_error(c->stream, L);
  HIP_TRY(hipGetLastError());
  unsigned long long counts[MO_WORDS] = {0};
  if (result) HIP_TRY(hipMemcpyAsync(counts, c->err_counts, sizeof(counts), hipMemcpyDeviceToHost, c->stream));
  if (out_sigma && !device_pointers) HIP_TRY(hipMemcpyAsync(out_sigma, sigma_dev, npix * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  if (result || !device_pointers) HIP_TRY(hipStreamSynchronize(c->stream));
  if (result) {
    result->pixels = (int64_t)L.gw * (int64_t)L.gh;
    result->estimated = (int64_t)counts[MO_ESTIMATED]; result->above = (int64_t)counts[MO_ABOVE]; result->sum_var_q16 = counts[MO_SUM_VAR];
    for (int k = 0; k < MO_BINS; k++) result->bins[k] = (int64_t)counts[MO_BIN0 + k];
  }
  return DR_OK;
}

int dr_accum_present(dr_context* c, int divide_by, uint8_t* out_rgb8) {
  if (!c || !out_rgb8 || !c->accum || divide_by == 0) { set_error("bad argument"); return DR_ERR_INVALID; }
  HIP_TRY(hipSetDevice(c->device));
  DR_TRY(join_pipeline(c));
  size_t bytes = (size_t)c->accW * c->accH * 3;
  DR_TRY(c->present.grow(bytes, c->stream));
  launch_present(c->stream, c->accum, c->hist, c->present, c->accW, c->accH, divide_by);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out_rgb8, c->present, bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return DR_OK;
}

int dr_accum_device_ptr(dr_context* c, void** dev_ptr, uint64_t* bytes) {
  if (!c || !dev_ptr || !c->accum) { set_error("no accumulator"); return DR_ERR_INVALID; }
  // the caller orders its own work on dr_context_stream(): the frames submitted before are launched, and that stream waits for their adds
  HIP_TRY(hipSetDevice(c->device));
  DR_TRY(join_pipeline(c));
  *dev_ptr = c->accum;
  if (bytes) *bytes = (uint64_t)c->accW * c->accH * 3 * sizeof(int32_t);
  return DR_OK;
}

}  // extern "C"
