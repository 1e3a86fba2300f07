// The accumulator and what is computed from it on the device: reset, first-hit AOVs, the denoiser, the upscaler, temporal reprojection, the noise
// estimate, present, the stripe copies of the multi-GPU gather, reads and device pointers.  A stage's entry checks what needs the context, has its
// call judged and its launch struct filled by params_host.hpp's judge_* (the host build runs the same judges), adds the pointers -- guides from a
// GuidePlanes set (context.hpp), host outputs staged as a query's channels (context_query.cpp) -- and launches.
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

// A launch_aov over the window (x0, y0, w, h) of a view's pixel grid, no channel wanted yet
AovLaunch aov_launch(const dr_context* c, float focus, int x0, int y0, int w, int h) {
  AovLaunch A;
  memset(&A, 0, sizeof(A));
  A.x0 = x0; A.y0 = y0; A.w = w; A.h = h;
  A.focus = focus;
  A.slot_to_orig = c->slot_to_orig_dev;
  return A;
}

// A launch_aov_lens over the window (x0, y0, w, h) of the view in P (as aov_view filled it), no channel wanted yet: nframes frames of the view's
// spp = (int)settings13[10] samples, frame k seeded frame_seed + k * seed_stride, N = nframes * spp in 1 .. AOV_LENS_MAX (`who` starts the refusal)
int aov_lens_launch(const float settings13[13], int x0, int y0, int w, int h, uint64_t frame_seed, uint64_t seed_stride, int nframes, const char* who,
                    RenderParams& P, AovLensLaunch& A) {
  const int spp = hf2i(settings13[10]);
  if (nframes < 1 || spp < 1 || (long long)nframes * spp > AOV_LENS_MAX) {
    set_error(std::string(who) + ": " + std::to_string(nframes) + " frames of " + std::to_string(spp) + " samples per pixel; a lens pass takes 1 .. " +
              std::to_string(AOV_LENS_MAX) + " samples");
    return DR_ERR_INVALID;
  }
  memset(&A, 0, sizeof(A));
  A.x0 = x0; A.y0 = y0; A.w = w; A.h = h;
  A.focus = settings13[7];
  A.nframes = nframes; A.spp = spp;
  P.seed = frame_seed; P.batch_seed_stride = seed_stride;
  return DR_OK;
}

// The guides of view P (of settings13) over its gw x gh > 0 pixel grid in G, a set of `quads` float4 planes: traced unless G holds them already
// (*passes then counts the pass).  launch_aov writes normal and depth into float4 plane 1 (3n + n floats), albedo and material into their planes;
// the guide prepare packs (n, z) into plane 0 and forms gz from them
int trace_guides(dr_context* c, GuidePlanes& G, int quads, const float settings13[13], int W, int H, const RenderParams& P, int traversal, int* passes) {
  const int gw = P.gx * 8, gh = P.gy * 8;
  DR_TRY(G.grow((size_t)gw * (size_t)gh, quads, c->stream));
  const int frames = c->guide_frames;
  if (G.key.matches(settings13, W, H, c->scene_gen, frames)) return DR_OK;
  AovLaunch A = aov_launch(c, settings13[7], 0, 0, gw, gh);
  A.normal = G.quad(1); A.depth = G.quad(1) + 3 * G.n; A.albedo = G.rgb(); A.material = G.material();
  if (frames > 0) {      // option guide_frames: the same planes from the renderer's own camera rays, averaged over `frames` frames of DR_GUIDE_SEED
    AovLensLaunch AL;
    RenderParams PL = P;
    DR_TRY(aov_lens_launch(settings13, 0, 0, gw, gh, DR_GUIDE_SEED, 1, frames, "guide_frames", PL, AL));
    AL.as_guides = 1;
    AL.normal = A.normal; AL.depth = A.depth; AL.albedo = A.albedo; AL.material = A.material;
    launch_aov_lens(c->stream, PL, traversal, c->aov_lens_loop, AL);
  } else launch_aov(c->stream, P, traversal, A);
  HIP_TRY(hipGetLastError());
  DnLaunch L;
  memset(&L, 0, sizeof(L));
  L.gw = gw; L.gh = gh;
  L.normal = A.normal; L.depth = A.depth; L.mat = A.material; L.guide = G.quad(0); L.gz = G.scalar();
  launch_denoise_guides(c->stream, L);
  HIP_TRY(hipGetLastError());
  G.key.store(settings13, W, H, c->scene_gen, frames);
  if (passes) ++*passes;
  return DR_OK;
}

// The low side of dr_accum_denoise and dr_accum_upscale over the pixel grid of settings13 (L as its judge filled it, L.gw x L.gh > 0, with the
// accumulator's planes L.acc, L.hist, L.m2): the planes (allocated by the first call; colour plane A doubles as the trace's scratch), the cached
// guides (*aov_passes counts a trace), colour stage 0 and -- filter -- the variance pre-pass and the L.D.iterations a-trous passes.  On return
// L.src is the plane of the result: (e, l) after stage 0, (e, var) after the last pass; L.guide, L.albedo, L.mat and L.gz are the guides.
int denoise_low_side(dr_context* c, const float settings13[13], const RenderParams& P, int traversal, DnLaunch& L, bool filter, int* aov_passes) {
  GuidePlanes& G = c->dn_guides;
  DR_TRY(trace_guides(c, G, 3, settings13, L.W, L.H, P, traversal, aov_passes));
  float* const pa = G.quad(1);
  float* const pb = G.quad(2);
  L.albedo = G.rgb(); L.mat = G.material(); L.guide = G.quad(0); L.gz = G.scalar();
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

// The W x H x 3 image a stage hands out as floats, as bytes or as both: the channels of query_begin / query_end (context_query.cpp) over the pixels
struct ImageOut {
  QueryOut ch[2];
  QueryIo io;
  ImageOut(float* out_f32, uint8_t* out_rgb8) : ch{{out_f32, 3, true}, {out_rgb8, 3, true, 1}} {}
  int begin(dr_context* c, int W, int H, int device_pointers) { return query_begin(c, (size_t)W * (size_t)H, 1, nullptr, 0, ch, 2, device_pointers != 0, io); }
  float* f32() const { return (float*)io.out[0]; }
  uint8_t* rgb8() const { return (uint8_t*)io.out[1]; }
  int end(dr_context* c, int device_pointers) { return query_end(c, ch, 2, device_pointers != 0, io); }
};

// One of the accumulator's planes (the sums, the history, the second moments) and its bytes per pixel
using PlaneOf = void* (*)(const dr_context*);
void* sums_of(const dr_context* c) { return c->accum; }
void* history_of(const dr_context* c) { return c->hist; }
void* moments_of(const dr_context* c) { return c->m2; }

// A plane read back behind the frames submitted before, or zeros where there is none (no history, no moments yet)
int plane_read(dr_context* c, void* out, PlaneOf plane_of, size_t bytes_per_pixel) {
  if (!c || !out || !c->accum) { set_error("no accumulator"); return DR_ERR_INVALID; }
  HIP_TRY(hipSetDevice(c->device));
  DR_TRY(join_pipeline(c));
  const void* const plane = plane_of(c);
  const size_t bytes = (size_t)c->accW * c->accH * bytes_per_pixel;
  if (!plane) { memset(out, 0, bytes); return DR_OK; }
  HIP_TRY(hipMemcpyAsync(out, plane, bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return DR_OK;
}

// A plane's device address (null: there is none) and size.  The caller orders its own work on dr_context_stream(): the frames submitted before are
// launched, and that stream waits for their adds
int plane_device_ptr(dr_context* c, void** dev_ptr, uint64_t* bytes, PlaneOf plane_of, size_t bytes_per_pixel) {
  if (!c || !dev_ptr || !c->accum) { set_error("no accumulator"); return DR_ERR_INVALID; }
  HIP_TRY(hipSetDevice(c->device));
  DR_TRY(join_pipeline(c));
  *dev_ptr = plane_of(c);
  if (bytes) *bytes = *dev_ptr ? (uint64_t)c->accW * c->accH * bytes_per_pixel : 0;
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
  // the channels: where the caller wants each, its words per pixel
  const QueryOut ch[9] = {{buffers->t, 1, true}, {buffers->distance, 1, true}, {buffers->depth, 1, true}, {buffers->object, 1, true}, {buffers->material, 1, true},
                          {buffers->normal, 3, true}, {buffers->uv, 2, true}, {buffers->albedo, 3, true}, {buffers->dir, 3, true}};
  bool any = false;
  for (int k = 0; k < 9; k++) any = any || ch[k].p;
  if (!any) return DR_OK;
  QueryIo io;
  DR_TRY(query_begin(c, (size_t)w * (size_t)h, 1, nullptr, 0, ch, 9, device_pointers != 0, io));
  AovLaunch A = aov_launch(c, settings13[7], x0, y0, w, h);
  A.t = (float*)io.out[0]; A.distance = (float*)io.out[1]; A.depth = (float*)io.out[2]; A.object = (int32_t*)io.out[3]; A.material = (int32_t*)io.out[4];
  A.normal = (float*)io.out[5]; A.uv = (float*)io.out[6]; A.albedo = (float*)io.out[7]; A.dir = (float*)io.out[8];
  launch_aov(c->stream, P, traversal, A);
  HIP_TRY(hipGetLastError());
  return query_end(c, ch, 9, device_pointers != 0, io);
}

int dr_render_aov_lens(dr_context* c, const float settings13[13], int W, int H, int x0, int y0, int w, int h, uint64_t frame_seed, uint64_t seed_stride,
                       int nframes, const dr_aov_lens_buffers* buffers, int device_pointers) {
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
  AovLensLaunch A;
  DR_TRY(aov_lens_launch(settings13, x0, y0, w, h, frame_seed, seed_stride, nframes, "render_aov_lens", P, A));
  DR_TRY(join_pipeline(c));      // ordered behind the frames submitted before
  const QueryOut ch[6] = {{buffers->coverage, 1, true}, {buffers->depth, 1, true}, {buffers->distance, 1, true}, {buffers->material, 1, true},
                          {buffers->normal, 3, true}, {buffers->albedo, 3, true}};
  bool any = false;
  for (int k = 0; k < 6; k++) any = any || ch[k].p;
  if (!any) return DR_OK;
  QueryIo io;
  DR_TRY(query_begin(c, (size_t)w * (size_t)h, 1, nullptr, 0, ch, 6, device_pointers != 0, io));
  A.coverage = (float*)io.out[0]; A.depth = (float*)io.out[1]; A.distance = (float*)io.out[2]; A.material = (int32_t*)io.out[3];
  A.normal = (float*)io.out[4]; A.albedo = (float*)io.out[5];
  launch_aov_lens(c->stream, P, traversal, c->aov_lens_loop, A);
  HIP_TRY(hipGetLastError());
  return query_end(c, ch, 6, device_pointers != 0, io);
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
  DnLaunch L;
  const std::string why = judge_denoise(P, divide_by, params, L);
  if (!why.empty()) { set_error(why); return DR_ERR_INVALID; }
  if (!out_f32 && !out_rgb8) { set_error("denoise: no output (both out_f32 and out_rgb8 are NULL)"); return DR_ERR_INVALID; }
  DR_TRY(join_pipeline(c));      // ordered behind the frames submitted before

  L.acc = c->accum; L.hist = c->hist;
  L.m2 = c->denoise_variance ? c->m2 : nullptr;
  if (L.D.iterations > 0 && L.gw > 0 && L.gh > 0) DR_TRY(denoise_low_side(c, settings13, P, traversal, L, true, nullptr));
  ImageOut out(out_f32, out_rgb8);
  DR_TRY(out.begin(c, W, H, device_pointers));
  L.out_f32 = out.f32(); L.out_rgb8 = out.rgb8();
  launch_denoise_finish(c->stream, L);
  HIP_TRY(hipGetLastError());
  return out.end(c, device_pointers);
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
  full_view13(settings13, full13);
  DR_TRY(aov_view(c, full13, W, H, PF, traversal));
  DR_TRY(accum_matches(c, "upscale", W, H));
  UpLaunch U;
  DnLaunch L;                                              // the low side: the denoiser's planes; without a prefilter only the demodulated colour of stage 0
  const std::string why = judge_upscale(P, PF, settings13, divide_by, params, prefilter, U, L);
  if (!why.empty()) { set_error(why); return DR_ERR_INVALID; }
  if (!out_f32 && !out_rgb8) { set_error("upscale: no output (both out_f32 and out_rgb8 are NULL)"); return DR_ERR_INVALID; }
  DR_TRY(join_pipeline(c));      // ordered behind the frames submitted before

  U.acc = c->accum; U.hist = c->hist;
  c->up_passes = 0;
  if (U.U.mode == UP_GUIDED && U.gw > 0 && U.gh > 0) {
    L.acc = c->accum; L.hist = c->hist;
    L.m2 = c->denoise_variance ? c->m2 : nullptr;
    DR_TRY(denoise_low_side(c, settings13, P, traversal, L, prefilter != nullptr, &c->up_passes));
    U.e = L.src; U.guide = L.guide; U.mat = L.mat;
    GuidePlanes& F = c->up_guides;                         // the full side: planes of its own, traced once per view
    DR_TRY(trace_guides(c, F, 2, full13, W, H, PF, traversal, &c->up_passes));
    U.Fguide = F.quad(0); U.Falbedo = F.rgb(); U.Fmat = F.material(); U.Fgz = F.scalar();
  }
  ImageOut out(out_f32, out_rgb8);
  DR_TRY(out.begin(c, W, H, device_pointers));
  U.out_f32 = out.f32(); U.out_rgb8 = out.rgb8();
  launch_upscale(c->stream, U);
  HIP_TRY(hipGetLastError());
  return out.end(c, device_pointers);
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
  if (const char* why = check_reproject_views(Pf, Pt)) { set_error(why); return DR_ERR_INVALID; }      // (the judge's first check, ahead of the context's)
  if (c->stripe_mod != 1 || c->stripe_rem != 0) { set_error("reproject: the context renders a stripe (dr_context_set_stripe); only (1, 0) is supported"); return DR_ERR_INVALID; }
  DR_TRY(accum_matches(c, "reproject", W, H));
  RpLaunch L;
  const std::string why = judge_reproject(Pf, Pt, frames, params, L);
  if (!why.empty()) { set_error(why); return DR_ERR_INVALID; }
  DR_TRY(join_pipeline(c));      // ordered behind the frames submitted before

  const int gw = L.gw, gh = L.gh;
  const size_t n = (size_t)gw * (size_t)gh, npix = (size_t)W * (size_t)H;
  DR_TRY(c->accum2.grow(npix * 3, c->stream));
  const int hto = c->hist ? 1 - c->hist_cur : 0;
  DR_TRY(c->hist_buf[hto].grow(npix, c->stream));
  const int mto = 1 - c->m2_cur;                               // (a second-moment plane is carried into the other buffer of its pair)
  if (c->m2) DR_TRY(c->m2_buf[mto].grow(npix, c->stream));
  DR_TRY(c->rp_counts.grow(4, c->stream));
  // the guides: the cached planes serve as `from` when their key matches; the `to` view is traced into the other set (into none when it is
  // the `from` view itself) and becomes the cache
  const bool warm = c->rp_guides[c->rp_cur].key.matches(from_settings13, W, H, c->scene_gen);
  const bool same_view = memcmp(from_settings13, to_settings13, 13 * sizeof(float)) == 0;
  const int sf = warm ? c->rp_cur : 0, st = same_view ? sf : 1 - sf;
  c->rp_guides[c->rp_cur].key.valid = false;
  c->rp_passes = 0;
  // (t, normal and material only, no float4 plane and no guide prepare: not trace_guides)
  auto trace = [&](GuidePlanes& G, const RenderParams& P, const float* st13) -> int {
    if (n == 0) return DR_OK;
    DR_TRY(G.grow(n, 0, c->stream));
    AovLaunch A = aov_launch(c, st13[7], 0, 0, gw, gh);
    A.t = G.scalar(); A.normal = G.rgb(); A.material = G.material();
    launch_aov(c->stream, P, traversal, A);
    HIP_TRY(hipGetLastError());
    c->rp_passes++;
    return DR_OK;
  };
  GuidePlanes &Gf = c->rp_guides[sf], &Gt = c->rp_guides[st];
  if (!warm) DR_TRY(trace(Gf, Pf, from_settings13));
  if (!same_view) DR_TRY(trace(Gt, Pt, to_settings13));
  if (n > 0) {
    L.t_from = Gf.scalar(); L.normal_from = Gf.rgb(); L.mat_from = Gf.material();
    L.t_to = Gt.scalar(); L.normal_to = Gt.rgb(); L.mat_to = Gt.material();
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
  Gt.key.store(to_settings13, W, H, c->scene_gen);
  c->rp_cur = st; Gt.key.valid = n > 0;
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
  return plane_read(c, out_int3, sums_of, 3 * sizeof(int32_t));
}
int dr_accum_history_read(dr_context* c, int32_t* out) {
  return plane_read(c, out, history_of, sizeof(int32_t));
}
int dr_accum_moments_read(dr_context* c, uint64_t* out) {
  return plane_read(c, out, moments_of, sizeof(uint64_t));
}

int dr_accum_device_ptr(dr_context* c, void** dev_ptr, uint64_t* bytes) {
  return plane_device_ptr(c, dev_ptr, bytes, sums_of, 3 * sizeof(int32_t));
}
int dr_accum_history_device_ptr(dr_context* c, void** dev_ptr, uint64_t* bytes) {
  return plane_device_ptr(c, dev_ptr, bytes, history_of, sizeof(int32_t));
}
int dr_accum_moments_device_ptr(dr_context* c, void** dev_ptr, uint64_t* bytes) {
  return plane_device_ptr(c, dev_ptr, bytes, moments_of, sizeof(uint64_t));
}

int dr_accum_error(dr_context* c, const float settings13[13], int W, int H, int divide_by, float tolerance, float* out_sigma, dr_error_result* result,
                   int device_pointers) {
  if (!c || !settings13) { set_error("null argument"); return DR_ERR_INVALID; }
  RenderParams P;
  int traversal = 0;
  DR_TRY(aov_view(c, settings13, W, H, P, traversal));
  DR_TRY(accum_matches(c, "error", W, H));
  if (!c->m2) { set_error("error: no moments plane (set option moments = 1 before dr_accum_reset)"); return DR_ERR_INVALID; }
  MoLaunch L;
  const std::string why = judge_error(P, divide_by, tolerance, L);
  if (!why.empty()) { set_error(why); return DR_ERR_INVALID; }
  if (!out_sigma && !result) { set_error("error: no output (both out_sigma and result are NULL)"); return DR_ERR_INVALID; }
  DR_TRY(join_pipeline(c));      // ordered behind the frames submitted before

  L.acc = c->accum; L.hist = c->hist; L.m2 = c->m2;
  const QueryOut ch[1] = {{out_sigma, 1, true}};
  QueryIo io;
  DR_TRY(query_begin(c, (size_t)W * (size_t)H, 1, nullptr, 0, ch, 1, device_pointers != 0, io));
  L.out_sigma = (float*)io.out[0];
  if (L.out_sigma && (L.gw < W || L.gh < H)) HIP_TRY(hipMemsetAsync(L.out_sigma, 0, io.out_bytes[0], c->stream));      // pixels outside the grid are 0
  if (result) {
    DR_TRY(c->err_counts.grow(MO_WORDS, c->stream));
    HIP_TRY(hipMemsetAsync(c->err_counts, 0, MO_WORDS * sizeof(unsigned long long), c->stream));
    L.counts = c->err_counts;
  }
  launch_moments_error(c->stream, L);
  HIP_TRY(hipGetLastError());
  unsigned long long counts[MO_WORDS] = {0};
  if (result) HIP_TRY(hipMemcpyAsync(counts, c->err_counts, sizeof(counts), hipMemcpyDeviceToHost, c->stream));
  DR_TRY(query_end(c, ch, 1, device_pointers != 0, io));
  if (result && device_pointers) HIP_TRY(hipStreamSynchronize(c->stream));      // (the counts are read even when the plane stays on the device)
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
  const QueryOut ch[1] = {{out_rgb8, 3, true, 1}};
  QueryIo io;
  DR_TRY(query_begin(c, (size_t)c->accW * c->accH, 1, nullptr, 0, ch, 1, false, io));
  launch_present(c->stream, c->accum, c->hist, (uint8_t*)io.out[0], c->accW, c->accH, divide_by);
  HIP_TRY(hipGetLastError());
  return query_end(c, ch, 1, false, io);
}

}  // extern "C"
