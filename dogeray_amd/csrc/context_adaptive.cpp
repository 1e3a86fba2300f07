// Adaptive sampling (dr_render_adaptive): one pass -- the selection of the tiles that ask for samples, launches of the persistent
// kernel over those tiles only (LaunchSite's subset: context_render.cpp splits the launch's order by the flags), and the fold of the frames into the
// planes of those tiles.  Everything runs on the context's own stream, one step behind the other; the host waits once, for the counts.  The
// call is judged by params_host.hpp's judge_adaptive, which the host build runs too; the owner of the pass's buffers is context.hpp's TileSubset.
#include "context.hpp"

using namespace dr;

extern "C" {

int dr_adaptive_defaults(dr_adaptive_params* p) {
  if (!p) { set_error("null argument"); return DR_ERR_INVALID; }
  p->tolerance = AD_DEFAULTS.tolerance; p->min_samples = AD_DEFAULTS.min_samples; p->max_samples = AD_DEFAULTS.max_samples; p->tile_pixels = AD_DEFAULTS.tile_pixels;
  return DR_OK;
}

int dr_render_adaptive(dr_context* c, const float settings13[13], int W, int H, float background, uint64_t frame_seed, uint64_t seed_stride, int nframes,
                       int divide_by, const dr_adaptive_params* params, dr_adaptive_result* result) {
  if (!c || !settings13) { set_error("null argument"); return DR_ERR_INVALID; }
  HIP_TRY(hipSetDevice(c->device));
  // what the context refuses, before anything is touched
  if (!c->walk) { set_error("no scene uploaded"); return DR_ERR_INVALID; }
  if (!c->accum || c->accW != W || c->accH != H) { set_error("adaptive: call dr_accum_reset(W, H) first"); return DR_ERR_INVALID; }
  if (!c->m2) { set_error("adaptive: no moments plane (set option moments = 1 before dr_accum_reset)"); return DR_ERR_INVALID; }
  if (c->stripe_mod != 1) { set_error("adaptive: a stripe is set (dr_context_set_stripe): the pass renders whole frames' tiles"); return DR_ERR_INVALID; }
  if (!uses_persistent(c)) { set_error("adaptive: the pass needs the persistent kernel's tile queues (option kernel, ordered traversal)"); return DR_ERR_INVALID; }
  DR_TRY(join_pipeline(c));      // ordered behind the frames submitted before: the selection reads the planes as they are then
  LaunchSite site = c->own_site();
  site.subset = &c->adaptive;
  RenderParams P;
  DR_TRY(make_params(c, site, settings13, W, H, background, frame_seed, P, 1));
  AdLaunch L;
  const std::string why = judge_adaptive(P, nframes, divide_by, params, L);
  if (!why.empty()) { set_error(why); return DR_ERR_INVALID; }
  const int tiles = P.ncols * P.gy;
  if (result) memset(result, 0, sizeof(*result));
  if (tiles <= 0) { c->adaptive.invalidate(); return DR_OK; }

  const size_t npix = (size_t)W * H, elems = npix * 3;
  const int room = pipeline_group_room(c);      // frames per launch: the pipeline's rule for its groups
  TileSubset& sub = c->adaptive;
  DR_TRY(sub.grow(tiles, elems, nframes < room ? nframes : room, c->stream));
  if (!c->hist) {                // no history plane yet: one of zeros, the first of the reprojection's pair (dr_accum_reset drops it as it drops theirs)
    DR_TRY(c->hist_buf[0].grow(npix, c->stream));
    HIP_TRY(hipMemsetAsync(c->hist_buf[0], 0, npix * sizeof(int32_t), c->stream));
    c->hist = c->hist_buf[0]; c->hist_cur = 0;
  }
  // the selection: one for all launches of the pass
  L.acc = c->accum; L.hist = c->hist; L.m2 = c->m2; L.flags = sub.flags; L.counts = sub.counts;
  HIP_TRY(hipMemsetAsync(sub.counts, 0, AD_WORDS * sizeof(unsigned), c->stream));
  launch_adaptive_select(c->stream, L);
  HIP_TRY(hipGetLastError());
  sub.tiles = tiles;
  // the frames, in groups as the pipeline forms them, each into the owner's buffers (the tiles a launch skips are never read: nothing is cleared)
  // and folded behind its launch
  L.frames = sub.frames; L.frame_stride = elems;
  uint64_t launches = 0;
  for (int k = 0; k < nframes; k += room) {
    const int n = nframes - k < room ? nframes - k : room;
    DR_TRY(make_params(c, site, settings13, W, H, background, frame_seed + (uint64_t)k * seed_stride, P, n));
    P.out = sub.frames;
    P.accumulate = 0;
    P.batch = n; P.batch_seed_stride = seed_stride;
    P.out_frame_stride = n > 1 ? (uint32_t)elems : 0u;      // (a group of one is an ordinary launch, as the pipeline's)
    DR_TRY(enqueue_frame(c, site, P));
    HIP_TRY(hipGetLastError());
    L.nframes = n;
    launch_adaptive_add(c->stream, L, sub.pair.order, sub.pair.region_start, P.regions);
    HIP_TRY(hipGetLastError());
    launches++;
  }
  unsigned counts[AD_WORDS] = {0};
  HIP_TRY(hipMemcpyAsync(counts, sub.counts, sizeof(counts), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->stats.launches += launches;
  c->stats.samples += (uint64_t)counts[AD_ACTIVE] * 64ull * (uint64_t)(P.spp_f > 0 ? ceilf(P.spp_f) : 0) * (uint64_t)nframes;
  if (result) {
    result->tiles = tiles; result->active_tiles = counts[AD_ACTIVE];
    result->pixels = (int64_t)tiles * 64; result->asking_pixels = counts[AD_ASKING];
    result->samples_added = (int64_t)counts[AD_ACTIVE] * 64 * nframes;
  }
  return DR_OK;
}

}  // extern "C"
