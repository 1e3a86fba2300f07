// Render launches: settings13 -> per-launch constants, the three caches of launch_state.hpp (tile order, tile words, sky split) around a launch of the persistent or the
// per-tile kernel, and the calls that render on the context's own stream (dr_render_frame, dr_render_accumulate, dr_render_accumulate_async,
// dr_context_synchronize).  Replaces CudaStarter (kernel.cu K:2562-2669), which mallocs, uploads the whole scene, launches, synchronises,
// downloads and frees on every call.
#include "context.hpp"

namespace dr {

void fill_scene(const dr_context* c, RenderParams& P) {
  P.walk = c->walk; P.walk_bytes = (uint32_t)c->walk_bytes; P.pairs = c->pairs; P.prims = c->prims; P.shade = c->shade; P.tex = c->tex; P.texels = c->texels;
  P.wide = c->wide; P.wide_bytes = (uint32_t)c->wide_bytes; P.wide_pmax = c->wide_pmax; P.wide_mu = c->wide_mu;
}

// option coop_tiles_per_wave as a launch at `site` counts it
static int tiles_per_wave(const dr_context* c, const LaunchSite& site) {
  // (pipe_lean: the lean six-wave build and one queue per XCD, as for long launches -- the tail it leaves runs beside the next frames)
  return site.lean ? 0 : c->coop_tiles_per_wave;
}

// settings[13] -> per-launch constants: the view (params_host.hpp: the camera block K:1016-1052, evaluated once on the host), the
// resident scene, and the scheduling options.
int make_params(dr_context* c, const LaunchSite& site, const float* st, int W, int H, float background, uint64_t seed, RenderParams& P, int batch_hint) {
  if (!c->walk) { set_error("no scene uploaded"); return DR_ERR_INVALID; }
  memset(&P, 0, sizeof(P));
  if (const char* why = fill_view_params(st, W, H, background, seed, c->stripe_mod, c->stripe_rem, P)) { set_error(why); return DR_ERR_INVALID; }
  if (P.backtex >= c->n_tex) { set_error("backtex refers to a texture that is not loaded"); return DR_ERR_INVALID; }
  memcpy(c->cur_settings, st, sizeof(c->cur_settings));
  fill_scene(c, P);
  P.counters = c->counters;
  P.wave_log = c->wave_log_on ? c->wave_log.p : nullptr;
  P.coop_steps = c->coop_steps; P.coop_rounds = c->coop_rounds; P.split_parts = c->split_parts;
  P.coop_lanes = c->coop_lanes;
  const int tiles = P.ncols * P.gy;
  P.regions = plan_regions(tiles, batch_hint, c->xcd_regions != 0, c->short_one_queue != 0, tiles_per_wave(c, site), c->num_cus);
  for (int r = 0; r <= MAX_REGIONS; r++) P.region_start[r] = r <= P.regions ? (int)(((long long)tiles * r + P.regions - 1) / P.regions) : tiles;
  return DR_OK;
}

PersistentCfg persistent_cfg(const dr_context* c, const LaunchSite& site) {
  PersistentCfg cfg;
  cfg.traversal = traversal_of(c); cfg.occupancy = c->occupancy; cfg.schedule = c->schedule;
  cfg.num_cus = c->num_cus - c->reserve_cus > 0 ? c->num_cus - c->reserve_cus : 1; cfg.coop_tiles_per_wave = tiles_per_wave(c, site); cfg.count = c->count != 0;
  return cfg;
}

ViewKey view_key(const dr_context* c, const RenderParams& P) {
  ViewKey k;
  memcpy(k.st, c->cur_settings, sizeof(k.st));
  k.W = P.W; k.H = P.H; k.stripe_mod = P.stripe_mod; k.stripe_rem = P.stripe_rem; k.ncols = P.ncols; k.gy = P.gy; k.regions = P.regions;
  k.scene_gen = c->scene_gen;
  k.cert_factor = c->cert_factor; k.cert_levels = c->cert_levels; k.camera_entry = c->camera_entry; k.camera_cert = c->camera_cert;
  return k;
}

namespace {

// The cost feedback of a launch (launch_state.hpp order_begin): the order its queues hold (or null) and the per-pixel cost buffer it fills (or null)
OrderUse feedback_buffers(dr_context* c, const LaunchSite& site, const ViewKey& key, int tiles, const int*& order, unsigned*& pcost) {
  OrderUse use = order_begin(c->order.state, key, tiles, c->feedback != 0, c->order_follows_camera != 0, site.hold_order);
  if (use.grow && c->order.grow(site.stream) != DR_OK) use = {false, false, false};
  order = use.use_order ? c->order.order.p : nullptr;
  pcost = use.record_costs ? c->order.pixel_cost.p : nullptr;
  return use;
}

// The camera rays' grazing certificate of the launch's view and their entry table: what launch_state.hpp camera_words_plan says -- the
// cached tile words are reused, or computed on the site's stream.  The two are independent -- the certificate needs a tree with own bounds (option
// camera_cert), the table any wide tree (option camera_entry) -- and share the view, the key and the word per tile that the kernel reads.
// Without either P keeps cert_level = null and wide_cert_k = 1: every ray carries the scene's margin and starts at the root, as before.
void cert_prepare(dr_context* c, const LaunchSite& site, const ViewKey& key, RenderParams& P, int tiles) {
  P.cert_level = nullptr;
  for (float& k : P.wide_cert_k) k = 1.0f;
  CameraWords& w = c->words;
  const bool want_cert = c->camera_cert && c->wide_own_bounds > 0 && c->wide_mu.e > 0.0f;
  const bool want_entry = c->camera_entry && c->wide_leaf_rec && c->wide_range && c->wide_leaves > 0;
  const CameraWordsPlan plan = camera_words_plan(w.state, key, want_cert, want_entry, traversal_of(c) == DR_TRAVERSAL_WIDE && c->wide, tiles, site.hold_order, P.batch);
  if (plan != WORDS_REUSE && plan != WORDS_COMPUTE) return;
  if (plan == WORDS_COMPUTE) {
    const double a_star = 1e-4 * (double)c->cert_factor;
    CertView cv;
    bool cert_ok = false, entry_ok = false;
    camera_words_begin(w.state);
    // (the table asks nothing of the view's E: a scene without own bounds passes any)
    if (fill_cert_view(P, a_star, want_cert ? c->wide_mu.e : 1.0f, cv)) {
      if (w.grow(tiles, want_entry, site.stream) != DR_OK) return;
      for (float& k : w.state.k) k = 1.0f;
      if (want_cert) {
        cert_ladder(c->cert_factor, c->cert_levels != 0, cv);
        if (w.grow_mask(tiles, cv.n_levels, site.stream) != DR_OK) return;
        launch_cert_mask(site.stream, c->prims, c->n_prims, cv, w.mask, w.level, tiles);
        for (int g = 1; g <= CERT_MAX_LEVELS; g++) w.state.k[g] = g <= cv.n_levels ? cert_factor_k(cv.level_a[g - 1]) : 1.0f;
      } else {
        (void)hipMemsetAsync(w.level, 0, cert_level_words(tiles) * sizeof(uint32_t), site.stream);      // no certificate: grade 0, the scene's margin
      }
      // the tiles' words for the kernel: the grades, and the camera rays' entry records (no table: the root everywhere)
      launch_camera_entry(site.stream, c->wide, c->wide_leaf_rec, c->wide_range, c->wide_leaves, cv, want_entry ? w.mm.p : nullptr, w.level, w.word, tiles);
      cert_ok = want_cert; entry_ok = want_entry;
    }
    camera_words_commit(w.state, key, tiles, cert_ok, entry_ok);
  }
  if (camera_words_in_use(w.state)) { P.cert_level = w.word; memcpy(P.wide_cert_k, w.state.k, sizeof(P.wide_cert_k)); }
}

// Sky tiles (option sky_tiles): when the launch runs the lean build over a view with an entry table, the tiles no leaf can be seen from
// are rendered by sky_tiles_kernel, in front of the persistent kernel on the same stream, and order / region_start become the launch's own pair
// that holds the other tiles only (kept from launch to launch while the tiles' words and the order are the same).  The plan is still made from every tile (the number of geometry tiles stays on the device).  A pipelined launch
// beside others is not split, nor one on another stream than the context's (the launch's own pair is one per context).
// sky_tiles = 2: no kernel in front -- the list, the counts and the launch's unit cursor (`cursor`: zero when the launch starts) travel in P and the
// persistent kernel's waves render the sky tiles when they retire, a unit of SKY_CHUNK frames at a time.  Only a launch that adds atomically
// (P.accumulate == 2) may cut a tile's batch into several units; every other launch is of one frame, one unit per tile.
bool sky_split(dr_context* c, const LaunchSite& site, RenderParams& P, int tiles, const int*& order, const int*& region_start, unsigned* pcost, unsigned* cursor) {
  if (!c->sky_tiles || !c->words.state.entry_ok || !P.cert_level || site.hold_order || site.stream != c->stream || P.out_frame_stride != 0) return false;
  if (P.max_depth <= 0 || !(P.spp_f > 0.0f)) return false;
  if (!plan_sky_split(plan_persistent(persistent_cfg(c, site), (long long)tiles * P.batch, P.coop_steps, false, P.wave_log != nullptr))) return false;
  // the split of the same words and the same order is the same arrays: made once, on this stream, and reused by the launches behind it (every launch
  // that splits runs on this stream, so none reads the arrays while they are rewritten)
  SkySplit& sky = c->sky;
  const SkyKey key = sky_key(c->words.state, c->order.state, order != nullptr, tiles, P.regions);
  if (!sky_split_reusable(sky.state, key, sky.room(tiles))) {
    if (sky.grow(tiles, site.stream) != DR_OK) return false;
    launch_order_split(site.stream, SPLIT_BY_WORD, order, region_start, P.region_start, P.cert_level, tiles, P.regions, sky.pair.order, sky.pair.region_start, sky.list,
                       sky.counts);
    sky_split_commit(sky.state, key);
  }
  if (c->sky_tiles == 2) {
    P.sky_list = sky.list; P.sky_counts = sky.counts; P.sky_cursor = cursor;
    P.sky_chunk = sky_chunk_frames(P.batch, P.accumulate == 2 ? SKY_CHUNK : 0);
  } else launch_sky_tiles(site.stream, P, sky.list, sky.counts, pcost);
  order = sky.pair.order; region_start = sky.pair.region_start;
  return true;
}

// A launch over the site's tile subset (dr_render_adaptive): order / region_start become the subset's own pair, split on the launch's stream from the
// order this launch would have used and the subset's flags.  Made for every such launch -- a pass's groups may differ in their queues -- and read
// behind it by the fold (launch_adaptive_add), on the same stream.
void subset_split(const LaunchSite& site, const RenderParams& P, int tiles, const int*& order, const int*& region_start) {
  TileSubset& sub = *site.subset;
  launch_order_split(site.stream, SPLIT_BY_FLAG, order, region_start, P.region_start, sub.flags, tiles, P.regions, sub.pair.order, sub.pair.region_start, nullptr, nullptr);
  order = sub.pair.order; region_start = sub.pair.region_start;
}

}  // namespace

// enqueue one launch (P.batch frames) at `site_in`; no events, no sync
int enqueue_frame(dr_context* c, const LaunchSite& site_in, const RenderParams& P_in) {
  RenderParams P = P_in;
  const int tiles = P.ncols * P.gy;
  P.sample_magic = sample_order_magic(c->sample_order, P.batch);      // every launch comes through here with its batch set (dr_render_accumulate, the pipeline's groups)
  // (a held launch runs beside the previous frame's: it may read the tile order but nobody may write it, or the costs, meanwhile; a launch over a
  // tile subset is held too -- its costs would be a part of the view's: launch_state.hpp site_use)
  const SiteUse su = site_use(site_in.hold_order, site_in.subset != nullptr);
  LaunchSite site = site_in;
  site.hold_order = su.hold;
  if (uses_persistent(c)) {
    const CursorTake take = cursor_take(c->tile_cursor, c->queue_cursor_stride, c->queue_cursor_skew);
    if (take.wrap) (void)hipMemsetAsync(c->tile_counters, 0, CURSOR_RING_ALLOC * sizeof(unsigned), site.stream);
    unsigned* counter = c->tile_counters + take.block;      // a cursor per region, queue_cursor_stride words apart, and the sky units' cursor in the last slot
    c->tile_cursor = take.next;
    const ViewKey key = view_key(c, P);
    const int* order; unsigned* pcost;
    const OrderUse use = feedback_buffers(c, site, key, tiles, order, pcost);
    if (!c->wave_log_on) P.wave_log = nullptr;
    cert_prepare(c, site, key, P, tiles);
    const int* launch_order = order; const int* launch_rstart = c->order.region_start;      // what the persistent kernel's queues hold: the order, or the split's part of it
    c->sky.state.last = su.sky_split && sky_split(c, site, P, tiles, launch_order, launch_rstart, pcost, counter + cursor_sky_slot(c->queue_cursor_stride));
    if (su.subset_pair) subset_split(site, P, tiles, launch_order, launch_rstart);
    const int log_waves = launch_persistent_kernel(site.stream, P, persistent_cfg(c, site), counter, c->queue_cursor_stride, launch_order, launch_rstart, pcost);
    if (log_waves < 0) { set_error("the persistent kernel has no build for this launch (launch_plan.hpp)"); return DR_ERR_DEVICE; }
    c->wave_log_waves = log_waves;
    // next launch's order from this launch's costs (stream-ordered, no host sync), when launch_state.hpp order_end says so
    if (order_end(c->order.state, use, c->feedback_every)) {
      const int split_limit = plan_split_limit(c->num_cus, c->occupancy, c->split_parts, c->split_waves);
      launch_tile_feedback(site.stream, c->order.pixel_cost, c->order.tile_cost, c->order.order, c->order.region_start, tiles, P.regions, c->heavy_factor, c->split_steps, split_limit);
      const int args[5] = {tiles, P.regions, c->heavy_factor, c->split_steps, split_limit};
      memcpy(c->order.state.args, args, sizeof(args));
    }
    return DR_OK;
  }
  c->sky.state.last = false;
  launch_tile_kernel(site.stream, P, traversal_of(c), c->count != 0, c->occupancy);
  return DR_OK;
}

}  // namespace dr

using namespace dr;

namespace {

int launch_render(dr_context* c, const RenderParams& P) {
  int tiles = P.ncols * P.gy;
  if (tiles <= 0) return DR_OK;
  HIP_TRY(hipEventRecord(c->ev0, c->stream));
  DR_TRY(enqueue_frame(c, c->own_site(), P));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(c->ev1, c->stream));
  return DR_OK;
}

// waits for e1 and adds the time since e0, the frames and the samples to the statistics
int collect_time(dr_context* c, hipEvent_t e0, hipEvent_t e1, uint64_t frames, uint64_t samples) {
  HIP_TRY(hipEventSynchronize(e1));
  float ms = 0;
  HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
  c->stats.kernel_ms += ms;
  c->stats.frames += frames;
  c->stats.samples += samples;
  return DR_OK;
}

// time of an asynchronous batch whose events are still outstanding (waits for that batch, not for later ones)
int collect_pending(dr_context* c, int k) {
  return c->async.collect(k, [c](hipEvent_t e0, hipEvent_t e1, uint64_t frames, uint64_t samples) { return collect_time(c, e0, e1, frames, samples); });
}

// enqueues the launches of `nframes` frames between two event records; no host synchronisation
int accumulate_enqueue(dr_context* c, const float settings13[13], int W, int H, float background, uint64_t frame_seed,
                       uint64_t seed_stride, int nframes, hipEvent_t e0, hipEvent_t e1, uint64_t& samples) {
  samples = 0;
  if (!c || !settings13 || nframes < 0) { set_error("bad argument"); return DR_ERR_INVALID; }
  if (!c->accum || c->accW != W || c->accH != H) { set_error("call dr_accum_reset(W, H) first"); return DR_ERR_INVALID; }
  HIP_TRY(hipSetDevice(c->device));
  DR_TRY(join_pipeline(c));
  RenderParams P;
  // The persistent kernel renders the frames in batches of `batch_frames` per launch (one work
  // queue over all their tiles, atomic accumulation); the per-tile kernel takes one frame per launch.
  const int per_launch = (uses_persistent(c) && c->batch_frames > 1) ? c->batch_frames : 1;
  DR_TRY(make_params(c, c->own_site(), settings13, W, H, background, frame_seed, P, nframes < per_launch ? nframes : per_launch));
  if (c->traversal == DR_TRAVERSAL_ORDERED && c->tree_depth > ORDERED_STACK) { set_error("tree too deep for ordered traversal"); return DR_ERR_SCENE; }
  P.out = c->accum;
  P.accumulate = 1;
  int tiles = P.ncols * P.gy;
  HIP_TRY(hipEventRecord(e0, c->stream));
  uint64_t launches = 0;
  for (int k = 0; k < nframes && tiles > 0; k += per_launch) {
    P.seed = frame_seed + (uint64_t)k * seed_stride;
    P.batch = nframes - k < per_launch ? nframes - k : per_launch;
    P.batch_seed_stride = seed_stride;
    P.accumulate = P.batch > 1 ? 2 : 1;
    DR_TRY(enqueue_frame(c, c->own_site(), P));
    launches++;
  }
  c->stats.launches += launches;
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(e1, c->stream));
  samples = (uint64_t)(tiles > 0 ? tiles : 0) * 64ull * (uint64_t)(P.spp_f > 0 ? ceilf(P.spp_f) : 0) * (uint64_t)nframes;
  return DR_OK;
}

}  // namespace

extern "C" {

int dr_render_frame(dr_context* c, const float settings13[13], int W, int H, float background, uint64_t frame_seed,
                    int32_t* out_int3) {
  if (!c || !settings13) { set_error("null argument"); return DR_ERR_INVALID; }
  HIP_TRY(hipSetDevice(c->device));
  DR_TRY(join_pipeline(c));
  RenderParams P;
  DR_TRY(make_params(c, c->own_site(), settings13, W, H, background, frame_seed, P));
  if (c->traversal == DR_TRAVERSAL_ORDERED && c->tree_depth > ORDERED_STACK) { set_error("tree too deep for ordered traversal"); return DR_ERR_SCENE; }
  size_t elems = (size_t)W * H * 3;
  DR_TRY(c->frame.grow(elems, c->stream));
  HIP_TRY(hipMemsetAsync(c->frame, 0, elems * sizeof(int32_t), c->stream));   // unrendered margins are 0
  P.out = c->frame;
  P.accumulate = 0;
  DR_TRY(launch_render(c, P));
  c->stats.launches += 1;
  uint64_t samples = (uint64_t)P.ncols * P.gy * 64ull * (uint64_t)(P.spp_f > 0 ? ceilf(P.spp_f) : 0);
  DR_TRY(collect_time(c, c->ev0, c->ev1, 1, samples));
  if (out_int3) {
    HIP_TRY(hipMemcpyAsync(out_int3, c->frame, elems * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  return DR_OK;
}

int dr_render_accumulate(dr_context* c, const float settings13[13], int W, int H, float background, uint64_t frame_seed,
                         uint64_t seed_stride, int nframes) {
  if (!c) { set_error("bad argument"); return DR_ERR_INVALID; }
  if (nframes == 0) return DR_OK;
  // a second-moment plane needs every frame in a buffer of its own: the same sums through the pipeline, whose add squares the frame as well
  if (c->m2) return dr_render_accumulate_pipelined(c, settings13, W, H, background, frame_seed, seed_stride, nframes);
  uint64_t samples = 0;
  DR_TRY(accumulate_enqueue(c, settings13, W, H, background, frame_seed, seed_stride, nframes, c->ev0, c->ev1, samples));
  DR_TRY(collect_time(c, c->ev0, c->ev1, (uint64_t)nframes, samples));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return DR_OK;
}

int dr_render_accumulate_async(dr_context* c, const float settings13[13], int W, int H, float background, uint64_t frame_seed,
                               uint64_t seed_stride, int nframes) {
  if (!c) { set_error("bad argument"); return DR_ERR_INVALID; }
  if (nframes == 0) return DR_OK;
  if (c->m2) { set_error("dr_render_accumulate_async cannot feed a second-moment plane (option moments): use dr_render_accumulate or the pipeline"); return DR_ERR_INVALID; }
  const int k = c->async.older();
  DR_TRY(collect_pending(c, k));           // at most two batches in flight: reusing a pair of events waits for the batch before last
  uint64_t samples = 0;
  DR_TRY(accumulate_enqueue(c, settings13, W, H, background, frame_seed, seed_stride, nframes, c->async.batch[k].ev0, c->async.batch[k].ev1, samples));
  c->async.started((uint64_t)nframes, samples);
  return DR_OK;
}

int dr_context_synchronize(dr_context* c) {
  if (!c) { set_error("null context"); return DR_ERR_INVALID; }
  HIP_TRY(hipSetDevice(c->device));
  DR_TRY(join_pipeline(c));
  DR_TRY(collect_pending(c, c->async.older()));
  DR_TRY(collect_pending(c, c->async.newer()));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return DR_OK;
}

}  // extern "C"
