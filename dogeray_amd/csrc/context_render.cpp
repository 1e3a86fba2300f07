// Render launches: settings13 -> per-launch constants, the cost feedback and the grazing certificate around a launch of the persistent or the
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

namespace {

// Cost-feedback buffers for `tiles` tiles; returns the order to use for this launch (or null)
// and the per-pixel cost buffer to fill (or null).
void feedback_buffers(dr_context* c, const LaunchSite& site, const RenderParams& P, int tiles, const int*& order, unsigned*& pcost) {
  order = nullptr; pcost = nullptr;
  if (!c->feedback) return;
  if (c->order_capacity < tiles) {
    c->order_capacity = 0; c->order_valid = false;
    if (c->pixel_cost.grow((size_t)tiles * 64, site.stream) != DR_OK || c->tile_cost.grow((size_t)tiles, site.stream) != DR_OK ||
        c->region_start.grow(2 * MAX_REGIONS + 1, site.stream) != DR_OK || c->tile_order.grow((size_t)tiles, site.stream) != DR_OK)
      return;
    c->order_capacity = tiles;
  }
  // the stored order belongs to one view: same settings, size and stripe (progressive frames)
  float key[18] = {0};
  memcpy(key, c->cur_settings, 13 * sizeof(float));
  order_geometry(P, key + 13);
  if (c->order_valid && memcmp(c->order_key, key, sizeof(key)) == 0) order = c->tile_order;
  else if (c->order_valid && c->order_follows_camera && memcmp(c->order_key + 13, key + 13, 5 * sizeof(float)) == 0) {
    // same frame geometry, other camera / depth / samples (an interactive viewer moving the camera, K:2341-2500: every frame is a new
    // view): the last view's costs are a better guess than none -- any order is a valid order -- and they are refreshed at once
    order = c->tile_order;
    memcpy(c->order_key, key, sizeof(key));
    c->order_age = 0;
  } else { memcpy(c->order_key, key, sizeof(key)); c->order_valid = false; }
  pcost = c->pixel_cost;
}

// The camera rays' grazing certificate of the launch's view and their entry table: reuses the cached tile words when the key matches,
// recomputes them on the site's stream otherwise -- except in a pipelined launch that may run beside others reading them (site.hold_order): that one
// keeps the scene's margin and the root.  The two are independent -- the certificate needs a tree with own bounds (option camera_cert), the table any
// wide tree (option camera_entry) -- and share the view, the key and the word per tile that the kernel reads.
// Without either P keeps cert_level = null and wide_cert_k = 1: every ray carries the scene's margin and starts at the root, as before.
void cert_prepare(dr_context* c, const LaunchSite& site, RenderParams& P, int tiles) {
  P.cert_level = nullptr;
  for (float& k : P.wide_cert_k) k = 1.0f;
  const bool want_cert = c->camera_cert && c->wide_own_bounds > 0 && c->wide_mu.e > 0.0f;
  const bool want_entry = c->camera_entry && c->wide_leaf_rec && c->wide_range && c->wide_leaves > 0;
  if ((!want_cert && !want_entry) || traversal_of(c) != DR_TRAVERSAL_WIDE || !c->wide || tiles <= 0) return;
  float key[22] = {0};
  memcpy(key, c->cur_settings, 13 * sizeof(float));
  key[13] = (float)P.W; key[14] = (float)P.H; key[15] = (float)P.stripe_mod; key[16] = (float)P.stripe_rem; key[17] = (float)P.ncols; key[18] = (float)P.gy;
  key[19] = (float)(c->scene_gen & 0xffffff); key[20] = (float)c->cert_factor; key[21] = (float)(c->cert_levels + 2 * c->camera_entry + 4 * c->camera_cert);
  if (!(c->cert_valid && memcmp(c->cert_key, key, sizeof(key)) == 0)) {
    if (site.hold_order) return;
    // a single-frame launch of a view not seen before (a moving camera: every frame a new view) does not pay for the mask and the table (more than
    // they save in one frame): the view's second launch, or any launch of several frames, computes them
    if (P.batch < 2 && memcmp(c->cert_seen, key, sizeof(key)) != 0) { memcpy(c->cert_seen, key, sizeof(key)); return; }
    const double a_star = 1e-4 * (double)c->cert_factor;
    CertView cv;
    c->cert_valid = false;
    c->cert_ok = c->entry_ok = false;
    c->cert_gen++;
    // (the table asks nothing of the view's E: a scene without own bounds passes any)
    if (fill_cert_view(P, a_star, want_cert ? c->wide_mu.e : 1.0f, cv)) {
      if (c->cert_level.grow(cert_level_words(tiles), site.stream) != DR_OK || c->cert_word.grow((size_t)tiles, site.stream) != DR_OK ||
          (want_entry && c->entry_mm.grow(entry_mm_words(tiles), site.stream) != DR_OK)) return;
      for (float& k : c->cert_k) k = 1.0f;
      if (want_cert) {
        cert_ladder(c->cert_factor, c->cert_levels != 0, cv);
        if (c->cert_mask.grow(cert_mask_words(tiles, cv.n_levels), site.stream) != DR_OK) return;
        launch_cert_mask(site.stream, c->prims, c->n_prims, cv, c->cert_mask, c->cert_level, tiles);
        for (int g = 1; g <= CERT_MAX_LEVELS; g++) c->cert_k[g] = g <= cv.n_levels ? cert_factor_k(cv.level_a[g - 1]) : 1.0f;
      } else {
        (void)hipMemsetAsync(c->cert_level, 0, cert_level_words(tiles) * sizeof(uint32_t), site.stream);      // no certificate: grade 0, the scene's margin
      }
      // the tiles' words for the kernel: the grades, and the camera rays' entry records (no table: the root everywhere)
      launch_camera_entry(site.stream, c->wide, c->wide_leaf_rec, c->wide_range, c->wide_leaves, cv, want_entry ? c->entry_mm.p : nullptr, c->cert_level, c->cert_word, tiles);
      c->cert_ok = want_cert; c->entry_ok = want_entry;
    }
    memcpy(c->cert_key, key, sizeof(key));
    c->cert_tiles = tiles;
    c->cert_valid = true;
  }
  if (c->cert_ok || c->entry_ok) { P.cert_level = c->cert_word; memcpy(P.wide_cert_k, c->cert_k, sizeof(P.wide_cert_k)); }
}

// Sky tiles (option sky_tiles): when the launch runs the lean build over a view with an entry table, the tiles no leaf can be seen from
// are rendered by sky_tiles_kernel, in front of the persistent kernel on the same stream, and order / region_start become the launch's own pair
// that holds the other tiles only (kept from launch to launch while the tiles' words and the order are the same).  The plan is still made from every tile (the number of geometry tiles stays on the device).  A pipelined launch
// beside others is not split, nor one on another stream than the context's (the launch's own pair is one per context).
// sky_tiles = 2: no kernel in front -- the list, the counts and the launch's unit cursor (`cursor`: zero when the launch starts) travel in P and the
// persistent kernel's waves render the sky tiles when they retire, a unit of SKY_CHUNK frames at a time.  Only a launch that adds atomically
// (P.accumulate == 2) may cut a tile's batch into several units; every other launch is of one frame, one unit per tile.
bool sky_split(dr_context* c, const LaunchSite& site, RenderParams& P, int tiles, const int*& order, const int*& region_start, unsigned* pcost, unsigned* cursor) {
  if (!c->sky_tiles || !c->entry_ok || !P.cert_level || site.hold_order || site.stream != c->stream || P.out_frame_stride != 0) return false;
  if (P.max_depth <= 0 || !(P.spp_f > 0.0f)) return false;
  if (!plan_sky_split(plan_persistent(persistent_cfg(c, site), (long long)tiles * P.batch, P.coop_steps, false, P.wave_log != nullptr))) return false;
  // the split of the same words and the same order is the same arrays: made once, on this stream, and reused by the launches behind it (every launch
  // that splits runs on this stream, so none reads the arrays while they are rewritten)
  const uint64_t key[5] = {c->cert_gen, order ? 1u : 0u, order ? c->order_gen : 0u, (uint64_t)tiles, (uint64_t)P.regions};
  const bool room = c->launch_order.n >= (size_t)tiles && c->sky_list.n >= (size_t)tiles && c->launch_region_start.p && c->sky_counts.p;
  if (!(room && c->sky_key_valid && memcmp(c->sky_key, key, sizeof(key)) == 0)) {
    c->sky_key_valid = false;
    if (c->launch_order.grow((size_t)tiles, site.stream) != DR_OK || c->sky_list.grow((size_t)tiles, site.stream) != DR_OK ||
        c->launch_region_start.grow(2 * MAX_REGIONS + 1, site.stream) != DR_OK || c->sky_counts.grow(2, site.stream) != DR_OK)
      return false;
    launch_sky_split(site.stream, order, region_start, P.region_start, P.cert_level, tiles, P.regions, c->launch_order, c->launch_region_start, c->sky_list, c->sky_counts);
    memcpy(c->sky_key, key, sizeof(key));
    c->sky_key_valid = true;
  }
  if (c->sky_tiles == 2) {
    P.sky_list = c->sky_list; P.sky_counts = c->sky_counts; P.sky_cursor = cursor;
    P.sky_chunk = sky_chunk_frames(P.batch, P.accumulate == 2 ? SKY_CHUNK : 0);
  } else launch_sky_tiles(site.stream, P, c->sky_list, c->sky_counts, pcost);
  order = c->launch_order; region_start = c->launch_region_start;
  return true;
}

}  // namespace

// enqueue one launch (P.batch frames) at `site`; no events, no sync
int enqueue_frame(dr_context* c, const LaunchSite& site, const RenderParams& P_in) {
  RenderParams P = P_in;
  const int tiles = P.ncols * P.gy;
  P.sample_magic = sample_order_magic(c->sample_order, P.batch);      // every launch comes through here with its batch set (dr_render_accumulate, the pipeline's groups)
  if (uses_persistent(c)) {
    if (c->tile_cursor + LAUNCH_COUNTERS > TILE_COUNTERS) {
      (void)hipMemsetAsync(c->tile_counters, 0, TILE_COUNTERS * sizeof(unsigned), site.stream);
      c->tile_cursor = 0;
    }
    unsigned* counter = c->tile_counters + c->tile_cursor;      // one counter per region, and the sky units' cursor behind them
    c->tile_cursor += LAUNCH_COUNTERS;
    const int* order; unsigned* pcost;
    if (site.hold_order) {
      // a pipelined launch runs beside the previous frame's: it may read the tile order but nobody may write it (or the costs) meanwhile
      float geom[5];
      order_geometry(P, geom);
      order = (c->order_valid && c->order_capacity >= tiles && memcmp(c->order_key + 13, geom, sizeof(geom)) == 0) ? c->tile_order.p : nullptr;
      pcost = nullptr;
    } else feedback_buffers(c, site, P, tiles, order, pcost);
    if (!c->wave_log_on) P.wave_log = nullptr;
    cert_prepare(c, site, P, tiles);
    const int* launch_order = order; const int* launch_rstart = c->region_start;      // what the persistent kernel's queues hold: the order, or the split's part of it
    c->sky_split_last = sky_split(c, site, P, tiles, launch_order, launch_rstart, pcost, counter + MAX_REGIONS);
    const int log_waves = launch_persistent_kernel(site.stream, P, persistent_cfg(c, site), counter, launch_order, launch_rstart, pcost);
    if (log_waves < 0) { set_error("the persistent kernel has no build for this launch (launch_plan.hpp)"); return DR_ERR_DEVICE; }
    c->wave_log_waves = log_waves;
    // next launch's order from this launch's costs (stream-ordered, no host sync).  The view does not change between the frames of
    // a progressive render, so after the first two launches of a view the order is refreshed every feedback_every-th launch only
    // (the two kernels take 75 us: nothing for a launch of 32 frames, 6 % of a launch of one)
    if (pcost && !order) c->order_age = 0;
    if (pcost && (c->order_age < 2 || c->order_age % c->feedback_every == 0)) {
      const int split_limit = plan_split_limit(c->num_cus, c->occupancy, c->split_parts, c->split_waves);
      launch_tile_feedback(site.stream, c->pixel_cost, c->tile_cost, c->tile_order, c->region_start, tiles, P.regions, c->heavy_factor, c->split_steps, split_limit);
      c->order_gen++;
      c->order_args[0] = tiles; c->order_args[1] = P.regions; c->order_args[2] = c->heavy_factor; c->order_args[3] = c->split_steps; c->order_args[4] = split_limit;
      c->order_valid = true;
    }
    c->order_age++;
    return DR_OK;
  }
  c->sky_split_last = false;
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
  if (!c->pending[k]) return DR_OK;
  DR_TRY(collect_time(c, c->pev0[k], c->pev1[k], c->pending_frames[k], c->pending_samples[k]));
  c->pending[k] = false;
  return DR_OK;
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
  const int k = c->pending_next;
  DR_TRY(collect_pending(c, k));           // at most two batches in flight: reusing a pair of events waits for the batch before last
  uint64_t samples = 0;
  DR_TRY(accumulate_enqueue(c, settings13, W, H, background, frame_seed, seed_stride, nframes, c->pev0[k], c->pev1[k], samples));
  c->pending[k] = true; c->pending_frames[k] = (uint64_t)nframes; c->pending_samples[k] = samples;
  c->pending_next = k ^ 1;
  return DR_OK;
}

int dr_context_synchronize(dr_context* c) {
  if (!c) { set_error("null context"); return DR_ERR_INVALID; }
  HIP_TRY(hipSetDevice(c->device));
  DR_TRY(join_pipeline(c));
  DR_TRY(collect_pending(c, c->pending_next));       // older first
  DR_TRY(collect_pending(c, c->pending_next ^ 1));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return DR_OK;
}

}  // extern "C"
