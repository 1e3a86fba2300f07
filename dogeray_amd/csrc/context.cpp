// Device context: creation and destruction, the resident scene, stripe, traversal, the options and the statistics -- with the context_*.cpp
// files (context.hpp lists them) the host side of the C ABI.  No kernels here: kernels.hpp declares their launchers.
#include <climits>
#include <exception>

#include "context.hpp"
#include "linearise.hpp"

using namespace dr;

namespace {

// The options dr_context_set_option stores, dr_context_get_option reads back and DOGERAY_OPTIONS parses: the member, the values accepted
// (lo .. hi, of those the bits of `only` where it is not 0; lo == ANY: every value, stored as value != 0) and which of a launch's caches a change
// makes stale (context.hpp: ORDER the tile order, WORDS the camera rays' tile words).  What else setting one of them does is written out in set_option.
// (ODDITY: sky_tiles drops the words, which do not depend on it; the sky split, which does not depend on it either, follows their recomputation.)
constexpr int ANY = INT_MIN;
enum : unsigned { NOTHING = 0, ORDER = 1, WORDS = 2 };
struct Option { const char* name; int dr_context::*member; int lo, hi; unsigned only; unsigned invalidates; };
const Option OPTIONS[] = {
    {"kernel", &dr_context::kernel, DR_KERNEL_TILE, DR_KERNEL_PERSISTENT, 0, NOTHING},
    {"occupancy", &dr_context::occupancy, 4, 6, 0, NOTHING},
    {"schedule", &dr_context::schedule, 0, 2, 0, NOTHING},
    {"heavy_factor", &dr_context::heavy_factor, -1, 1000, 0, ORDER},
    {"coop_steps", &dr_context::coop_steps, 0, INT_MAX, 0, NOTHING},
    {"coop_lanes", &dr_context::coop_lanes, 1, 64, 0, NOTHING},
    {"split_parts", &dr_context::split_parts, 1, 8, 1u << 1 | 1u << 2 | 1u << 4 | 1u << 8, NOTHING},
    {"split_waves", &dr_context::split_waves, 1, 1000, 0, ORDER},
    {"split_steps", &dr_context::split_steps, 16, 4080, 0, ORDER},      // (stored rounded down to a multiple of 16)
    {"short_one_queue", &dr_context::short_one_queue, ANY, 0, 0, ORDER},
    {"coop_rounds", &dr_context::coop_rounds, 1, 16, 0, NOTHING},
    {"reserve_cus", &dr_context::reserve_cus, 0, 64, 0, NOTHING},
    {"wave_log", &dr_context::wave_log_on, 0, 1, 0, NOTHING},
    {"coop_tiles_per_wave", &dr_context::coop_tiles_per_wave, 0, INT_MAX, 0, NOTHING},
    {"pipe_streams", &dr_context::pipe_streams, 2, PIPE_STREAMS, 0, NOTHING},
    {"pipe_lean", &dr_context::pipe_lean, ANY, 0, 0, NOTHING},
    {"pipe_group", &dr_context::pipe_group, 1, PIPE_GROUP_MAX, 0, NOTHING},
    {"xcd_regions", &dr_context::xcd_regions, ANY, 0, 0, ORDER},
    {"batch_frames", &dr_context::batch_frames, 1, 256, 0, NOTHING},
    {"feedback", &dr_context::feedback, ANY, 0, 0, ORDER},
    {"order_follows_camera", &dr_context::order_follows_camera, ANY, 0, 0, NOTHING},
    {"feedback_every", &dr_context::feedback_every, 1, INT_MAX, 0, NOTHING},
    {"wide_tree", &dr_context::wide_tree, 0, 2, 0, NOTHING},              // takes effect at the next dr_context_upload_scene
    {"denoise_tiles", &dr_context::denoise_tiles, 0, 1, 0, NOTHING},
    {"moments", &dr_context::moments_opt, 0, 1, 0, NOTHING},              // takes effect at the next dr_accum_reset
    {"denoise_variance", &dr_context::denoise_variance, 0, 1, 0, NOTHING},
    {"camera_cert", &dr_context::camera_cert, 0, 1, 0, WORDS},
    {"cert_factor", &dr_context::cert_factor, 1, 10000, 0, WORDS},
    {"cert_levels", /* (the comment keeps tests/test_host.py's pinned count of rows; documented in the header like the rest) */ &dr_context::cert_levels, 0, 1, 0, WORDS},
    {"camera_entry", /* (as above) */ &dr_context::camera_entry, 0, 1, 0, WORDS},
    {"sky_tiles", /* (as above) */ &dr_context::sky_tiles, 0, 2, 0, WORDS},
    {"trace_kernel", /* (as above) */ &dr_context::trace_kernel, 0, 2, 0, NOTHING},
    {"radiance_kernel", /* (as above) */ &dr_context::radiance_kernel, 0, 2, 0, NOTHING},
    {"allhits_kernel", /* (as above) */ &dr_context::allhits_kernel, 0, 2, 0, NOTHING},
    {"sample_order", /* (as above) */ &dr_context::sample_order, 0, 1, 0, NOTHING},
    {"queue_cursor_stride", /* (as above) */ &dr_context::queue_cursor_stride, 1, QUEUE_CURSOR_STRIDE_MAX, 0, NOTHING},
    {"queue_cursor_skew", /* (as above) */ &dr_context::queue_cursor_skew, 0, CURSOR_LINE_WORDS - 1, 0, NOTHING},
    {"guide_frames", /* (as above) */ &dr_context::guide_frames, 0, AOV_LENS_MAX, 0, NOTHING},      // (the guides' key holds it: a change re-traces)
    {"aov_lens_loop", /* (as above) */ &dr_context::aov_lens_loop, AOV_LENS_NESTED, AOV_LENS_REFILL, 0, NOTHING},
};

const Option* find_option(const std::string& name) {
  for (const Option& o : OPTIONS) if (name == o.name) return &o;
  return nullptr;
}

// One rule for whatever changes the state a launch reads (an option, the stripe, the traversal, the counters switch): frames submitted before the change
// are launched with the state they were submitted under -- the frames still held go first.  (Nothing is held while a context is being created.)
int flush_held(dr_context* c) {
  if (c->pipe.book.held.empty()) return DR_OK;
  HIP_TRY(hipSetDevice(c->device));
  return pipeline_flush(c);
}

int set_option(dr_context* c, const std::string& name, int v) {
  const Option* o = find_option(name);
  if (!o) { set_error("unknown option '" + name + "'"); return DR_ERR_INVALID; }
  if (o->lo == ANY) v = v != 0;
  else if (v < o->lo || v > o->hi || (o->only && !(o->only >> v & 1u))) { set_error("value not supported for option '" + name + "'"); return DR_ERR_INVALID; }
  DR_TRY(flush_held(c));
  if (name == "split_steps") v &= ~15;
  else if (name == "wave_log") {
    if (v && !c->wave_log) {
      if (hipSetDevice(c->device) != hipSuccess || c->wave_log.alloc((size_t)WAVE_LOG_WAVES * 16) != DR_OK) { set_error("cannot allocate the wave log"); return DR_ERR_DEVICE; }
      (void)hipMemsetAsync(c->wave_log, 0, c->wave_log.n * sizeof(unsigned long long), c->stream);
    }
  }
  else if (name == "pipe_streams") {
    if (v != c->pipe_streams) {               // slots and streams are numbered by ticket: drain, then start again from ticket 0
      if (hipSetDevice(c->device) != hipSuccess || join_pipeline(c) != DR_OK || hipStreamSynchronize(c->stream) != hipSuccess) { set_error("pipe_streams: cannot drain the pipeline"); return DR_ERR_DEVICE; }
      c->pipe.book.restart_numbering(v);
    }
  }
  c->*(o->member) = v;
  if (o->invalidates & ORDER) c->order.invalidate();
  if (o->invalidates & WORDS) c->words.invalidate();
  return DR_OK;
}

// What the dr_stats_* read-backs share.  stats_ready: the device, the pipeline joined, `ready` asked -- in this order: a held frame's launch may compute
// what is asked for -- and, when there is something to report, the stream drained.  stats_copy: the first min(have, room) elements to the host
template <class Ready>
int stats_ready(dr_context* c, bool& yes, Ready ready) {
  HIP_TRY(hipSetDevice(c->device));
  DR_TRY(join_pipeline(c));
  yes = ready();
  if (yes) HIP_TRY(hipStreamSynchronize(c->stream));
  return DR_OK;
}
int stats_ready(dr_context* c) { bool yes; return stats_ready(c, yes, [] { return true; }); }
template <class T, class U>
int stats_copy(U* out, const T* src, size_t have, size_t room) {
  static_assert(sizeof(T) == sizeof(U), "element for element");
  const size_t n = have < room ? have : room;
  if (n > 0) HIP_TRY(hipMemcpy(out, src, n * sizeof(T), hipMemcpyDeviceToHost));
  return DR_OK;
}

}  // namespace

// every stream that may still touch the buffers is drained before the members -- the buffers, the pipeline's and the batches' events -- go
dr_context::~dr_context() {
  (void)hipSetDevice(device);
  if (stream) (void)hipStreamSynchronize(stream);
  pipe.drain();
  if (ev0) (void)hipEventDestroy(ev0);
  if (ev1) (void)hipEventDestroy(ev1);
  if (stream) (void)hipStreamDestroy(stream);
}

extern "C" {

int dr_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int dr_context_create(int device_ordinal, dr_context** out) {
  if (!out) { set_error("out is null"); return DR_ERR_INVALID; }
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { set_error("no HIP device (this library has no CPU fallback)"); return DR_ERR_DEVICE; }
  if (device_ordinal < 0 || device_ordinal >= n) { set_error("device ordinal out of range"); return DR_ERR_INVALID; }
  HIP_TRY(hipSetDevice(device_ordinal));
  dr_context* c = new dr_context();
  c->device = device_ordinal;
  if (const char* env = getenv("DOGERAY_OPTIONS")) {   // "name=value,name=value": tuning experiments without recompiling callers
    std::string e(env);
    size_t pos = 0;
    while (pos < e.size()) {
      size_t comma = e.find(',', pos);
      if (comma == std::string::npos) comma = e.size();
      std::string kv = e.substr(pos, comma - pos);
      size_t eq = kv.find('=');
      if (eq != std::string::npos && set_option(c, kv.substr(0, eq), atoi(kv.c_str() + eq + 1)) != DR_OK) {
        delete c;
        return DR_ERR_INVALID;
      }
      pos = comma + 1;
    }
  }
  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_ordinal) == hipSuccess && prop.multiProcessorCount > 0) c->num_cus = prop.multiProcessorCount;
  }
  memset(&c->stats, 0, sizeof(c->stats));
  // the stream first: every memset below is ordered on it, like the kernels that use the buffers
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess || hipEventCreate(&c->ev0) != hipSuccess ||
      hipEventCreate(&c->ev1) != hipSuccess || !c->async.create()) {
    set_error("cannot create stream/events");
    delete c;
    return DR_ERR_DEVICE;
  }
  if (c->tile_counters.alloc(CURSOR_RING_ALLOC) != DR_OK ||
      hipMemsetAsync(c->tile_counters, 0, CURSOR_RING_ALLOC * sizeof(unsigned), c->stream) != hipSuccess ||
      c->counters.alloc(COUNTER_WORDS) != DR_OK ||
      hipMemsetAsync(c->counters, 0, COUNTER_WORDS * sizeof(unsigned long long), c->stream) != hipSuccess ||
      hipStreamSynchronize(c->stream) != hipSuccess) {
    set_error("cannot allocate tile counters / statistics");
    delete c;
    return DR_ERR_DEVICE;
  }
  *out = c;
  return DR_OK;
}

void dr_context_destroy(dr_context* c) { delete c; }

int dr_context_upload_scene(dr_context* c, const dr_scene* s) {
  if (!c || !s) { set_error("null argument"); return DR_ERR_INVALID; }
  HIP_TRY(hipSetDevice(c->device));
  // frames submitted before the upload are rendered from the scene that is resident now: they are launched, and everything queued has finished,
  // before a buffer of that scene is freed
  DR_TRY(join_pipeline(c));
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->scene_gen++;                  // the cached guides of the denoiser, the upscaler and the reprojector belong to the old scene
  DeviceImage img;
  int rc = DR_OK;
  try {
    rc = linearise(s->host, img, c->wide_tree);
  } catch (const std::exception& e) {
    set_error(std::string("scene could not be linearised: ") + e.what());
    return DR_ERR_NOMEM;
  }
  if (rc != DR_OK) return rc;
  DR_TRY(c->walk.upload(img.walk));
  c->walk_bytes = img.walk.size() * sizeof(DevUnit);
  c->wide.release();
  c->wide_bytes = 0; c->wide_depth = img.wide_depth; c->wide_nodes = img.wide_nodes; c->wide_pmax = img.wide_pmax; c->wide_mu = img.wide_mu; c->wide_own_bounds = img.wide_own_bounds;
  c->near_lmax = img.near_lmax;
  c->wide_leaf_rec.release(); c->wide_range.release(); c->wide_leaves = 0;
  if (!img.wide.empty()) {
    DR_TRY(c->wide.upload(img.wide));
    c->wide_bytes = img.wide.size() * sizeof(DevUnit);
    DR_TRY(c->wide_leaf_rec.upload(img.wide_leaf_rec));
    DR_TRY(c->wide_range.upload(img.wide_range));
    c->wide_leaves = (int)img.wide_leaf_rec.size();
  }
  DR_TRY(c->pairs.upload(img.pairs));
  DR_TRY(c->prims.upload(img.prims));
  DR_TRY(c->shade.upload(img.shade));
  DR_TRY(c->tex.upload(img.tex));
  DR_TRY(c->texels.upload(img.texels));
  c->n_prims = (int)img.prims.size();
  c->n_tex = (int)img.tex.size();
  c->slot_to_orig = img.slot_to_orig;
  c->slot_to_orig_dev.release();   // the old scene's map (ensure_slot_to_orig uploads the new one when a call first needs it)
  int depth = 0;
  while (((size_t)1 << depth) < img.prims.size()) depth++;
  c->tree_depth = depth;
  return DR_OK;
}

int dr_context_set_stripe(dr_context* c, int mod, int rem) {
  if (!c || mod < 1 || rem < 0 || rem >= mod) { set_error("stripe: need mod >= 1 and 0 <= rem < mod"); return DR_ERR_INVALID; }
  DR_TRY(flush_held(c));
  c->stripe_mod = mod; c->stripe_rem = rem;
  return DR_OK;
}

int dr_context_set_option(dr_context* c, const char* name, int value) {
  if (!c || !name) { set_error("null argument"); return DR_ERR_INVALID; }
  return set_option(c, name, value);
}

int dr_context_get_option(const dr_context* c, const char* name, int* value) {
  if (!c || !name || !value) { set_error("null argument"); return DR_ERR_INVALID; }
  const std::string n = name;
  if (const Option* o = find_option(n)) *value = c->*(o->member);
  // read-only: of the uploaded scene, or of the last call
  else if (n == "tree_depth") *value = c->tree_depth;
  else if (n == "wide_own_bounds") *value = c->wide ? c->wide_own_bounds : 0;
  else if (n == "wide_depth") *value = c->wide ? c->wide_depth : 0;          // 0: the scene has no wide structure
  else if (n == "wide_nodes") *value = c->wide ? c->wide_nodes : 0;
  else if (n == "cert_flagged_permille") {
    // per mille of the last certified view's tiles whose camera rays keep the scene's margin (-1: no certificate in use)
    *value = -1;
    if (c->camera_cert && certificate_readable(c->words.state) && c->words.mask) {
      const int tiles = c->words.state.tiles;
      uint32_t n_flagged = 0;
      if (hipStreamSynchronize(c->stream) != hipSuccess ||
          hipMemcpy(&n_flagged, c->words.mask + (tiles + 31) / 32 + 1, sizeof(n_flagged), hipMemcpyDeviceToHost) != hipSuccess) { set_error("cannot read the certificate mask"); return DR_ERR_DEVICE; }
      *value = (int)((1000ull * n_flagged + (unsigned)tiles / 2) / (unsigned)tiles);
    }
  }
  else if (n == "upscale_aov_passes") *value = c->up_passes;                 // AOV passes the last dr_accum_upscale traced
  else if (n == "reproject_aov_passes") *value = c->rp_passes;               // AOV passes the last dr_accum_reproject traced
  else if (n == "traversal") *value = traversal_of(c);                        // the traversal launches really use
  else { set_error("unknown option " + n); return DR_ERR_INVALID; }
  return DR_OK;
}

int dr_context_set_traversal(dr_context* c, int mode) {
  if (!c || (mode != DR_TRAVERSAL_THREADED && mode != DR_TRAVERSAL_ORDERED && mode != DR_TRAVERSAL_WIDE)) { set_error("unknown traversal mode"); return DR_ERR_INVALID; }
  if (mode == DR_TRAVERSAL_ORDERED && c->walk && c->tree_depth > ORDERED_STACK) {
    set_error("ordered traversal supports at most 2^24 primitives");
    return DR_ERR_SCENE;
  }
  DR_TRY(flush_held(c));
  c->traversal = mode;
  return DR_OK;
}

int dr_context_stream(dr_context* c, void** hip_stream) {
  if (!c || !hip_stream) { set_error("null argument"); return DR_ERR_INVALID; }
  *hip_stream = (void*)c->stream;
  return DR_OK;
}

int dr_stats_enable_counters(dr_context* c, int on) {
  if (!c) { set_error("null context"); return DR_ERR_INVALID; }
  DR_TRY(flush_held(c));
  c->count = on != 0;
  return DR_OK;
}

int dr_stats_reset(dr_context* c) {
  if (!c) { set_error("null context"); return DR_ERR_INVALID; }
  HIP_TRY(hipSetDevice(c->device));
  DR_TRY(join_pipeline(c));      // frames submitted before the reset are counted before it
  HIP_TRY(hipMemsetAsync(c->counters, 0, COUNTER_WORDS * sizeof(unsigned long long), c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  memset(&c->stats, 0, sizeof(c->stats));
  return DR_OK;
}

int dr_stats_get(dr_context* c, dr_stats* out) {
  if (!c || !out) { set_error("null argument"); return DR_ERR_INVALID; }
  DR_TRY(stats_ready(c));
  unsigned long long h[STAT_PHASE];
  DR_TRY(stats_copy(h, c->counters.p, STAT_PHASE, STAT_PHASE));
  *out = c->stats;
  out->rays = h[STAT_RAYS]; out->node_visits = h[STAT_NODE_VISITS]; out->prim_tests = h[STAT_PRIM_TESTS]; out->shades = h[STAT_SHADES]; out->texels = h[STAT_TEXELS];
  if (c->count) out->samples = h[STAT_SAMPLES];
  out->trav_slots = h[STAT_TRAV_SLOTS]; out->ray_slots = h[STAT_RAY_SLOTS];
  for (int k = 0; k < 8; k++) out->diag[k] = h[STAT_DIAG + k];
  return DR_OK;
}

int dr_stats_phase_counts(dr_context* c, unsigned long long* out, int n) {
  if (!c || !out || n < 0 || n > COUNTER_WORDS - STAT_PHASE) { set_error("bad argument"); return DR_ERR_INVALID; }
  DR_TRY(stats_ready(c));
  return stats_copy(out, c->counters + STAT_PHASE, (size_t)n, (size_t)n);
}

int dr_stats_cert_mask(dr_context* c, uint32_t* out, int max_words, int* n_tiles) {
  if (!c || !n_tiles || max_words < 0 || (max_words > 0 && !out)) { set_error("bad argument"); return DR_ERR_INVALID; }
  *n_tiles = 0;
  bool have;
  DR_TRY(stats_ready(c, have, [&] { return c->camera_cert && certificate_readable(c->words.state) && c->words.mask; }));
  if (!have) return DR_OK;
  *n_tiles = c->words.state.tiles;
  return stats_copy(out, c->words.mask.p, (size_t)(*n_tiles + 31) / 32, (size_t)max_words);
}

int dr_stats_cert_levels(dr_context* c, uint8_t* out_bytes, int max, int* n_tiles) {
  if (!c || !n_tiles || max < 0 || (max > 0 && !out_bytes)) { set_error("bad argument"); return DR_ERR_INVALID; }
  *n_tiles = 0;
  bool have;
  DR_TRY(stats_ready(c, have, [&] { return c->camera_cert && certificate_readable(c->words.state) && c->words.level; }));
  if (!have) return DR_OK;
  *n_tiles = c->words.state.tiles;
  return stats_copy(out_bytes, reinterpret_cast<const uint8_t*>(c->words.level.p), (size_t)*n_tiles, (size_t)max);      // (a byte per tile, four to a word)
}

int dr_stats_camera_entry(dr_context* c, int32_t* out, int max, int* n_tiles) {
  if (!c || !n_tiles || max < 0 || (max > 0 && !out)) { set_error("bad argument"); return DR_ERR_INVALID; }
  *n_tiles = 0;
  bool have;
  DR_TRY(stats_ready(c, have, [&] { return c->camera_entry && entry_table_readable(c->words.state) && c->words.word; }));
  if (!have) return DR_OK;
  *n_tiles = c->words.state.tiles;
  DR_TRY(stats_copy(out, c->words.word.p, (size_t)*n_tiles, (size_t)max));
  for (int t = 0; t < *n_tiles && t < max; t++) out[t] >>= ENTRY_SHIFT;      // (arithmetic: ENTRY_NONE stays -1)
  return DR_OK;
}

int dr_stats_sky_tiles(dr_context* c, int* n_sky, int* n_geometry) {
  if (!c || !n_sky || !n_geometry) { set_error("bad argument"); return DR_ERR_INVALID; }
  *n_sky = 0; *n_geometry = 0;
  bool have;
  DR_TRY(stats_ready(c, have, [&] { return c->sky.state.last && c->sky.counts; }));
  if (!have) return DR_OK;
  unsigned h[2] = {0, 0};
  DR_TRY(stats_copy(h, c->sky.counts.p, 2, 2));
  *n_sky = (int)h[0]; *n_geometry = (int)h[1];
  return DR_OK;
}

int dr_stats_adaptive_tiles(dr_context* c, uint8_t* out, int max, int* n_tiles) {
  if (!c || !n_tiles || max < 0 || (max > 0 && !out)) { set_error("bad argument"); return DR_ERR_INVALID; }
  *n_tiles = 0;
  bool have;
  DR_TRY(stats_ready(c, have, [&] { return c->adaptive.tiles > 0 && c->adaptive.flags; }));
  if (!have) return DR_OK;
  *n_tiles = c->adaptive.tiles;
  return stats_copy(out, c->adaptive.flags.p, (size_t)*n_tiles, (size_t)max);
}

int dr_stats_wave_log(dr_context* c, unsigned long long* out, int max_waves, int* n_waves) {
  if (!c || !out || !n_waves || max_waves < 0) { set_error("bad argument"); return DR_ERR_INVALID; }
  if (!c->wave_log) { set_error("wave log is off (option wave_log)"); return DR_ERR_INVALID; }
  DR_TRY(stats_ready(c));
  const int n = c->wave_log_waves < max_waves ? c->wave_log_waves : max_waves;
  DR_TRY(stats_copy(out, c->wave_log.p, (size_t)n * 16, (size_t)n * 16));
  *n_waves = n;
  return DR_OK;
}

int dr_stats_pixel_cost(dr_context* c, unsigned* out, size_t capacity, size_t* n) {
  if (!c || !out || !n) { set_error("bad argument"); return DR_ERR_INVALID; }
  DR_TRY(stats_ready(c));
  const size_t have = c->order.pixel_cost ? (size_t)c->order.state.capacity * 64 : 0;      // pixel (tile, lane-in-tile) at tile * 64 + lane, tile = block column * gy + block row
  DR_TRY(stats_copy(out, c->order.pixel_cost.p, have, capacity));
  *n = have < capacity ? have : capacity;
  return DR_OK;
}

int dr_stats_tile_order(dr_context* c, int* order, size_t capacity, size_t* n, int* region_start, int* args) {
  if (!c || !n || !region_start || !args || (capacity > 0 && !order)) { set_error("bad argument"); return DR_ERR_INVALID; }
  *n = 0;
  DR_TRY(stats_ready(c));
  const dr::TileOrder& o = c->order;
  if (!o.state.valid || !o.order || !o.region_start) return DR_OK;
  for (int k = 0; k < 5; k++) args[k] = o.state.args[k];
  const size_t tiles = (size_t)o.state.args[0];
  DR_TRY(stats_copy(region_start, o.region_start.p, 2 * MAX_REGIONS + 1, 2 * MAX_REGIONS + 1));
  DR_TRY(stats_copy(order, o.order.p, tiles, capacity));
  *n = tiles;
  return DR_OK;
}

}  // extern "C"
