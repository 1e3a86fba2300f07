// The device context (struct dr_context: resident scene, options, accumulator, pipeline state) and what the context_*.cpp files share: the error
// macros, the owning device buffer, the guide caches' key, the launch site, the owners of a render launch's three caches (launch_state.hpp: tile order,
// camera words, sky split), the owner of the pipelined present loop (pipeline_state.hpp: the ticket book and the ordering plans), and the internal functions
// one file defines and another calls.
//   context.cpp            create / destroy / upload / stripe / traversal / options / statistics
//   context_render.cpp     per-launch constants, the three caches around a launch, the launches of dr_render_frame / dr_render_accumulate*
//   context_pipeline.cpp   pipelined single frames (dr_pipeline_*): asks pipeline_state.hpp's book, issues its plans, launches; FramePipeline's setup / drain
//   context_accum.cpp      the accumulator: reset, AOV, denoise, upscale, reproject, error, present, stripes, reads
//   context_adaptive.cpp   adaptive sampling (dr_render_adaptive): selection, the launches over the tile subset, the masked fold
//   context_query.cpp      what the queries on caller lists share: staging in and out, scratch, cursor, the object map's upload
//   context_trace.cpp      ray queries on caller rays (dr_trace_rays)
//   context_radiance.cpp   radiance queries on caller rays (dr_trace_radiance)
//   context_nearest.cpp    nearest-surface point queries (dr_query_nearest)
//   context_allhits.cpp    every crossing of a caller ray (dr_trace_all_hits)
//   context_probe.cpp      measurement probes and known-answer hooks
// Host only, no kernels: kernels.hpp declares their launchers.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "kernels.hpp"
#include "launch_state.hpp"
#include "params_host.hpp"
#include "pipeline_state.hpp"
#include "scene_host.hpp"

#define HIP_TRY(expr)                                                                      \
  do {                                                                                     \
    hipError_t e_ = (expr);                                                                \
    if (e_ != hipSuccess) {                                                                \
      dr::set_error(std::string(#expr) + ": " + hipGetErrorString(e_));                    \
      return DR_ERR_DEVICE;                                                                \
    }                                                                                      \
  } while (0)

// a call that returns a dr_status: anything but DR_OK is the caller's result
#define DR_TRY(expr)                                                                       \
  do {                                                                                     \
    const int rc_ = (expr);                                                                \
    if (rc_ != DR_OK) return rc_;                                                          \
  } while (0)

namespace dr {

// An owned device allocation of n elements (PINNED: page-locked host memory instead); reads as its pointer.  A failed allocation leaves it null
// with n = 0.  The destructor frees: whoever destroys it has synchronised the streams that use it.
template <class T, bool PINNED = false>
struct DevMem {
  T* p = nullptr;
  size_t n = 0;
  DevMem() = default;
  DevMem(const DevMem&) = delete;
  DevMem& operator=(const DevMem&) = delete;
  ~DevMem() { release(); }
  operator T*() const { return p; }
  void release() {
    if (p) (void)(PINNED ? hipHostFree(p) : hipFree(p));
    p = nullptr; n = 0;
  }
  void swap(DevMem& o) { std::swap(p, o.p); std::swap(n, o.n); }
  // room for `need` elements, growing only; the contents do not survive growing.  `stream` is the one whose queued work may still use the
  // allocation that is too small: it is drained before that is freed
  int grow(size_t need, hipStream_t stream) {
    if (p && n >= need) return DR_OK;
    if (p) { HIP_TRY(hipStreamSynchronize(stream)); release(); }
    const hipError_t e = PINNED ? hipHostMalloc((void**)&p, need * sizeof(T), hipHostMallocDefault) : hipMalloc((void**)&p, need * sizeof(T));
    if (e != hipSuccess) { p = nullptr; set_error(std::string("cannot allocate ") + std::to_string(need * sizeof(T)) + " bytes: " + hipGetErrorString(e)); return DR_ERR_DEVICE; }
    n = need;
    return DR_OK;
  }
  int alloc(size_t count) { release(); return grow(count ? count : 1, nullptr); }      // a fresh allocation of at least one element
  int upload(const std::vector<T>& src) { DR_TRY(alloc(src.size())); return put(src.data(), src.size()); }
  int put(const T* src, size_t count) { if (count) HIP_TRY(hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice)); return DR_OK; }
  int get(T* dst, size_t count) const { if (count) HIP_TRY(hipMemcpy(dst, p, count * sizeof(T), hipMemcpyDeviceToHost)); return DR_OK; }
};
template <class T, bool PINNED>
void swap(DevMem<T, PINNED>& a, DevMem<T, PINNED>& b) { a.swap(b); }

// The key of a cached set of first-hit guides: the view's settings13, the frame size and the scene upload they were traced for, and the frames
// they were averaged over (option guide_frames; 0: the pinhole pass, which is all dr_accum_reproject's pair ever holds)
struct GuideKey {
  bool valid = false;
  float st[13] = {0};
  int W = 0, H = 0;
  uint64_t gen = 0;
  int frames = 0;
  bool matches(const float* settings13, int w, int h, uint64_t scene_gen, int guide_frames = 0) const {
    return valid && W == w && H == h && gen == scene_gen && frames == guide_frames && memcmp(st, settings13, sizeof(st)) == 0;
  }
  void store(const float* settings13, int w, int h, uint64_t scene_gen, int guide_frames = 0) {
    memcpy(st, settings13, sizeof(st));
    W = w; H = h; gen = scene_gen; frames = guide_frames; valid = true;
  }
};

// A set of first-hit guide planes over a grid of n pixels, in one allocation, and the key of the view traced into them.  In floats:
//   quad(0) 4n | ... | quad(quads - 1) 4n | rgb 3n | material n | scalar n
// the float4 planes first (hipMalloc's alignment, and n is a multiple of 64: every one of them is 16-byte aligned).  The denoiser's set has three
// float4 planes -- the guide (n, z), then the colour planes A and B --, the upsampler's full-resolution set two -- the guide and a scratch --; rgb is
// the albedo and scalar the depth gradient gz.  Plane 1 is where trace_guides (context_accum.cpp) has launch_aov write normal and depth before the
// guide prepare packs them.  A set of dr_accum_reproject's pair has no float4 plane, and its scalar, t, comes first:
//   scalar n | rgb 3n | material n          (rgb is the normal)
// The casts live here only.
struct GuidePlanes {
  DevMem<float> mem;
  GuideKey key;
  size_t n = 0;
  int quads = 0;
  // room for `pixels` x (4 float4_planes + 5) floats; growing loses the contents, so the key no longer holds
  int grow(size_t pixels, int float4_planes, hipStream_t stream) {
    const size_t need = pixels * (size_t)(4 * float4_planes + 5);
    if (need > mem.n) key.valid = false;
    DR_TRY(mem.grow(need, stream));
    n = pixels; quads = float4_planes;
    return DR_OK;
  }
  float* quad(int k) const { return mem.p + 4 * n * (size_t)k; }
  float* rgb() const { return quad(quads) + (quads ? 0 : n); }
  int32_t* material() const { return reinterpret_cast<int32_t*>(rgb() + 3 * n); }
  float* scalar() const { return quads ? rgb() + 4 * n : mem.p; }
};

// Where a render launch goes and what it may touch on the way
struct TileSubset;
struct LaunchSite {
  hipStream_t stream;       // the launch, the tile counters' memset, the certificate mask and the feedback kernels
  bool hold_order;          // use the stored tile order as it is, record no costs, compute no mask (a pipelined launch beside another one)
  bool lean;                // option pipe_lean: the launch counts 0 for coop_tiles_per_wave
  TileSubset* subset = nullptr;      // the launch renders the flagged tiles only (dr_render_adaptive; launch_state.hpp site_use); null everywhere else
};

// The three caches of a render launch (launch_state.hpp holds their state and every rule about it; context_render.cpp is the only writer).  Each owns
// its buffers, and invalidate() is all that anything outside may do to it.

// Cost feedback of the persistent kernel: per-pixel cost of the last frame, per-tile cost, and the tile order made from them
struct TileOrder {
  DevMem<unsigned> pixel_cost, tile_cost;
  DevMem<int> order, region_start;
  OrderState state;
  void invalidate() { state.valid = false; }
  // room for the state.capacity tiles order_begin asked for (OrderUse::grow: the stored order is gone already); none at all if that fails
  int grow(hipStream_t stream) {
    const size_t tiles = (size_t)state.capacity;
    state.capacity = 0;
    DR_TRY(pixel_cost.grow(tiles * 64, stream)); DR_TRY(tile_cost.grow(tiles, stream));
    DR_TRY(region_start.grow(2 * MAX_REGIONS + 1, stream)); DR_TRY(order.grow(tiles, stream));
    state.capacity = (int)tiles;
    return DR_OK;
  }
};

// The camera rays' grazing certificate and entry table of one view, computed on the launch's stream by launch_cert_mask and, behind
// it, launch_camera_entry, and kept under one key: per tile one bit of the mask (set: its camera rays keep the scene's margin), one byte (its grade on
// the ladder of option cert_levels) and one word, entry code << ENTRY_SHIFT | grade -- what the render kernel reads (RenderParams cert_level)
struct CameraWords {
  DevMem<uint32_t> mask;
  DevMem<uint32_t> level;                  // the grades, four tiles to a word
  DevMem<uint32_t> mm;                     // scratch: the lowest and the highest rank per tile
  DevMem<uint32_t> word;
  CameraWordsState state;
  void invalidate() { state.valid = false; }
  // room for the words of `tiles` tiles (mm_too: and the entry table's scratch); what the buffers held does not survive
  int grow(int tiles, bool mm_too, hipStream_t stream) {
    state.valid = false;
    DR_TRY(level.grow(cert_level_words(tiles), stream)); DR_TRY(word.grow((size_t)tiles, stream));
    if (mm_too) DR_TRY(mm.grow(entry_mm_words(tiles), stream));
    return DR_OK;
  }
  int grow_mask(int tiles, int n_levels, hipStream_t stream) { state.valid = false; return mask.grow(cert_mask_words(tiles, n_levels), stream); }
};

// A launch's own order / region_start pair: what launch_order_split (kernels.hpp) writes and the persistent kernel's queues then hold instead of TileOrder's
struct LaunchPair {
  DevMem<int> order, region_start;
  bool room(int tiles) const { return order.n >= (size_t)tiles && region_start.p; }
  int grow(int tiles, hipStream_t stream) { DR_TRY(order.grow((size_t)tiles, stream)); return region_start.grow(2 * MAX_REGIONS + 1, stream); }
};

// The frame buffers of a launch of several frames: cap_frames buffers of elems_each int32, one after the other
struct FrameBuffers {
  DevMem<int32_t> frames; size_t elems_each = 0; int cap_frames = 0;
  operator int32_t*() const { return frames.p; }
  // room for `need` buffers of `elems` int32: made anew (*regrown), `cap` >= need of them, when a buffer's size changes or they are too few; stream: DevMem::grow's
  int fit(size_t elems, int need, int cap, hipStream_t stream, bool* regrown = nullptr) {
    const bool stale = elems_each != elems || cap_frames < need || !frames;
    if (regrown) *regrown = stale;
    if (!stale) return DR_OK;
    cap_frames = 0;
    DR_TRY(frames.grow(elems * (size_t)cap, stream));
    elems_each = elems; cap_frames = cap;
    return DR_OK;
  }
};

// Sky tiles: a lean launch with an entry table hands the tiles of code ENTRY_NONE to sky_tiles_kernel, or to its own retiring waves,
// and the rest of its order to the persistent kernel's queues (context_render.cpp sky_split).  The split is made on the launch's stream and kept while
// the words and the order it was made from are the same (the split's kernel takes 0.53 % of a 32-frame launch of the bench view,
// profiles/sky_tiles_ab.txt)
struct SkySplit {
  LaunchPair pair;
  DevMem<int> list;
  DevMem<unsigned> counts;                 // [0] sky tiles, [1] geometry tiles of the last split
  SkySplitState state;
  void invalidate() { state.valid = false; }
  bool room(int tiles) const { return pair.room(tiles) && list.n >= (size_t)tiles && counts.p; }
  int grow(int tiles, hipStream_t stream) {
    state.valid = false;
    DR_TRY(pair.grow(tiles, stream)); DR_TRY(list.grow((size_t)tiles, stream));
    return counts.grow(2, stream);
  }
};

// The tiles of one adaptive pass (dr_render_adaptive; context_adaptive.cpp is the only writer): a flag per tile of the view and the two
// counts, made by the selection on the context's stream; the launch's own order / region_start pair, split from the order each of the pass's launches
// would have used (context_render.cpp subset_split) and read by the persistent kernel and by the fold behind it; and the frame buffers the launches
// render into.  No cache: every pass selects anew, `tiles` only says what dr_stats_adaptive_tiles may read back
struct TileSubset {
  DevMem<uint8_t> flags;
  DevMem<unsigned> counts;                 // [AD_ACTIVE] active tiles, [AD_ASKING] asking pixels of the last selection
  LaunchPair pair;
  FrameBuffers frames;
  int tiles = 0;                           // tiles of the last pass's selection (0: none to read back)
  void invalidate() { tiles = 0; }
  int grow(int ntiles, size_t elems, int nframes, hipStream_t stream) {
    tiles = 0;
    DR_TRY(flags.grow((size_t)ntiles, stream)); DR_TRY(counts.grow(AD_WORDS, stream));
    DR_TRY(pair.grow(ntiles, stream));
    return frames.fit(elems, nframes, nframes, stream);
  }
};

// Pipelined single frames (dr_pipeline_*): render streams the groups alternate between, a stream that folds finished frames into the
// accumulator in ticket order, PIPE_DEPTH slots of frame / present buffers that rotate, and the book that says which ticket is where
// (pipeline_state.hpp holds it and every rule about it; context_pipeline.cpp asks, issues and launches).  Outside it: restart_numbering(), drain()
struct FramePipeline {
  typedef DevMem<uint8_t, true> Image;             // a frame's present, pinned
  hipStream_t stream[PIPE_STREAMS] = {nullptr, nullptr, nullptr, nullptr}, acc_stream = nullptr;      // stream[0] is the context's own (not owned)
  struct Slot {
    FrameBuffers frames;
    int rect[6] = {-1, 0, 0, 0, 0, 0};             // W, H, gx, gy, stripe mod, stripe rem the buffers were last rendered with (their margins are 0)
    hipEvent_t rendered = nullptr;                 // end of the group's launch
    hipEvent_t added[PIPE_GROUP_MAX] = {nullptr};  // frame f of the group has been added (and presented)
    DevMem<uint8_t> rgb_dev[PIPE_GROUP_MAX]; Image rgb_host[PIPE_GROUP_MAX];      // frame f's present: on the device, and its pinned copy
  };
  Slot slot[PIPE_DEPTH];
  hipEvent_t last[PIPE_STREAMS] = {nullptr, nullptr, nullptr, nullptr};        // end of the newest launch on each render stream
  hipEvent_t barrier = nullptr;                    // end of the newest launch that ran alone: later launches read the order it left
  hipEvent_t sync = nullptr;                       // orders the pipeline after earlier work on the context's stream
  bool ready = false;                              // every stream and event exists (setup)
  TicketBook<Image> book;
  int setup(hipStream_t own);                      // context_pipeline.cpp: creates what is missing
  void drain() const;                              // ... waits for the streams it owns
  ~FramePipeline();                                // ... destroys its events and streams (drained by then); the buffers then free themselves
};

// dr_render_accumulate_async: two batches may be in flight, each with its own pair of events
struct AsyncBatches {
  struct Batch { hipEvent_t ev0 = nullptr, ev1 = nullptr; bool pending = false; uint64_t frames = 0, samples = 0; };
  Batch batch[2];
  int next = 0;                                    // the batch the next call uses: the older of the two
  int older() const { return next; }
  int newer() const { return next ^ 1; }
  bool create() {
    for (Batch& b : batch) if (hipEventCreate(&b.ev0) != hipSuccess || hipEventCreate(&b.ev1) != hipSuccess) return false;
    return true;
  }
  // batch k's time, if its events are still outstanding (waits for that batch, not for later ones): collect_time(ev0, ev1, frames, samples) adds it
  template <class CollectTime>
  int collect(int k, CollectTime collect_time) {
    Batch& b = batch[k];
    if (!b.pending) return DR_OK;
    DR_TRY(collect_time(b.ev0, b.ev1, b.frames, b.samples));
    b.pending = false;
    return DR_OK;
  }
  // the older batch's events now bracket a new batch: the other one is the older
  void started(uint64_t frames, uint64_t samples) {
    Batch& b = batch[next];
    b.pending = true; b.frames = frames; b.samples = samples;
    next ^= 1;
  }
  ~AsyncBatches() { for (Batch& b : batch) { if (b.ev0) (void)hipEventDestroy(b.ev0); if (b.ev1) (void)hipEventDestroy(b.ev1); } }
};

}  // namespace dr

// option sample_order's default (the macro serves variant libraries of an A/B, as DR_SKY_CHUNK does)
#ifndef DR_SAMPLE_ORDER
#define DR_SAMPLE_ORDER 1
#endif

struct dr_context {
  template <class T> using DevMem = dr::DevMem<T>;
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  dr::AsyncBatches async;
  // resident scene
  DevMem<dr::DevUnit> walk; size_t walk_bytes = 0;
  DevMem<dr::DevUnit> wide; size_t wide_bytes = 0; int wide_depth = 0, wide_nodes = 0; float wide_pmax = 0; dr::WideMu wide_mu = {0, 0, 0}; int wide_own_bounds = 0;   // null: scene not representable (threaded walk is used)
  int wide_tree = 2;        // structure of the wide walk's tree: 2 binned SAH with small triangles entered by their own bounds (default), 1 binned SAH over the reference's leaf boxes, 0 the reference's topology collapsed
  DevMem<dr::DevPair> pairs;
  DevMem<dr::DevPrim> prims;
  DevMem<dr::DevShade> shade;
  DevMem<dr::DevTex> tex;
  DevMem<uint32_t> texels;
  int n_prims = 0, n_tex = 0, tree_depth = 0;
  std::vector<int> slot_to_orig;
  DevMem<int32_t> slot_to_orig_dev;        // the same map on the device: uploaded by the first call that reads it after a scene upload (ensure_slot_to_orig)
  // the queries on caller lists (dr_trace_rays, dr_trace_radiance, dr_query_nearest, dr_trace_all_hits; context_query.cpp): the staging of host inputs
  // and results -- and of the host outputs of the accumulator's stages (dr_render_aov, dr_accum_denoise / _upscale / _error / _present) --, the
  // two words per entry between a walk kernel and its surface / finishing pass ({t or d2 bits, slot}), and the persistent kernels' cursor -- each
  // made by the first call that needs it (a context that never queries allocates nothing).  One of each serves every query: they are used on
  // `stream` only, one call's work queued behind the other's, and DevMem::grow drains `stream` before it frees what is too small, so no kernel of
  // an earlier device-pointer call still reads what a later call replaces
  DevMem<uint8_t> query_staging;
  DevMem<uint32_t> query_scratch;
  DevMem<unsigned> query_cursor;
  // options (private, for the tests): 0 the plan decides (launch_plan.hpp), 1 the one-ray-per-lane kernel, 2 the persistent kernel where it exists
  int trace_kernel = 0, radiance_kernel = 0, allhits_kernel = 0;
  float near_lmax = 0;                     // dr_query_nearest: the scene's largest |e1| + |e2| / radius (the pruning slack's constant, device_nearest.hpp)
  // dr_accum_denoise: the guide planes and the two colour planes of the pixel grid (made by the first call), keyed by the view they were traced
  // for (settings13, W, H, scene generation)
  dr::GuidePlanes dn_guides;
  // dr_accum_upscale: the full-resolution guides (made by the first guided call), keyed by settings13 with element 11 = 1, W, H, scene generation,
  // and the AOV passes of the last call
  dr::GuidePlanes up_guides;
  int up_passes = 0;
  int guide_frames = 0;                    // option: 0 the guides are the pinhole pass's; G > 0 the lens kernel's over G frames of DR_GUIDE_SEED (trace_guides)
  int aov_lens_loop = 0;                   // private option: the lens kernel's loop shape (kernels.hpp AOV_LENS_*: 0 nested, 1 refilling), for the A/B
  uint64_t scene_gen = 0;                  // scene uploads so far: a guide cache of an earlier scene does not match
  // dr_accum_reproject: the second accumulator of the pair (swapped with `accum` by every reprojection), the two history planes (hist: the
  // current one, null until the first reprojection and after dr_accum_reset), the guide planes of two views (t n | normal 3n | material n
  // floats each; set rp_cur holds the cached `to` view under its key, the other set's key is never valid), the class counts and the AOV passes of
  // the last call
  DevMem<int32_t> accum2;
  DevMem<int32_t> hist_buf[2];
  int32_t* hist = nullptr; int hist_cur = 0;
  dr::GuidePlanes rp_guides[2]; int rp_cur = 0;
  DevMem<unsigned long long> rp_counts;
  int rp_passes = 0;
  // the second-moment plane (option "moments", read by dr_accum_reset): m2 is the current plane (null: none), one of m2_buf -- the second one
  // appears with the first reprojection, as for the history; the allocations outlive resets of the same size.  dr_accum_error's counts
  int moments_opt = 0;                     // option: dr_accum_reset gives the accumulator a plane
  int denoise_variance = 0;                // option: the denoiser's variance pre-pass takes the temporal variance from the plane (n >= 4)
  DevMem<unsigned long long> m2_buf[2];
  unsigned long long* m2 = nullptr; int m2_cur = 0;
  DevMem<unsigned long long> err_counts;
  int denoise_tiles = 1;                   // option: a-trous passes on 16x16 lattice tiles in LDS (1) or with every tap loaded from the planes (0)
  // the camera rays' grazing certificate and entry table: the options, the wide tree's side arrays the table is made from, and the
  // words of the last view (launch_state.hpp same_words_view: keyed by settings13, frame, stripe, tile grid, scene upload and the four options)
  int camera_cert = 1;                     // option: camera rays of tiles the certificate clears carry the certified margin (0: every ray the scene's)
  int cert_factor = 40;                    // option: the certified |a^| in units of hit_tri's 1e-4 cut-off (a_star = cert_factor * 1e-4)
  int cert_levels = 1;                     // option: 1 the graded ladder cert_factor x {1/4, 1/2, 1, 2, 4} (params_host.hpp cert_ladder), 0 the single step cert_factor
  int camera_entry = 1;                    // option: a tile's camera rays start at the lowest record that holds every leaf they can reach (0: at the root)
  DevMem<uint32_t> wide_leaf_rec, wide_range;   // the wide tree's side arrays (linearise.hpp): rank -> leaf record; record -> the ranks under it
  int wide_leaves = 0;
  dr::CameraWords words;
  int sample_order = DR_SAMPLE_ORDER;      // option: which samples of a tile share a unit of the queue (launch_plan.hpp tile_sample): 0 a frame's 64 pixels, 1 a pixel's frames
  int sky_tiles = 2;                       // option: 0 every tile goes through the persistent kernel; 1 sky_tiles_kernel in front of it; 2 its retiring waves
  dr::SkySplit sky;
  dr::TileSubset adaptive;                 // dr_render_adaptive's tiles, launch pair and frame buffers
  // frame + accumulator
  DevMem<int32_t> frame;
  DevMem<int32_t> accum; int accW = 0, accH = 0;
  // multi-GPU gather: two packed copies of this context's stripe (double buffer), sized for the accumulator
  DevMem<int32_t> packed[2];
  DevMem<unsigned long long> counters;
  // the ring of the queues' cursors, where the last launch's block ended, and the layout's two options (launch_plan.hpp cursor_take holds the rule)
  DevMem<unsigned> tile_counters; int tile_cursor = 0;
  int queue_cursor_stride = dr::QUEUE_CURSOR_STRIDE, queue_cursor_skew = 0;
  int num_cus = 256;
  // cost feedback (persistent kernel): its options, and the tile order of the last view
  int feedback = 1;
  int order_follows_camera = 1;    // a view with the same frame geometry but other settings starts from the previous view's tile order
  int feedback_every = 8;          // ... the order is recomputed after the first two of them and then after every feedback_every-th
  dr::TileOrder order;
  int stripe_mod = 1, stripe_rem = 0;
  int traversal = DR_TRAVERSAL_WIDE;
  int count = 0;
  // tunables (dr_context_set_option / DOGERAY_OPTIONS; the table in context.cpp names them)
  int kernel = DR_KERNEL_PERSISTENT;
  int occupancy = 6;        // waves per SIMD the kernel is built and launched for (persistent: 4, 5, or 6 = six for the lean wide build and five for the others; tile kernel: 4 or 6)
  int schedule = 0;         // persistent kernel: 0 = shade / refill below 32 walking lanes, leaf steps for 20 lanes, two steps per iteration (tuned); 1 = 32 / 8 / 1; 2 = 48 / leaves on the spot / 1
  int xcd_regions = 1;      // persistent kernel: one tile queue per XCD (image bands), with stealing
  int heavy_factor = 1;     // tile order: tiles costlier than this x the mean start first, the rest keep their natural order (0 = all natural, -1 = all by cost)
  int coop_steps = 2;       // persistent kernel, drain phase: rays older than this many steps are shared with idle lanes / finished cooperatively (0 = off)
  int coop_tiles_per_wave = 32;   // wide walk: launches with fewer tiles per wave than this run the build with the work-sharing drain
  int coop_lanes = 8;       // ... in waves with at most this many lanes still walking
  int split_parts = 4;      // short launches: the tiles with last frame's longest pixels are handed out in this many parts (1, 2, 4, 8), the rest of each wave helps
  int split_waves = 12;     // ... as many of them as give this many percent of the waves a part to start with
  int split_steps = 400;    // ... tiles whose longest pixel took at least this many node steps (multiple of 16)
  int short_one_queue = 1;  // short launches use one tile queue instead of one per XCD
  int coop_rounds = 2;      // work sharing: hand-over rounds per loop iteration
  int reserve_cus = 0;      // persistent kernel: launch workgroups for this many CUs fewer than the device has (room for a gather's copy / RCCL kernels beside the rendering)
  int wave_log_on = 0;      // persistent kernel writes begin / queue-empty / end stamps of every wave (dr_stats_wave_log)
  DevMem<unsigned long long> wave_log; int wave_log_waves = 0;
  int batch_frames = 32;    // persistent kernel: at most this many frames per launch in dr_render_accumulate
  float cur_settings[13] = {0};
  dr_stats stats;
  // pipelined single frames (dr_pipeline_*): the three options (the option table holds int members) and the pipeline itself
  int pipe_streams = 2;     // render streams the pipeline alternates between (a change restarts the ticket numbering)
  int pipe_lean = 0;        // pipelined launches run the lean build with one queue per XCD instead of the work-sharing build (their tails overlap other frames)
  int pipe_group = 8;       // most frames per group (1 = a launch per frame)
  dr::FramePipeline pipe;

  dr::LaunchSite own_site() const { return {stream, false, false}; }      // an ordinary launch: on `stream`, with cost feedback
  ~dr_context();            // context.cpp: drains every stream, destroys its own events and stream; the members then release theirs
};

namespace dr {

// the traversal a launch really uses: the wide walk needs its structure (scenes it cannot represent walk the threaded links)
inline int traversal_of(const dr_context* c) { return (c->traversal == DR_TRAVERSAL_WIDE && !c->wide) ? DR_TRAVERSAL_THREADED : c->traversal; }
inline bool uses_persistent(const dr_context* c) { return c->kernel == DR_KERNEL_PERSISTENT && traversal_of(c) != DR_TRAVERSAL_ORDERED; }

// context_render.cpp
void fill_scene(const dr_context* c, RenderParams& P);      // the resident scene's buffers
ViewKey view_key(const dr_context* c, const RenderParams& P);      // the launch's view: make_params' settings, P's geometry, the scene and the words' options
int make_params(dr_context* c, const LaunchSite& site, const float* st, int W, int H, float background, uint64_t seed, RenderParams& P, int batch_hint = 1);
PersistentCfg persistent_cfg(const dr_context* c, const LaunchSite& site);
int enqueue_frame(dr_context* c, const LaunchSite& site, const RenderParams& P_in);
// context_pipeline.cpp
int join_pipeline(dr_context* c);
int pipeline_flush(dr_context* c);
int pipeline_group_room(const dr_context* c);      // how many frames a group may hold right now (the pipeline's groups, and dr_render_adaptive's)
// context_query.cpp: a list of n caller items through the device and back; an accumulator stage's host outputs are the channels of a list of pixels
// without inputs
struct QueryIn { const void* p; int words; };                 // a caller's input array (null: not given) and its 4-byte words per item
// a channel (null: not wanted), its words per entry, each of `unit` bytes (rgb8: 3 words of 1); per_item: one entry per item whatever K
struct QueryOut { void* p; int words; bool per_item; int unit = 4; };
constexpr int QUERY_MAX_IN = 4, QUERY_MAX_OUT = 9;
struct QueryIo {
  const void* in[QUERY_MAX_IN];            // where the kernels read input k (null: not given) ...
  void* out[QUERY_MAX_OUT];                // ... and write channel k (null: not wanted): the caller's memory, or staging
  size_t out_bytes[QUERY_MAX_OUT];
};
int ensure_slot_to_orig(dr_context* c);
int query_begin(dr_context* c, size_t n, size_t K, const QueryIn* in, int n_in, const QueryOut* out, int n_out, bool device_pointers, QueryIo& io);
int query_scratch(dr_context* c, size_t entries, uint32_t*& words);
int query_cursor(dr_context* c, unsigned*& cursor);
int query_end(dr_context* c, const QueryOut* out, int n_out, bool device_pointers, const QueryIo& io);

}  // namespace dr
