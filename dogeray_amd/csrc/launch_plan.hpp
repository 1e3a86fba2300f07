// Which build of render_persistent_kernel a launch runs, with what grid, and the launch-size rules around it, as plain data.
// No HIP: kernels_render.hip launches what plan_persistent returns, and the host build exports it (tests/test_launch_plan_host.py).
// ODDITY marks behaviour nobody would write on purpose that is kept bit for bit; DESIGN.md 4.3 explains each.
#pragma once
#include "../../include/dogeray_amd.h"
#include "device_layout.h"

namespace dr {

constexpr int MAX_REGIONS = 8;           // tile queues of the persistent kernels (one per XCD)
constexpr int WAVE_LOG_WAVES = 16384;    // waves the wave log (option wave_log) has room for

// What a launch of the persistent kernel needs to know of the context's options (dr_context_set_option)
struct PersistentCfg {
  int traversal;             // the traversal the launch really uses (DR_TRAVERSAL_WIDE or DR_TRAVERSAL_THREADED)
  int occupancy;             // 4, 5 or 6 waves per SIMD
  int schedule;              // 0, 1, 2: option "schedule" (DR_SCHEDULE_* below)
  int num_cus;               // CUs the launch may fill (the device's less option reserve_cus)
  int coop_tiles_per_wave;
  bool count;                // counting build
};

struct PersistentBuild { int count, occ, trav_min, park_min, unroll, wide, coop, perframe; };      // render_persistent_kernel's template arguments
inline bool operator==(const PersistentBuild& a, const PersistentBuild& b) {
  return a.count == b.count && a.occ == b.occ && a.trav_min == b.trav_min && a.park_min == b.park_min && a.unroll == b.unroll && a.wide == b.wide &&
         a.coop == b.coop && a.perframe == b.perframe;
}

// The instantiated schedules (option "schedule") as TRAV_MIN, PARK_MIN, P_UNROLL and the work-sharing build's own PARK_MIN, P_UNROLL:
// 0 = the tuned one -- shade / refill below 32 walking lanes, leaf steps for 20 lanes, two steps per loop iteration --; 1 and 2 keep the other
// paths of the loop alive in the tests (leaf steps for 8 lanes, one step per iteration; shade / refill below 48 lanes, leaves tested on the
// spot).  Every other combination rounds 2 and 3 measured is in profiles/r2_*, r3_p_*.
// (the work-sharing build's own pair: short launches like fewer lanes per leaf step and more steps between two looks at the queue: 32 / 12 / 4
// against the lean build's 32 / 20 / 2, one frame per launch 0.915 against 0.945 ms, profiles/r4_q_short_launch_schedule.txt)
#define DR_SCHEDULE_0 32, 20, 2, 12, 4
#define DR_SCHEDULE_1 32, 8, 1, 8, 1
#define DR_SCHEDULE_2 48, 0, 1, 0, 1
struct PersistentSchedule { int trav_min, park_min, unroll, coop_park, coop_unroll; };
constexpr PersistentSchedule PERSISTENT_SCHEDULES[3] = {{DR_SCHEDULE_0}, {DR_SCHEDULE_1}, {DR_SCHEDULE_2}};

// Every instantiation that exists, X(count, occ, trav_min, park_min, unroll, wide, coop, perframe): 33.  Per occupancy 4 / 5 and schedule: wide
// counting, wide work-sharing, wide lean, threaded counting, threaded plain (the threaded builds never read COOP: they carry the template's
// default, true); then the six-wave lean build -- 80 VGPRs and 26 KiB of LDS per workgroup: only the wide walk's lean build fits, and only with
// the default schedule --, its twin that stores every frame of a batch into its own buffer, and the five-wave work-sharing build that does.
#define DR_BUILDS_OF_(X, OCC, T, P, U, CP, CU)                                                                                          \
  X(true, OCC, T, P, U, true, false, false) X(false, OCC, T, CP, CU, true, true, false) X(false, OCC, T, P, U, true, false, false)     \
  X(true, OCC, T, P, U, false, true, false) X(false, OCC, T, P, U, false, true, false)
#define DR_BUILDS_OF(X, OCC, SCHEDULE) DR_BUILDS_OF_(X, OCC, SCHEDULE)
#define DR_BUILDS_OCC(X, OCC) DR_BUILDS_OF(X, OCC, DR_SCHEDULE_0) DR_BUILDS_OF(X, OCC, DR_SCHEDULE_1) DR_BUILDS_OF(X, OCC, DR_SCHEDULE_2)
#define DR_PERSISTENT_BUILDS(X)                                                                                                         \
  X(false, 6, 32, 20, 2, true, false, true) X(false, 6, 32, 20, 2, true, false, false) X(false, 5, 32, 12, 4, true, true, true)        \
  DR_BUILDS_OCC(X, 5) DR_BUILDS_OCC(X, 4)

// The instantiations of the per-tile kernel, X(count, mode, occ): 12
#define DR_TILE_BUILDS_OCC(X, OCC)                                                                                                      \
  X(true, DR_TRAVERSAL_ORDERED, OCC) X(true, DR_TRAVERSAL_WIDE, OCC) X(true, DR_TRAVERSAL_THREADED, OCC)                                \
  X(false, DR_TRAVERSAL_ORDERED, OCC) X(false, DR_TRAVERSAL_WIDE, OCC) X(false, DR_TRAVERSAL_THREADED, OCC)
#define DR_TILE_BUILDS(X) DR_TILE_BUILDS_OCC(X, 6) DR_TILE_BUILDS_OCC(X, 4)

struct PersistentPlan {
  PersistentBuild build;
  int blocks;               // workgroups of 256 threads
  int log_waves;            // what launch_persistent_kernel returns: the waves the caller takes to have written the wave log
  bool clear_wave_log;      // the launch passes wave_log = nullptr
};

// fewer than tiles_per_wave tiles for each of `waves` waves (the callers measure against different wave counts)
inline bool short_launch(long long work, int tiles_per_wave, long long waves) { return work < (long long)tiles_per_wave * waves; }

// the six-wave lean build fits, and with it the builds that store every frame of a batch into its own buffer (out_frame_stride != 0) exist
inline bool persistent_can_store_per_frame(const PersistentCfg& cfg) {
  return cfg.traversal == DR_TRAVERSAL_WIDE && !cfg.count && cfg.schedule == 0 && cfg.occupancy >= 6;
}

// work = tiles x frames of the launch; coop_steps, per_frame, wave_log_on: RenderParams' coop_steps, out_frame_stride != 0, wave_log != null
inline PersistentPlan plan_persistent(const PersistentCfg& cfg, long long work, int coop_steps, bool per_frame, bool wave_log_on) {
  const PersistentSchedule& s = PERSISTENT_SCHEDULES[cfg.schedule == 0 ? 0 : cfg.schedule == 1 ? 1 : 2];
  const bool wide = cfg.traversal == DR_TRAVERSAL_WIDE, six = persistent_can_store_per_frame(cfg);
  per_frame = per_frame && six;      // (every other configuration renders a batch into one buffer: context_pipeline.cpp asks before it sets a stride)
  auto blocks_for = [&](int occ) {   // occ waves per SIMD on every CU, four waves per workgroup, no more waves than work
    const int blocks = cfg.num_cus * occ;
    return (long long)blocks * 4 > work ? (int)((work + 3) / 4) : blocks;
  };
  PersistentPlan p;
  // ODDITY: too short for six waves is measured against a five-wave grid NOT clamped to the work ...
  if (six && !(coop_steps > 0 && short_launch(work, cfg.coop_tiles_per_wave, (long long)cfg.num_cus * 5 * 4))) {
    p.build = {false, 6, s.trav_min, s.park_min, s.unroll, true, false, per_frame};
    p.blocks = blocks_for(6);
    p.log_waves = 0; p.clear_wave_log = true;      // (the lean kernel does not log its waves)
    return p;
  }
  const int occ = cfg.occupancy >= 5 ? 5 : 4;
  p.blocks = blocks_for(occ);
  p.clear_wave_log = wave_log_on && p.blocks * 4 > WAVE_LOG_WAVES;
  p.log_waves = wave_log_on && !p.clear_wave_log ? p.blocks * 4 : 0;
  // the cooperative drain shortens a launch's tail; with many tiles per wave the tail does not show and the leaner build is faster
  // ODDITY: ... and here against the launch's own grid, which is; a short group of per-frame stores does not ask again
  const bool coop = per_frame || (coop_steps > 0 && short_launch(work, cfg.coop_tiles_per_wave, (long long)p.blocks * 4));
  // ODDITY: only the wide work-sharing build writes the log, but the threaded builds and the counting build of a short launch keep log_waves
  if (!wide) p.build = {cfg.count, occ, s.trav_min, s.park_min, s.unroll, false, true, false};
  else if (cfg.count) p.build = {true, occ, s.trav_min, s.park_min, s.unroll, true, false, false};
  else if (coop) p.build = {false, occ, s.trav_min, s.coop_park, s.coop_unroll, true, true, per_frame};
  else p.build = {false, occ, s.trav_min, s.park_min, s.unroll, true, false, false};
  if (wide && !coop) p.log_waves = 0;
  return p;
}

// Option sky_tiles: a launch may leave its sky tiles (entry code ENTRY_NONE) to a kernel of their own only in the lean build of the wide walk that adds
// a batch into one buffer -- the counting build keeps every pixel (its counters are the bench's metric), the work-sharing build and the per-frame
// stores are not split
inline bool plan_sky_split(const PersistentPlan& p) { return p.build.wide && !p.build.count && !p.build.coop && !p.build.perframe; }

// Option sky_tiles = 2: the lean build's waves render the sky tiles themselves once all their lanes have retired (kernels_render.hip), a unit at a time
// from a cursor.  A unit is a position in sky_list and a chunk of consecutive frames of the launch's batch: unit u is chunk u % chunks of list entry
// u / chunks, chunks = ceil(batch / chunk frames), the last chunk the shorter one.  `chunk` = frames per unit, 0 (or more than the batch): the whole
// batch, one unit per sky tile.  (constexpr: the kernel and the host build call the same functions.)
#ifndef DR_SKY_CHUNK
#define DR_SKY_CHUNK 0
#endif
constexpr int SKY_CHUNK = DR_SKY_CHUNK;
struct SkyUnit { int index, first, count; };      // position in sky_list, first frame of the batch, frames
constexpr int sky_chunk_frames(int batch, int chunk) { return chunk > 0 && chunk < batch ? chunk : (batch > 0 ? batch : 1); }
constexpr int sky_chunks(int batch, int chunk) { return batch > 0 ? (batch + sky_chunk_frames(batch, chunk) - 1) / sky_chunk_frames(batch, chunk) : 0; }
constexpr unsigned sky_units(unsigned n_sky, int batch, int chunk) { return n_sky * (unsigned)sky_chunks(batch, chunk); }
constexpr SkyUnit sky_unit(unsigned u, int batch, int chunk) {
  const unsigned chunks = (unsigned)sky_chunks(batch, chunk), index = u / chunks;
  const int frames = sky_chunk_frames(batch, chunk), first = (int)(u - index * chunks) * frames;
  return SkyUnit{(int)index, first, batch - first < frames ? batch - first : frames};
}

// Option sample_order: which of a tile's 64 x batch samples (pixel-in-tile p, frame f) share a unit of the queue.  A tile's units are
// numbered 0 .. batch - 1 and unit u hands out the sample indices j = 64 u + l, l = 0 .. 63, in ascending order.  Order 0: p = j % 64, f = j / 64 -- a
// unit is the tile's 64 pixels of one frame.  Order 1 (frame-minor): p = j / batch, f = j % batch -- a unit is consecutive frames of one or two pixels
// (of at most ceil(64 / batch) + 1).  Either is a bijection of [0, 64 batch) onto [0, 64) x [0, batch), and with batch = 1 the identity.
// The division by the batch is a multiply-high by sample_order_magic's word m = ceil(2^32 / batch): j m = (j / batch) 2^32 + rest with
// 0 <= rest < 2^32 as long as j (m batch - 2^32) < 2^32, and m batch - 2^32 < batch <= 256, j < 2^14.  ceil(2^32 / 1) does not fit a word: the word is
// 0 for batch 1 and for order 0, and 0 means order 0 (wave-uniform in the kernel).  (constexpr: the kernel and the host build call the same functions.)
constexpr int SAMPLE_ORDER_MAX_BATCH = 256;      // (dr_context's batch_frames ends there)
struct TileSample { int p, f; };
constexpr uint32_t sample_order_magic(int order, int batch) {
  return order == 1 && batch > 1 && batch <= SAMPLE_ORDER_MAX_BATCH ? (uint32_t)((0x100000000ull + (uint64_t)batch - 1ull) / (uint64_t)batch) : 0u;
}
constexpr TileSample tile_sample(uint32_t magic, int batch, int j) {
  if (magic == 0u) return TileSample{j & 63, j >> 6};
  const int p = (int)(uint32_t)(((uint64_t)(uint32_t)j * (uint64_t)magic) >> 32);
  return TileSample{p, j - p * batch};
}

// Tile queues of a launch of `tiles` tiles (batch_hint frames of them): one per XCD, or one
inline int plan_regions(int tiles, int batch_hint, bool xcd_regions, bool short_one_queue, int tiles_per_wave, int num_cus) {
  int regions = xcd_regions ? MAX_REGIONS : 1;
  if (tiles < 64 * MAX_REGIONS) regions = 1;                 // tiny frames: one queue
  // a short launch (few tiles per wave: one frame, or a thin stripe of a few) ends when its slowest band ends; one queue
  // balances better there than eight (1.88 instead of 2.00 ms for a single 1920x1080 frame of the bench scene)
  // ODDITY: five waves on every CU of the device: num_cus WITHOUT option reserve_cus taken off
  if (short_one_queue && short_launch((long long)tiles * batch_hint, tiles_per_wave, (long long)num_cus * 5 * 4)) regions = 1;
  return regions;
}

// ---- the queues' cursors.  Every launch takes a block of zeroed words out of a ring: a cursor per tile queue, `stride` words apart
// (the kernel adds to tile_counter[region * stride]), and in the block's last slot the sky units' cursor (option sky_tiles = 2).  Every wave of every
// XCD adds to these words with device-scope atomics, which are served where the word's line lives: cursors that share a line queue up behind each
// other, and how many of a packed block's nine words share one depended on the launch's number (profiles/queue_cursors_ab.txt).  With the default
// stride no two cursors share a 128-byte line.  The block is (MAX_REGIONS + 1) * stride words, and the blocks follow each other, so each is aligned
// to the stride.  Options: queue_cursor_stride (1: the packed layout) and queue_cursor_skew, a measuring aid: s > 0 starts every launch's block s
// words into a 128-byte line (the blocks' pitch is then rounded up to whole lines), which pins the alignment that a packed block otherwise gets
// from the launch's number.  (The skew is how profiles/queue_cursors_ab.txt showed the cause and that a strided block does not care where it
// starts; it is not for production use -- cursor_block_pitch's second arm serves it alone.)
// The ring: CURSOR_RING_LAUNCHES blocks, or as many as the allocation holds (stride 64: 113; stride 1024: 7).  Taking the block that no longer fits
// wraps: the whole allocation is cleared first (256 KiB, a few microseconds once per 128 launches) and the launch runs alone in the pipeline
// (pipeline_state.hpp group_plan).  The words from the cursor on are zero whatever layout the earlier blocks had, so an option may change between two
// launches: a cursor that is no multiple of the new pitch wraps, any other goes on.
constexpr int QUEUE_CURSOR_STRIDE = 32;                           // option queue_cursor_stride's default: a 128-byte line per cursor
constexpr int QUEUE_CURSOR_STRIDE_MAX = 1024;
constexpr int CURSOR_LINE_WORDS = 32;
constexpr int CURSOR_RING_LAUNCHES = 128;
constexpr int CURSOR_RING_ALLOC = 1 << 16;                        // words allocated (and cleared at a wrap)
constexpr int cursor_block_words(int stride) { return (MAX_REGIONS + 1) * stride; }
constexpr int cursor_sky_slot(int stride) { return MAX_REGIONS * stride; }      // the sky units' cursor: the block's last slot
constexpr int cursor_block_pitch(int stride, int skew) {
  return skew > 0 ? (skew + cursor_block_words(stride) + CURSOR_LINE_WORDS - 1) / CURSOR_LINE_WORDS * CURSOR_LINE_WORDS : cursor_block_words(stride);
}
constexpr int cursor_ring_blocks(int stride, int skew) {
  return CURSOR_RING_ALLOC / cursor_block_pitch(stride, skew) < CURSOR_RING_LAUNCHES ? CURSOR_RING_ALLOC / cursor_block_pitch(stride, skew) : CURSOR_RING_LAUNCHES;
}
static_assert(cursor_ring_blocks(QUEUE_CURSOR_STRIDE_MAX, CURSOR_LINE_WORDS - 1) >= 2, "the ring holds the widest block");
// The one rule "next block, and does taking it wrap the ring": `cursor` is where the previous launch's block ended
struct CursorTake { int block, next; bool wrap; };      // the launch's block (first word), the cursor behind it, the ring is cleared first
constexpr CursorTake cursor_take(int cursor, int stride, int skew) {
  const int pitch = cursor_block_pitch(stride, skew);
  const bool wrap = cursor < 0 || cursor % pitch != 0 || cursor + pitch > cursor_ring_blocks(stride, skew) * pitch;
  const int at = wrap ? 0 : cursor;
  return CursorTake{at + (skew > 0 ? skew : 0), at + pitch, wrap};
}

// Tile order: at most split_waves % of the waves start with a part of a split tile.  ODDITY: the device's num_cus again, and never six waves
inline int plan_split_limit(int num_cus, int occupancy, int split_parts, int split_waves) {
  return split_parts > 1 ? (int)((long long)num_cus * (occupancy >= 5 ? 5 : 4) * 4 * split_waves / (100 * split_parts)) : 0;
}

// ---- the queries on caller lists: one ray per lane in workgroups of 256, or -- where the query has one -- a persistent kernel whose waves take chunks
// of the list (device_list.hpp).  plan_ray_list decides for n > 0 rays: can_persist: the persistent kernel exists for this scene and traversal (it cannot
// be forced where it does not); force: the query's private option; min_rays: its measured cross-over; occ, chunk: the persistent kernel's waves per SIMD
// and rays per chunk -- no more waves than chunks.  The per-query constants and what they were measured on stay with each query below.
enum { QUERY_KERNEL_PLAIN = 0, QUERY_KERNEL_PERSISTENT = 1 };
enum { QUERY_FORCE_NONE = 0, QUERY_FORCE_PLAIN = 1, QUERY_FORCE_PERSISTENT = 2 };      // options "trace_kernel", "radiance_kernel", "allhits_kernel"
struct RayListPlan { int kernel, blocks; };      // QUERY_KERNEL_*, workgroups of 256 threads
inline RayListPlan plan_ray_list(long long n, bool can_persist, int force, long long min_rays, int occ, int chunk, int num_cus) {
  const bool persistent = can_persist && (force == QUERY_FORCE_PERSISTENT || (force != QUERY_FORCE_PLAIN && n >= min_rays));
  if (!persistent) return {QUERY_KERNEL_PLAIN, (int)((n + 255) / 256)};
  const long long full = (long long)num_cus * occ, need = (n + 4 * chunk - 1) / (4 * chunk);
  return {QUERY_KERNEL_PERSISTENT, (int)(need < full ? need : full)};
}

// ---- dr_trace_rays (kernels_trace.hip): which kernel walks a list of caller rays, and with what grid
// The persistent kernel's parameters are those of the trace-only probe's best variant (profiles/r4_j_trace_only_probe.txt, variant 2: six waves per
// SIMD, refill once 8 lanes are free, leaf steps for 20 lanes: 5.65 Grays/s against 4.91 for one ray per lane); it exists for the wide walk only.
// TRACE_PERSISTENT_MIN_RAYS is the measured cross-over (profiles/trace_rays_rate.txt, part c, a frame's rays of the bench scene in wavefront order):
// one ray per lane is faster up to 16.8 M rays (x 0.63 at 262 144, x 0.83 at 4.2 M, x 0.98 at 16.8 M), the persistent kernel from 49.3 M on
// (x 1.07, x 1.09 at 65.7 M; any-hit the same within 0.02); 2^25 lies between the two, near their geometric mean.  A grid of one-ray-per-lane
// workgroups refills itself, workgroup by workgroup; the persistent waves' refill rounds pay only once the list is long enough for its tail to matter.
constexpr int TRACE_OCC = 6, TRACE_REFILL_MIN = 8, TRACE_PARK = 20;
constexpr int TRACE_CHUNK = 128;                          // rays a wave takes from the list per atomic
constexpr long long TRACE_PERSISTENT_MIN_RAYS = 1 << 25;
struct TracePlan {
  int kernel;               // QUERY_KERNEL_*
  int traversal;            // the walk really used: a scene without a wide tree walks the threaded links
  int blocks;               // workgroups of 256 threads
};
// n > 0 rays; traversal: the context's; force: option "trace_kernel" (the persistent kernel cannot be forced where it does not exist)
inline TracePlan plan_trace(long long n, int traversal, bool has_wide, int num_cus, int force) {
  const int walk = (traversal == DR_TRAVERSAL_WIDE && !has_wide) ? DR_TRAVERSAL_THREADED : traversal;
  const RayListPlan l = plan_ray_list(n, walk == DR_TRAVERSAL_WIDE, force, TRACE_PERSISTENT_MIN_RAYS, TRACE_OCC, TRACE_CHUNK, num_cus);
  return {l.kernel, walk, l.blocks};
}

// ---- dr_trace_radiance (kernels_radiance.hip): which kernel path-traces a list of caller rays, and with what grid.  As plan_trace: the persistent
// kernel exists for the wide walk only, and cannot be forced where it does not exist.  Its chunk is half the trace kernel's: a ray here is a whole
// path (spp samples of up to max_depth walks), so a wave's last chunk weighs more than the atomics saved.
// RADIANCE_PERSISTENT_MIN_RAYS is the measured cross-over (profiles/radiance_rate.txt, parts b and d; bench scene, spp 1, depth 10; one ray per lane
// against persistent): camera rays x 0.61 at 2^16, x 0.93 at 2^20, x 1.01 at 2^22, x 1.10 at 2^24; rays that start on the surfaces x 0.89, x 0.99,
// x 1.51 (2.70 -> 1.79 ms), x 1.84 (8.32 -> 4.51 ms).  The phase at 32 waiting lanes (the render kernel's TRAV_MIN) rather than the trace kernel's 8:
// a phase here shades, and 2^24 camera rays took 5.66 ms against 6.30 at 8.
constexpr int RADIANCE_OCC = 5, RADIANCE_REFILL_MIN = 32, RADIANCE_PARK = 20;
constexpr int RADIANCE_CHUNK = 64;                        // rays a wave takes from the list per atomic
constexpr long long RADIANCE_PERSISTENT_MIN_RAYS = 1 << 22;
struct RadiancePlan {
  int kernel;               // QUERY_KERNEL_*
  int traversal;            // the walk really used: a scene without a wide tree walks the threaded links
  int blocks;               // workgroups of 256 threads
};
// n > 0 rays; traversal: the context's; force: option "radiance_kernel"
inline RadiancePlan plan_radiance(long long n, int traversal, bool has_wide, int num_cus, int force) {
  const int walk = (traversal == DR_TRAVERSAL_WIDE && !has_wide) ? DR_TRAVERSAL_THREADED : traversal;
  const RayListPlan l = plan_ray_list(n, walk == DR_TRAVERSAL_WIDE, force, RADIANCE_PERSISTENT_MIN_RAYS, RADIANCE_OCC, RADIANCE_CHUNK, num_cus);
  return {l.kernel, walk, l.blocks};
}

// ---- dr_query_nearest (kernels_nearest.hip): one query per lane, workgroups of 256; the 4-way records where the scene has them, else the threaded links
struct NearestPlan {
  bool wide;
  int blocks;
};
inline NearestPlan plan_nearest(long long n, bool has_wide) {      // n > 0 queries
  NearestPlan p;
  p.wide = has_wide;
  p.blocks = (int)((n + 255) / 256);
  return p;
}

// ---- dr_trace_all_hits (kernels_allhits.hip): which kernel walks a list of caller rays for all their crossings, and with what grid.  A scene with a
// wide tree is walked through it whatever the traversal option says (plan_nearest's rule); the persistent kernel exists for that walk only and cannot be
// forced where it does not exist.  Its parameters are the trace kernel's, but five waves per SIMD: a workgroup holds 32 KiB of LDS, the lanes' stacks
// and their lists.  ALLHITS_PERSISTENT_MIN_RAYS is the measured cross-over (profiles/allhits_rate.txt, part c; a frame's rays of the bench scene in
// wavefront order, K = 4): one ray per lane is faster up to 3.3 M rays (x 0.51 at 262 144, x 0.69 at 1.0 M, x 0.86 at 3.3 M), the persistent kernel
// from 13.1 M on (x 1.22, x 1.40 at 52.5 M; the count alone x 1.34, x 1.58); 2^23 lies between the two, near their geometric mean.
constexpr int ALLHITS_OCC = 5, ALLHITS_REFILL_MIN = 8, ALLHITS_PARK = 20;
constexpr int ALLHITS_CHUNK = 128;                        // rays a wave takes from the list per atomic
constexpr long long ALLHITS_PERSISTENT_MIN_RAYS = 1 << 23;
struct AllHitsPlan {
  int kernel;               // QUERY_KERNEL_*
  bool wide;                // the 4-way records, else the threaded links
  int blocks;               // workgroups of 256 threads
};
// n > 0 rays; force: option "allhits_kernel"
inline AllHitsPlan plan_allhits(long long n, bool has_wide, int num_cus, int force) {
  const RayListPlan l = plan_ray_list(n, has_wide, force, ALLHITS_PERSISTENT_MIN_RAYS, ALLHITS_OCC, ALLHITS_CHUNK, num_cus);
  return {l.kernel, has_wide, l.blocks};
}

}  // namespace dr
