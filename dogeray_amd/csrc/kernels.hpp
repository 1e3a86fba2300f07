// Launchers of the device code, one translation unit per family of kernels:
//   kernels_render.hip        the per-tile kernel (reference launch shape) and the persistent kernel (waves as pools of 64 path slots)
//   kernels_aux.hip           tile-order feedback, the split of a launch's order, the sky tiles' kernel, present divide, stripe copies of the multi-GPU gather, gather probe, trace-only probe
//   kernels_kat.hip           known-answer kernels behind dr_kat_*: generator, intersections, optics, normal, closest hit; the shading step
//   kernels_aov.hip           first-hit AOV buffers of a window of pinhole camera rays (dr_render_aov)
//   kernels_trace.hip         closest hit and occlusion of caller rays (dr_trace_rays)
//   kernels_radiance.hip      path-traced radiance along caller rays (dr_trace_radiance)
//   kernels_nearest.hip       nearest-surface point queries (dr_query_nearest)
//   kernels_allhits.hip       every crossing of a caller ray, the first K sorted (dr_trace_all_hits)
//   kernels_denoise.hip       the AOV-guided a-trous denoiser of the accumulator (dr_accum_denoise)
//   kernels_reproject.hip     temporal reprojection of the accumulator and its history plane into another view (dr_accum_reproject)
//   kernels_upscale.hip       the AOV-guided upsampler of a low-resolution accumulator (dr_accum_upscale)
//   kernels_moments.hip       the second-moment plane: the fused frame add and the per-pixel noise estimate (option "moments", dr_accum_error)
//   kernels_adaptive.hip      adaptive sampling: the tiles that ask for samples, the masked fold (dr_render_adaptive)
// (the measured-slower kernels of rounds 2 and 3 -- two paths per lane, waves with roles, the pool kernel -- are archived under tools/experiments/)
// context.cpp and the context_*.cpp files (host only: resident scene, options, the C ABI) call these and never see a kernel.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include "device_launch.h"
#include "device_layout.h"
#include "launch_plan.hpp"

namespace dr {

// kernels_render.hip
void launch_tile_kernel(hipStream_t stream, const RenderParams& P, int traversal, bool count, int occupancy);
// launches the build plan_persistent (launch_plan.hpp) picks; returns the plan's log_waves, or -1: the plan names a build that is not instantiated
// (tile_counter, cursor_stride: the launch's block of queue cursors, zero, and the words between two of them -- launch_plan.hpp cursor_take)
int launch_persistent_kernel(hipStream_t stream, const RenderParams& P, const PersistentCfg& cfg, unsigned* tile_counter, int cursor_stride, const int* order,
                             const int* region_start, unsigned* pixel_cost);

// The 64-bit words of a context's statistics buffer (RenderParams counters).  The render kernels write them, context.cpp reads them
// (dr_stats_get: words [0, STAT_PHASE); dr_stats_phase_counts: the words from STAT_PHASE on), context_probe.cpp sets the ray log's.
enum StatWord {
  STAT_RAYS = 0, STAT_NODE_VISITS, STAT_PRIM_TESTS, STAT_SHADES, STAT_TEXELS, STAT_SAMPLES, STAT_TRAV_SLOTS, STAT_RAY_SLOTS,      // the ray counters, in the order of Ctr
  STAT_DIAG = 8,               // dr_stats.diag[0 .. 8): the persistent kernel's, summed over its waves
  STAT_WAVE_CYCLES = STAT_DIAG, STAT_PHASE_CYCLES, STAT_ITERATIONS, STAT_PHASES, STAT_NODE_STEPS, STAT_LEAF_STEPS, STAT_SHADED,
  STAT_WAVE_TICKS,             // wave lifetime in 100 MHz ticks (every build, as STAT_WAVE_CYCLES; the six between them: counting build)
  STAT_PHASE = 16,             // the shade / refill phase's budget (counting build):
  STAT_TURN_HIST = STAT_PHASE, // histogram of the rejection loop's turns per phase, STAT_TURN_BINS bins (the last: that many or more)
  STAT_PB_CANDS = 32, STAT_PB_TURNS, STAT_PB_SPHERE, STAT_PB_DISK, STAT_PB_RETIRED,      // candidates drawn, turns run, sphere / disk lanes, retired lanes over phases
  STAT_LOG_RAYS = 40, STAT_LOG_PTR, STAT_LOG_ROOM      // measurement aid (dr_context_probe_trace): rays logged, the log's address, its room in entries
};
constexpr int STAT_TURN_BINS = 16;
constexpr int COUNTER_WORDS = 48;
static_assert(STAT_TURN_HIST + STAT_TURN_BINS <= STAT_PB_CANDS && STAT_LOG_ROOM < COUNTER_WORDS, "statistics words");

// kernels_aux.hip
void launch_tile_feedback(hipStream_t stream, const unsigned* pixel_cost, unsigned* tile_cost, int* tile_order, int* region_start, int tiles, int regions,
                          int heavy_factor, int split_steps, int split_limit);
// the camera rays' grazing certificate of a view: mask = (ntiles + 31) / 32 words of tile bits (set: the tile's camera rays keep the scene's margin),
// then the "every tile" word, the number of flagged tiles and cv.n_levels scratch planes (cert_mask_words in all); level = a byte per tile, the tile's
// grade on cv's ladder, cert_level_words words (device_cert.hpp cert_leaf)
inline size_t cert_mask_words(int ntiles, int n_levels) { return (size_t)((ntiles + 31) / 32) * (size_t)(1 + n_levels) + 2; }
inline size_t cert_level_words(int ntiles) { return (size_t)((ntiles + 31) / 32) * 8; }
void launch_cert_mask(hipStream_t stream, const DevPrim* prims, int n, const CertView& cv, uint32_t* mask, uint32_t* level, int ntiles);
// the camera rays' entry table of that view (option camera_entry): mm = entry_mm_words words of scratch, or null (every tile at the root); word = a word
// per tile, its entry code << 3 | its grade from `level` (what the render kernel reads: RenderParams cert_level); leaf_rec / range: the wide tree's
// side arrays (linearise.hpp)
inline size_t entry_mm_words(int ntiles) { return 2 * (size_t)ntiles + 1; }
void launch_camera_entry(hipStream_t stream, const DevUnit* wide, const uint32_t* leaf_rec, const uint32_t* range, int n_leaves, const CertView& cv,
                         uint32_t* mm, const uint32_t* level, uint32_t* word, int ntiles);
// The split of a launch's order (device_split.hpp order_split_plain describes the arrays) -- order / region_start as the persistent kernel would take
// them (order null: the identity, regions from own_region_start, MAX_REGIONS + 1 ints on the host) -- into launch_order / launch_region_start for the
// persistent kernel.  kind SPLIT_BY_WORD (option sky_tiles): key = the tiles' words (uint32_t), a sky tile is dropped; dropped_list with counts ([0] sky
// tiles, [1] geometry tiles) are written for launch_sky_tiles.  kind SPLIT_BY_FLAG (dr_render_adaptive): key = a flag per tile (uint8_t), a tile without
// one is dropped; no list, no counts (both may be null), launch_adaptive_add reads the pair behind the launch.  One 1 024-thread workgroup
enum SplitKind { SPLIT_BY_WORD = 0, SPLIT_BY_FLAG = 1 };
void launch_order_split(hipStream_t stream, int kind, const int* order, const int* region_start, const int* own_region_start, const void* key, int tiles,
                        int regions, int* launch_order, int* launch_region_start, int* dropped_list, unsigned* counts);
// renders P.batch frames of the listed sky tiles (one wave per tile; pixel_cost non-null: their costs, 0)
void launch_sky_tiles(hipStream_t stream, const RenderParams& P, const int* sky_list, const unsigned* counts, unsigned* pixel_cost);
// hist: the history plane (int32 per pixel at x * H + y; the divisor of pixel p is hist[p] + div, a divisor of 0 gives 0), or null: acc / div
void launch_present(hipStream_t stream, const int32_t* acc, const int32_t* hist, uint8_t* rgb, int W, int H, int div);
void launch_frame_add(hipStream_t stream, int32_t* acc, const int32_t* frame, size_t n);      // acc += frame (pipelined single frames)
void launch_stripe_copy(hipStream_t stream, int32_t* dst, const int32_t* src, int ncols, int run4, long long dst_first4, long long dst_stride4,
                        long long src_first4, long long src_stride4);
void launch_gather_probe(hipStream_t stream, const RenderParams& P, int blocks, unsigned nrec, int iters, unsigned* out);
// trace-only probe (dr_context_probe_trace): variant 0 = one ray per lane, waves wait for their slowest; 1.. = persistent waves refilling from the ray list
// (occupancy / lanes that must be free before a refill / lanes at a leaf before a leaf step: 6/1/20, 6/8/20, 6/16/20, 8/8/20, 8/8/28, 6/8/28, 8/4/32)
void launch_trace_probe(hipStream_t stream, const RenderParams& P, int num_cus, int variant, const float* rays, unsigned n, unsigned* cursor, unsigned* out);

// kernels_kat.hip: one element per lane
void launch_kat_rng(hipStream_t stream, uint64_t seed, int n, double* out);
void launch_kat_aabb(hipStream_t stream, int n, const float* o, const float* d, const float* mn, const float* mx, int32_t* hit, float* dist);
void launch_kat_node_planes(hipStream_t stream, int n, const uint32_t* w, const float* a, const float* b, float* t_mix, float* t_cvt);
void launch_kat_tri(hipStream_t stream, int n, const float* o, const float* d, const float* v0, const float* v1, const float* v2, float* t);
void launch_kat_sphere(hipStream_t stream, int n, const float* o, const float* d, const float* c, const float* r, float* t);
void launch_kat_optics(hipStream_t stream, int n, const float* v, const float* nrm, const float* eta, float* refl, float* refr, float* sch);
void launch_kat_normal(hipStream_t stream, const RenderParams& P, int n, const int32_t* slot, const float* o, const float* d, const float* t, float* nrm, float* texco);
void launch_kat_hit(hipStream_t stream, const RenderParams& P, int traversal, int n, const float* o, const float* d, float* t, int32_t* slot, int32_t* visits);
// the shading step's (device_kat_shade.hpp says what each writes; "2": both forms, form f of element i at f * n + i)
void launch_kat_sample(hipStream_t stream, int n, const uint64_t* seed, const int32_t* warm, const int32_t* kind, float* p_plain, uint32_t* n_plain,
                       float* p_merged, uint32_t* n_merged);
void launch_kat_outside(hipStream_t stream, int n, const float* d2, int32_t* out);
void launch_kat_tex(hipStream_t stream, const RenderParams& P, int n, const int32_t* tex, const float* u, const float* v, uint32_t* rgba);
void launch_kat_bounce(hipStream_t stream, const RenderParams& P, int n, const int32_t* slot, const float* o, const float* d, const float* t,
                       const float* atten, const uint64_t* seed, const int32_t* warm, int32_t* alive2, float* o2, float* d2, float* atten2,
                       uint32_t* next2);
void launch_kat_miss(hipStream_t stream, const RenderParams& P, int n, const float* d, const float* atten, float* rgb);
void launch_kat_camera(hipStream_t stream, const RenderParams& P, int n, const int32_t* x, const int32_t* y, const int32_t* s, float* origin2,
                       float* dir2, uint32_t* next2);
void launch_kat_store(hipStream_t stream, const RenderParams& P, int n, const float* color);      // into P.out, pixel (i, 0) of an n x 1 frame
// the stores of n / 64 whole waves into the P.W x P.H accumulator P.out (P.accumulate 2) -- form 0 store_pixel, 1 store_pixels_merged, 2 store_pixels_merged_lds;
// lds_in / lds_out: KAT_MERGE_ROWS rows of 64 LDS words per wave, before and after (rows 1 .. 5 the slot rows)
constexpr int KAT_MERGE_ROWS = 7;
void launch_kat_store_merged(hipStream_t stream, const RenderParams& P, int form, int n, const int32_t* store_me, const int32_t* key, const int32_t* x,
                             const int32_t* y, const float* color, const int32_t* lds_in, int32_t* lds_out);

// kernels_aov.hip: the window (x0, y0, w, h) of the pixel grid and the channels to write (null: not written), each a row-major w x h plane
// (pixel (x, y) at (y - y0) * w + (x - x0); normal / albedo / dir 3 floats per pixel, uv 2)
struct AovLaunch {
  int x0, y0, w, h;
  float focus;                    // settings13[7]
  const int32_t* slot_to_orig;    // slot -> object index of the file
  float* t; float* distance; float* depth;
  int32_t* object; int32_t* material;
  float* normal; float* uv; float* albedo; float* dir;
};
void launch_aov(hipStream_t stream, const RenderParams& P, int traversal, const AovLaunch& A);
// ... and the lens-averaged channels of the same window (dr_render_aov_lens; device_aov_lens.hpp): N = nframes * spp samples per pixel, 1 .. AOV_LENS_MAX,
// with P.seed the frame seed and P.batch_seed_stride the stride between frames.  loop: AOV_LENS_NESTED the plain nested loop (the faster one as
// measured, DESIGN.md 4.22: the default), AOV_LENS_REFILL the refilling walk loop (private option aov_lens_loop: the A/B; the same bits)
constexpr int AOV_LENS_MAX = 256;
constexpr int AOV_LENS_NESTED = 0, AOV_LENS_REFILL = 1;
struct AovLensLaunch {
  int x0, y0, w, h;
  float focus;                    // settings13[7]
  int nframes, spp;
  int as_guides;                  // trace_guides' form: a pixel whose material is -1 a miss in every channel, albedo + (1 - coverage)
  float* coverage; float* depth; float* distance;
  int32_t* material;
  float* normal; float* albedo;
};
void launch_aov_lens(hipStream_t stream, const RenderParams& P, int traversal, int loop, const AovLensLaunch& A);

// kernels_trace.hip: n caller rays (origin / dir 3 floats per ray, tmax one or null: every ray 10000) and what to write per ray (null: not written).
// The trace kernel writes t (-1: miss), object (slot_to_orig of the slot, -1: miss), occluded (1 / 0) and hit -- {t bits, slot}, miss {-1, -1}: what
// the surface pass reads --; launch_trace_surface maps (origin, dir, hit) to distance, material, normal, uv, albedo (dr_render_aov's channels)
struct TraceLaunch {
  const float* origin; const float* dir; const float* tmax;
  unsigned n;
  const int32_t* slot_to_orig;
  float* t; int32_t* object; int32_t* occluded;
  uint32_t* hit;                  // two words per ray
  unsigned* cursor;               // persistent kernel: the ray list's cursor, zeroed on the launch's stream by the caller
  float* distance; int32_t* material; float* normal; float* uv; float* albedo;
};
// any: DR_TRACE_ANY; plan: plan_trace's (launch_plan.hpp).  n > 0.
void launch_trace(hipStream_t stream, const RenderParams& P, const TracePlan& plan, bool any, const TraceLaunch& T);
void launch_trace_surface(hipStream_t stream, const RenderParams& P, const TraceLaunch& T);

// kernels_allhits.hip (dr_trace_all_hits): n caller rays as TraceLaunch's, the list length K = max_hits (0 .. DR_ALLHITS_MAX) and the kinds that count.
// The walk kernel writes count (n), t and object (n * K; unused entries -1) and hit -- {t bits, slot} per entry, unused {-1, -1}: what the surface
// pass reads --; launch_allhits_surface, one thread per entry, maps (origin, dir, hit) to distance, material, normal, uv, albedo.  Null: not written.
struct AllHitsLaunch {
  const float* origin; const float* dir; const float* tmax;
  unsigned n;
  int K, kind_mask;
  const int32_t* slot_to_orig;
  int32_t* count; float* t; int32_t* object;
  uint32_t* hit;                  // two words per entry
  unsigned* cursor;               // persistent kernel: the ray list's cursor, zeroed on the launch's stream by the caller
  float* distance; int32_t* material; float* normal; float* uv; float* albedo;
};
// plan: plan_allhits' (launch_plan.hpp).  n > 0; the surface pass needs K > 0.
void launch_allhits(hipStream_t stream, const RenderParams& P, const AllHitsPlan& plan, const AllHitsLaunch& A);
void launch_allhits_surface(hipStream_t stream, const RenderParams& P, const AllHitsLaunch& A);

// kernels_radiance.hip: R (RadianceLaunch, device_launch.h) by the kernel of plan (plan_radiance's, launch_plan.hpp); P: the scene, max_depth, bgint,
// backtex.  n > 0; the persistent kernel's cursor zeroed on `stream` by the caller.
void launch_radiance(hipStream_t stream, const RenderParams& P, const RadiancePlan& plan, const RadianceLaunch& R);

// kernels_nearest.hip: N (NearestLaunch, device_launch.h) by the walk of plan (plan_nearest's, launch_plan.hpp): the walk kernel writes N.key, d2,
// distance, object; the finishing pass reads N.key and writes material, qpoint, uv.  n > 0.
void launch_nearest(hipStream_t stream, const RenderParams& P, const NearestPlan& plan, const NearestLaunch& N);
void launch_nearest_finish(hipStream_t stream, const RenderParams& P, const NearestPlan& plan, const NearestLaunch& N);

// The accumulator stages: their launch structs (DnLaunch, UpLaunch, RpLaunch, MoLaunch) are in device_launch.h, without HIP, because the per-pixel
// bodies of the device_*.hpp headers and the host build take them too
// kernels_denoise.hip
void launch_denoise_guides(hipStream_t stream, const DnLaunch& L);                 // normal, depth, mat -> guide, gz
void launch_denoise_colour(hipStream_t stream, const DnLaunch& L, int stage);      // 0: acc -> (e, l) in dst; 1: src (e, l) -> (e, var) in dst
void launch_denoise_pass(hipStream_t stream, const DnLaunch& L, int step, int lattice);   // src -> dst, one a-trous iteration
void launch_denoise_finish(hipStream_t stream, const DnLaunch& L);                 // src (or, iterations 0, acc) -> out_f32 / out_rgb8

// kernels_upscale.hip
void launch_upscale(hipStream_t stream, const UpLaunch& L);

// kernels_reproject.hip
void launch_reproject(hipStream_t stream, const RpLaunch& L);

// kernels_moments.hip
// acc += frame and m2 += the frame's capped luma squared, in one pass (npix pixels; acc / frame column-major x 3, m2 one word per pixel)
void launch_moments_add(hipStream_t stream, int32_t* acc, const int32_t* frame, unsigned long long* m2, size_t npix);
void launch_moments_error(hipStream_t stream, const MoLaunch& L);

// kernels_adaptive.hip (dr_render_adaptive; device_adaptive.hpp describes the arrays)
void launch_adaptive_select(hipStream_t stream, const AdLaunch& L);      // the planes -> L.flags, L.counts
// L.nframes frame buffers into the planes of the launch_region_start[regions] tiles at the head of launch_order
void launch_adaptive_add(hipStream_t stream, const AdLaunch& L, const int* launch_order, const int* launch_region_start, int regions);

}  // namespace dr
