// The render kernels: the per-tile kernel (the reference's launch shape, kernel.cu K:2634-2640) and the persistent kernel (a wave is a
// pool of 64 path slots that refill from tile queues).  Launchers at the end; context.cpp picks options, launch_plan.hpp picks the instantiation.
#include <hip/hip_runtime.h>

#include "device_core.hpp"
#include "device_coop.hpp"
#include "device_sky.hpp"
#include "kernels.hpp"
#include "../../include/dogeray_amd.h"

namespace dr {

// ------------------------------------------------------------------ kernels
// One wave = one 8x8 pixel tile, as in the reference launch (K:2634-2640: block (8,8)); four
// tiles per 256-thread workgroup.  Tiles are numbered column-major over the block columns this
// context owns, so neighbouring waves work on vertically adjacent tiles (coherent rays, and the
// column-major framebuffer gives each wave eight 96-byte runs).
template <bool COUNT, int MODE, int OCC>
__global__ __launch_bounds__(256, OCC) void render_kernel(RenderParams P) {
  __shared__ int lds_stack[MODE == DR_TRAVERSAL_ORDERED ? ORDERED_STACK * 256 : (MODE == DR_TRAVERSAL_WIDE ? WIDE_STACK * 256 : 1)];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int tile = blockIdx.x * 4 + wave;
  Ctr c = {0, 0, 0, 0, 0, 0, 0, 0};
  if (tile < P.ncols * P.gy) {
    const int col = tile / P.gy, by = tile - col * P.gy;
    const int bx = P.stripe_rem + col * P.stripe_mod;
    const int x = bx * 8 + (lane >> 3), y = by * 8 + (lane & 7);
    if (MODE == DR_TRAVERSAL_ORDERED) {
      int* stack = lds_stack + wave * (ORDERED_STACK * 64) + lane;
      auto closest = [&](V3 o, V3 d, Ctr& cc) { return closest_hit_ordered<COUNT>(P.pairs, P.prims, o, d, cc, stack); };
      render_pixel<COUNT>(P, closest, x, y, c);
    } else if (MODE == DR_TRAVERSAL_WIDE) {
      const WalkRsrc wide = wide_rsrc(P);
      int* stack = lds_stack + wave * (WIDE_STACK * 64) + lane;
      auto closest = [&](V3 o, V3 d, Ctr& cc) { return closest_hit_wide<COUNT>(wide, P.wide_pmax, P.wide_mu.e, P.wide_mu.l, P.wide_mu.v, o, d, cc, stack); };
      render_pixel<COUNT>(P, closest, x, y, c);
    } else {
      const WalkRsrc walk = walk_rsrc(P);
      auto closest = [&](V3 o, V3 d, Ctr& cc) { return closest_hit_threaded<COUNT>(walk, o, d, cc); };
      render_pixel<COUNT>(P, closest, x, y, c);
    }
  }
  if (COUNT) {
    unsigned v[8] = {c.rays, c.V, c.L, c.S, c.T, c.samples, c.trav_slots, c.ray_slots};
    for (int k = 0; k < 8; k++) {
      unsigned long long s = v[k];
      for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
      if (lane == 0 && s) atomicAdd(&P.counters[STAT_RAYS + k], s);
    }
  }
}

// Persistent variant of the same megakernel.
//
// In the per-tile kernel above a wave's 64 lanes walk the BVH in lock step until the LAST of
// them is done, then shade, then walk again: on the 1M-triangle bench scene only 36 % of the
// lane-slots of the node loop and 77 % of the bounce loop do useful work.  Here a wave is a
// pool of 64 path slots.  Every loop iteration advances each walking lane by one node; as soon
// as fewer than TRAV_MIN lanes are still walking, the finished lanes are shaded (hit or miss),
// scatter into their next ray, or -- when their path has ended -- store their pixel and take the
// next unrendered pixel, so the node loop stays full until the frame runs out of pixels.
// Pixels are handed out in 8x8 tiles from per-XCD queues (one atomicAdd per tile), lane l of a tile is
// pixel (l >> 3, l & 7) of that tile: which lane renders a pixel does not enter its arithmetic (the RNG
// seed is a function of x, y and the frame, K:1065), so the frame is identical to the per-tile kernel's.
//
// lane states (kept in `tr.node`): >= 0 walking; LANE_DONE walk finished, needs shading; LANE_REFILL needs a new
// sample or pixel; LANE_RETIRED (device_walk.hpp).
// WIDE: the lanes walk the 4-way tree (wide_node_step / wide_leaf_step) instead of the threaded links.  A lane whose
// next record is a leaf waits until PARK_MIN lanes have one (the leaf step -- exact box + triangle -- is the long
// block, as the parked triangle test is in the threaded walk); its stack lives in the first WIDE_STACK words of
// the wave's LDS region, the phase stash behind it.
// COOP (wide walk): build with work sharing (lanes without a pixel take over subtrees of the rays still walking: once the queue is
// empty, and from the start in the waves that hold a part of a split tile).  It costs registers (96 VGPRs: five waves per SIMD) and
// code in the loop, so launches whose queue is long enough to hide their tail use the lean build (80 VGPRs and 26 KiB of LDS at
// OCC = 6: six waves per SIMD; launch_plan.hpp plan_persistent picks).

// ---- the persistent kernel's words, by name
// A pixel's code: tile * 64 + lane-in-tile, with the sign bit set for a pixel of a split tile (its wave holds while it lives)
constexpr int PCODE_SPLIT = (int)0x80000000, PCODE_MASK = 0x7fffffff;
// `share` of a lane (WIDE && COOP): negative = it walks a ray of its own, alone; 0 .. 63 = it helps that lane's ray (the owner); SHARE_OWNER = its own ray has helpers
constexpr int SHARE_ALONE = -1, SHARE_OWNER = 64;
// The phase stash: LDS words of a lane, word k at st[k * 64], that hold what the shade / refill phase does not need while it runs and -- WIDE -- what only
// the phase needs while the wave walks.
//  WIDE (WIDE_STASH words per lane behind the lane's WIDE_STACK stack words; 26 KiB of LDS per workgroup with the stack: six workgroups per CU):
//   * WS_TOP, the stack-pointer byte of WS_W1, WS_STEPS and (work-sharing build) WS_RSTART are the walk's state: stashed at the start of a phase, restored at
//     its end.  The lean build keeps no rstart (the ray's first step is of no use to it): its word is WS_BOUNCE, where the bounce count LIVES;
//   * the rest is needed in the phase only and LIVES here -- colour, x + 1 (0: no pixel) with y (make_params bounds the frame size), pixel code, sample, and in
//     the upper half of WS_W1 the frame of the batch: registers only between the read after shading and the write at the end of the phase (the walk loop has
//     eight registers more for the node step);
//   * byte 1 of WS_W1 (lean build) is the certificate's grade of the lane's ray: its tile's for a camera ray, 0 for any other; written with every new ray, read
//     with the stack pointer at the restore;
//   * between phases WS_STEPS and WS_RSTART are in registers, so the work sharing's exchange has those 2 * 64 words to itself: XCH_MAX hand-overs of XCH_FIELDS
//     words per round, field f of hand-over e at xch[f * XCH_MAX + e];
//   * between phases WS_TOP and WS_STEPS of the lean build (HIT_UV_CARRIED) carry the barycentrics u, v of the lane's best hit: the leaf step writes them
//     with every hit it accepts (device_wide.hpp wide_leaf_compute_uv), the phase reads them before it stashes the stack top and the step count there and puts
//     them back for the lanes that go on walking: v after shading, when the step count is a register again, u at the restore (in between it waits in
//     WS_COLOR_X, whose value is a register for that time).  Only a lane that shades a triangle hit
//     looks at them, so a new ray clears nothing.
//  Threaded walk (WAVE_LDS_DWORDS / 64 words per lane): the parked leaf, 1/direction, and -- not needed while the hit is shaded, back right after -- the pixel
//  bookkeeping; everything is stashed at the start of a phase and restored in it.
enum WideStashWord { WS_TOP = 0, WS_W1, WS_COLOR_X, WS_COLOR_Y, WS_COLOR_Z, WS_XY, WS_PCODE, WS_SAMPLE, WS_STEPS, WS_RSTART, WS_BOUNCE = WS_RSTART };
constexpr int WS_W1_SP_BYTE = 0, WS_W1_GRADE_BYTE = 1, WS_W1_FRAME_HALF = 1;      // WS_W1's fields, as indices of its bytes / half-words
constexpr int XCH_OFF = (WIDE_STACK + WS_STEPS) * 64, XCH_MAX = 16, XCH_FIELDS = 8;
enum XchField { XCH_OX = 0, XCH_OY, XCH_OZ, XCH_DX, XCH_DY, XCH_DZ, XCH_WORD, XCH_ROOT };      // the ray, the stack word handed over, the lane whose pixel the ray belongs to
static_assert(WS_RSTART + 1 == WIDE_STASH && XCH_MAX * XCH_FIELDS == (WIDE_STASH - WS_STEPS) * 64 && XCH_ROOT + 1 == XCH_FIELDS, "stash layout");
enum ThreadedStashWord { TS_V0X = 0, TS_C, TS_D = TS_C + 4, TS_INFO = TS_D + 4, TS_PARKED, TS_INV_X, TS_INV_Y, TS_INV_Z, TS_COLOR_X, TS_COLOR_Y, TS_COLOR_Z, TS_PX, TS_PY,
                         TS_PCODE, TS_FRAME, TS_SAMPLE, TS_STEPS, TS_RSTART, TS_WORDS };
static_assert(TS_WORDS * 64 == WAVE_LDS_DWORDS, "stash layout");

// The launch's sky units, taken from its cursor until none is left (option sky_tiles = 2; the end of render_persistent_kernel).  A function of its own
// that reads the launch's constants from the kernel's argument block: inlined -- against P, or against a copy read afresh -- the block changes the
// register allocation of the whole kernel and the launch's bulk runs 4.6 % slower (profiles/sky_inline_ab.txt).
typedef const __attribute__((address_space(4))) RenderParams* ArgBlock;
__device__ __attribute__((noinline)) void sky_units_run(ArgBlock args, int lane, unsigned* pixel_cost) {
#if defined(__HIP_DEVICE_COMPILE__)      // (the host pass has no copy out of the argument block's address space, and no use for the body)
  if (args->sky_list == nullptr) return;
  const RenderParams S = *args;
  const unsigned n_units = sky_units(S.sky_counts[0], S.batch, S.sky_chunk);
  __builtin_amdgcn_s_setprio(0);      // below the waves that still walk (the top of the kernel)
  for (;;) {
    unsigned u = 0;
    if (lane == 0) u = atomicAdd(S.sky_cursor, 1u);
    u = (unsigned)__builtin_amdgcn_readfirstlane((int)u);
    if (u >= n_units) break;
    const SkyUnit su = sky_unit(u, S.batch, S.sky_chunk);
    sky_tile_frames(S, S.sky_list[su.index], lane, su.first, su.count, pixel_cost);
  }
#endif
}

// PERFRAME: every frame of the launch's batch is stored into a buffer of its own (P.out + frame * P.out_frame_stride) instead of being added into one: the
// grouped present pipeline (dr_pipeline_*: the frames of a group share one launch and are added and shown one by one afterwards).
template <bool COUNT, int OCC, int TRAV_MIN, int PARK_MIN, int P_UNROLL, bool WIDE, bool COOP = true, bool PERFRAME = false>
__global__ __launch_bounds__(256, OCC) void render_persistent_kernel(RenderParams P, unsigned* __restrict__ tile_counter,
                                                                     const int* __restrict__ tile_order, const int* __restrict__ region_start,
                                                                     unsigned* __restrict__ pixel_cost, int cursor_stride) {
  const int lane = threadIdx.x & 63;
  const int wave_id = blockIdx.x * 4 + (threadIdx.x >> 6);
  // a launch whose retiring waves render its sky tiles (sky_units_run, at the end): the waves walk at priority 1 and drop to 0 for the sky units.  The
  // launch lasts as long as its slowest wave, and a SIMD's issue slots go to the higher priority first: at equal priority the sky units beside a
  // straggler slow it down and the launch gains nothing (profiles/sky_inline_ab.txt).  (wave-uniform: a kernel argument)
  if (WIDE && !COOP && !COUNT && !PERFRAME && P.sky_list != nullptr) __builtin_amdgcn_s_setprio(1);
  // LDS per wave (threaded walk: 6 KiB; wide walk: 6.5 KiB, 7.25 with work sharing), used for two things that never overlap in time
  // within a wave:
  //  * during the shade/refill phase, the state that phase does not need (threaded walk: the parked leaf, 1/direction; and while a
  //    hit is shaded also the pixel bookkeeping) waits here -- the shading code is where register pressure peaks, and this keeps
  //    the kernel within the VGPRs of its occupancy;
  //  * outside the phase, the node stack of the threaded walk's cooperative drain (COOP_STACK entries) / the exchange words of
  //    the wide walk's work sharing.  The wide walk's own stack (WIDE_STACK words per lane) sits in front of the stash.
  // WIDE && COOP: three more words per lane behind the stash -- the shared best hit (64-bit key) and the number of helper lanes of
  // a ray whose subtrees have been handed out (drain phase, below)
  constexpr int SHARE_OFF = (WIDE_STACK + WIDE_STASH) * 64;
  constexpr int REGION = WIDE ? (WIDE_STACK + WIDE_STASH + (COOP ? 3 : 0)) * 64 : WAVE_LDS_DWORDS;
  __shared__ __attribute__((aligned(16))) int wave_lds[4 * REGION];
  int* const my_lds = wave_lds + (threadIdx.x >> 6) * REGION;
  int* const my_stack = my_lds + lane;                             // WIDE: word k of this lane's stack at my_stack[k * 64]
  // the lean build's forms of the hit's inputs (device_prims.hpp): u, v carried in WS_TOP / WS_STEPS (the stash layout above), the lazy fetches of shade_prepare
  constexpr bool UV_CARRIED = HIT_UV_CARRIED && WIDE && !COOP && !COUNT, FETCH_LAZY = HIT_FETCH_LAZY && WIDE && !COOP && !COUNT;
  // the six-wave lean build pops its stack on one straight path (device_wide.hpp wide_pop_lean; it hands no words over: sb stays 0); every other build --
  // its per-frame twin of the present pipeline too -- keeps wide_pop
  constexpr bool POP_LEAN = WIDE && !COOP && !COUNT && !PERFRAME && OCC == 6;
  // ... and decides who steps on the scalar unit (step_by_masks below): the same steps in the same order, from wave masks instead of per-lane flags
  constexpr bool STEP_MASKS = POP_LEAN;
  float* const uv_words = reinterpret_cast<float*>(my_stack) + WIDE_STACK * 64;      // this lane's stash, as the leaf step sees it (UV_CARRIED only)
  unsigned long long* const share_key = reinterpret_cast<unsigned long long*>(my_lds + (WIDE ? SHARE_OFF : 0));     // [64], WIDE && COOP only
  unsigned* const share_pend = reinterpret_cast<unsigned*>(my_lds + (WIDE ? SHARE_OFF : 0) + 128);                   // [64]
  if (WIDE) {                      // the phase-only state lives in the stash (the layout above): no pixel yet
    int* const st0 = my_lds + WIDE_STACK * 64 + lane;
    for (int k = WS_W1; k < WS_STEPS; k++) st0[k * 64] = 0;
  }
  int share = SHARE_ALONE;
  WideStack ws; ws.top = 0u; ws.sp = 0; ws.sb = 0;
  const int ntiles = P.ncols * P.gy;
  const int nwork = ntiles * P.batch;          // queue length: every tile of every frame of the batch
  const WalkRsrc walk = WIDE ? wide_rsrc(P) : walk_rsrc(P);
  Ctr c = {0, 0, 0, 0, 0, 0, 0, 0};
  // wave-uniform work cursor
  // The queue hands out positions q = 0, 1, 2, ...; tile_order (when present) maps a position to
  // a tile so that the tiles that were most expensive in the previous frame of this view start
  // first (longest-processing-time-first: the kernel's duration is otherwise set by whichever
  // expensive tile happens to start last).
  // A launch may cover a batch of frames (same view, consecutive seeds): position q is tile
  // order[q / batch], unit q % batch, so the expensive tiles of ALL frames start first and the
  // tail of one frame (its longest paths) overlaps the bulk of the others.  A unit is 64 of the
  // tile's 64 x batch samples: the tile's pixels of frame q % batch, or -- option sample_order = 1 --
  // consecutive frames of one or two of its pixels (launch_plan.hpp tile_sample).
  // The queue is split into P.regions contiguous parts (tiles are numbered column by column, so a part
  // is a band of the image).  With 8 regions every XCD drains "its" band first -- its 4 MiB L2 then holds
  // the part of the scene that band sees instead of competing for all of it -- and helps the next band
  // once its own is empty.  Region r owns positions [region_start[r], region_start[r+1]) of the order.
  int cur_tile = ntiles, cur_frame = 0;        // chunk being handed out: tile (ntiles = none) and unit of the tile (with sample_order 0 the frame)
  unsigned cur_cert = 0u;          // lean build: cur_tile's word of P.cert_level (wave-uniform) -- in the low ENTRY_SHIFT bits its grade in the view's grazing certificate (0: its
                                   // camera rays keep the scene's margin), above them the entry code of its camera rays (0: the root)
  int cur_next = 64;               // next unassigned lane-in-tile of cur_tile (64 = exhausted: fetch first)
  int cur_limit = 64;              // ... and where this wave's share of cur_tile ends (split tiles: a part of the tile)
  bool cur_split = false;
  // tiles at the head of each region's order that are handed out in P.split_parts parts (work-sharing build, order from feedback)
  // (launches of ONE frame: with several frames in the queue the long pixels of one overlap the bulk of the others anyway, and waves that hold cost throughput)
  const bool splitting = WIDE && COOP && region_start && P.split_parts > 1 && P.batch == 1;      // region r's count: region_start[MAX_REGIONS + 1 + r]
  int region = 0, regions_left = P.regions;
  if (P.regions > 1) region = (int)(__builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11)) % (unsigned)P.regions);   // HW_REG_XCC_ID, 4 bits
  (void)nwork;
  // per-lane path slot
  Trav tr; tr.node = LANE_REFILL; tr.best_t = 0; tr.best_slot = -1;
  Path path; path.rayo = mk(0, 0, 0); path.raydir = mk(0, 0, 0); path.atten = mk(0, 0, 0);
  V3 inv = mk(0, 0, 0), color = mk(0, 0, 0);
  WideRay wr = wide_ray_none();    // WIDE: clamped 1/direction and margins of the folded node test, a function of the lane's ray
  SignMask sg = sign_mask(inv);    // ... and the signs of 1/direction as select masks
  Xorwow rng; rng.v0 = rng.v1 = rng.v2 = rng.v3 = rng.v4 = rng.d = 0;
  int px = -1, py = 0, sample = 0, bounce = 0;
  int frame = 0;                   // frame of the batch the pixel in this slot belongs to
  int pcode = 0;                   // tile * 64 + lane-in-tile of the pixel in this slot
  unsigned steps = 0;              // node steps spent on the pixel in this slot (the cost fed back)
  unsigned rstart = 0;             // value of `steps` when the current ray started
  const bool degenerate = P.max_depth <= 0 || !(P.spp_f > 0.0f);

  // diagnostic stamps (counting build only): wave lifetime, cycles inside the shade/refill phase
  unsigned long long t_begin = 0, t_phase = 0, n_iter = 0, n_phase = 0, n_nodestep = 0, n_leafstep = 0, n_shaded = 0;
  float* const ray_log = COUNT ? reinterpret_cast<float*>(P.counters[STAT_LOG_PTR]) : nullptr;      // measurement aid (dr_context_probe_trace)
  const unsigned long long ray_log_room = COUNT ? P.counters[STAT_LOG_ROOM] : 0ull;
  unsigned long long pb_cands = 0, pb_turns = 0, pb_sphere = 0, pb_disk = 0, pb_retired = 0;      // ... the phase's budget (dr_stats_phase_counts)
  unsigned long long r_begin = 0;
  // wave lifetime in shader cycles and in 100 MHz ticks, every build: two clock reads per wave, written to the statistics buffer only
  t_begin = __builtin_readcyclecounter(); r_begin = __builtin_amdgcn_s_memrealtime();
  bool held = false;               // COOP: this wave has pixels of a split tile and fetches no new tiles while they live
  // wave log (option wave_log): when this wave first found the queue empty, loop iterations since.  Only in the build that short launches
  // use (their timeline is what the log is for): the two scalar instructions per iteration cost the long launches 0.5 %
  constexpr bool WAVE_LOG = WIDE && COOP;
  unsigned long long r_empty = 0, n_after = 0;
  ParkedLeaf pk; pk.v0x = 0; pk.C = pk.D = u32x4{0, 0, 0, 0}; pk.info = 0; pk.parked = false;   // PARK_MIN > 0 only
  for (;;) {
    DR_MARK("loop_top");
    const unsigned long long walking = __ballot(tr.node >= 0 || (PARK_MIN > 0 && pk.parked));
    if (COUNT) n_iter++;
    if (WAVE_LOG && r_empty != 0ull) n_after++;
    // (a wave that only drains -- queue empty, nobody waiting to be shaded or refilled -- skips the phase: its stash/restore would be
    // paid on every iteration of the launch's tail)
    if (WIDE && COOP) {
      // a helper whose subtree is done reports (its best is in the key already) and is idle again; an owner whose own part is
      // done takes the shared result once its last helper has reported
      // (the pending word: helpers still out in the low 8 bits; above them the node steps the helpers have spent on this pixel's rays,
      // which the owner adds to its own when it takes the result -- the cost fed back for a pixel is all the work it caused)
      if (tr.node == LANE_DONE && share >= 0 && share < SHARE_OWNER) {
        atomicMin(&share_key[share], hit_key(tr.best_t, tr.best_slot));
        atomicAdd(&share_pend[share], (((steps - rstart - (unsigned)P.coop_steps) & 0xffffu) << 8) - 1u);
        tr.node = LANE_RETIRED; share = SHARE_ALONE;
      }
      if (tr.node == LANE_DONE && share == SHARE_OWNER) {
        atomicMin(&share_key[lane], hit_key(tr.best_t, tr.best_slot));      // its own last improvement may be newer than the key
        if ((share_pend[lane] & 0xffu) == 0u) {
          steps += share_pend[lane] >> 8;
          const unsigned long long k = share_key[lane];
          tr.best_t = __uint_as_float((unsigned)(k >> 32)); tr.best_slot = (int)(unsigned)k;
          share = SHARE_ALONE;
        }
      }
    }
    const bool waits_for_helpers = WIDE && COOP && share == SHARE_OWNER;      // (only ever true with tr.node == LANE_DONE here or while still walking)
    // (a holding wave -- long pixels, helpers walking for them -- shades as soon as a ray is finished: its pixels' latency is the point)
    // (STEP_MASKS: the count as a scalar int, device_prims.hpp wave_count)
    if (((STEP_MASKS ? wave_count(walking) < TRAV_MIN : __popcll(walking) < TRAV_MIN) || (WIDE && COOP && held)) && (walking == 0ull || __ballot((tr.node == LANE_DONE && !waits_for_helpers) || tr.node == LANE_REFILL) != 0ull)) {
      unsigned long long t0 = 0;
      DR_MARK("phase_begin");
      if (COUNT) { t0 = __builtin_readcyclecounter(); n_phase++; }
      const bool shade_me = tr.node == LANE_DONE && !(PARK_MIN > 0 && pk.parked) && !waits_for_helpers;
      if (COUNT) n_shaded += __popcll(__ballot(shade_me));
      bool fresh_ray = false;                  // this lane starts a new ray in this phase: 1/direction is recomputed after the phase
      constexpr bool BOUNCE_HOME = WIDE && !COOP;      // lean build: the bounce count lives in the stash, WS_BOUNCE (one register more for the walk)
      float* const st = reinterpret_cast<float*>(my_lds) + (WIDE ? WIDE_STACK * 64 : 0) + lane;      // slot k of this lane: st[k * 64]
      // lean build, HIT_UV_CARRIED: the barycentrics of the lane's best hit, left by the leaf step in the two words that the walk's state goes into next
      // (read by the lanes that shade a triangle hit only: a new ray clears nothing)
      const float hit_u = UV_CARRIED ? st[WS_TOP * 64] : 0.0f, hit_v = UV_CARRIED ? st[WS_STEPS * 64] : 0.0f;
      if (WIDE) {
        // what goes in now is the walk's state: stack top, stack pointer, step counts (the stash layout above; the phase-only words are there already)
        st[WS_TOP * 64] = __uint_as_float(ws.top);
        reinterpret_cast<unsigned char*>(st + WS_W1 * 64)[WS_W1_SP_BYTE] = (unsigned char)ws.sp;
        st[WS_STEPS * 64] = __uint_as_float(steps);
        if (COOP) st[WS_RSTART * 64] = __uint_as_float(rstart);      // (lean build: the word is WS_BOUNCE)
        asm volatile("" ::: "memory");
      } else {
        st[TS_V0X * 64] = pk.v0x;
        st[(TS_C + 0) * 64] = __uint_as_float(pk.C.x); st[(TS_C + 1) * 64] = __uint_as_float(pk.C.y); st[(TS_C + 2) * 64] = __uint_as_float(pk.C.z); st[(TS_C + 3) * 64] = __uint_as_float(pk.C.w);
        st[(TS_D + 0) * 64] = __uint_as_float(pk.D.x); st[(TS_D + 1) * 64] = __uint_as_float(pk.D.y); st[(TS_D + 2) * 64] = __uint_as_float(pk.D.z); st[(TS_D + 3) * 64] = __uint_as_float(pk.D.w);
        st[TS_INFO * 64] = __int_as_float(pk.info); st[TS_PARKED * 64] = pk.parked ? 1.0f : 0.0f;
        st[TS_INV_X * 64] = inv.x; st[TS_INV_Y * 64] = inv.y; st[TS_INV_Z * 64] = inv.z;
        // pixel bookkeeping: not needed while the hit is shaded, back right after
        st[TS_COLOR_X * 64] = color.x; st[TS_COLOR_Y * 64] = color.y; st[TS_COLOR_Z * 64] = color.z;
        st[TS_PX * 64] = __int_as_float(px); st[TS_PY * 64] = __int_as_float(py); st[TS_PCODE * 64] = __int_as_float(pcode);
        st[TS_FRAME * 64] = __int_as_float(frame); st[TS_SAMPLE * 64] = __int_as_float(sample);
        st[TS_STEPS * 64] = __uint_as_float(steps); st[TS_RSTART * 64] = __uint_as_float(rstart);
        asm volatile("" ::: "memory");           // the values must really travel through LDS (no forwarding in registers)
      }
      // ---- shade the lanes whose walk has finished
      DR_MARK("phase_shade");
      bool ended = false;
      V3 radiance = mk(0, 0, 0);
      // (the hit is shaded in two parts around the phase's ONE rejection loop, which serves the lanes that scatter -- a point in the unit
      // sphere -- and, further down, the lanes that start a path -- a point in the unit disk: device_rng.hpp rand_points_merged.  A path that ends
      // here, at an emissive surface or at the depth limit, draws nothing more: its generator is re-seeded with its next pixel.)
      ShadeCtx sc; sc.hitpoint = sc.N = sc.ocolor = mk(0, 0, 0); sc.add_x = sc.rough = sc.ir = sc.r5 = 0.0f; sc.mat = -1; sc.front = false;
      bool scatter_me = false;
      if (shade_me) {
        if (tr.best_slot >= 0 && tr.best_t > 0.0f) {
          if (UV_CARRIED || FETCH_LAZY ? !shade_prepare_hit<UV_CARRIED, FETCH_LAZY>(P, path, tr.best_t, tr.best_slot, hit_u, hit_v, rng, c, sc, radiance)
                                       : !shade_prepare<COUNT>(P, path, tr.best_t, tr.best_slot, rng, c, sc, radiance)) ended = true;
          else {
            if (BOUNCE_HOME) bounce = __float_as_int(st[WS_BOUNCE * 64]);
            bounce++;
            if (bounce >= P.max_depth) ended = true;        // depth exhausted: black (K:981)
            else scatter_me = true;
            if (BOUNCE_HOME) st[WS_BOUNCE * 64] = __int_as_float(bounce);
          }
        } else {
          radiance = shade_miss<COUNT>(P, path, c);
          ended = true;
        }
      }
      DR_MARK("phase_unstash");
      if (WIDE) {
        asm volatile("" ::: "memory");
        color = mk(st[WS_COLOR_X * 64], st[WS_COLOR_Y * 64], st[WS_COLOR_Z * 64]);
        { const int xy = __float_as_int(st[WS_XY * 64]); px = (int)((unsigned)xy >> 16) - 1; py = xy & 0xffff; }
        pcode = __float_as_int(st[WS_PCODE * 64]);
        frame = (int)((unsigned)__float_as_int(st[WS_W1 * 64]) >> (16 * WS_W1_FRAME_HALF)); sample = __float_as_int(st[WS_SAMPLE * 64]);
        steps = __float_as_uint(st[WS_STEPS * 64]);
        // (a lane that is still walking keeps its best hit's u, v through the phase: v goes back now that its word is read; u waits in the colour's first word,
        // which is a register from here to the restore, and goes back there -- neither is a register through the rest of the phase)
        if (UV_CARRIED) { st[WS_STEPS * 64] = hit_v; st[WS_COLOR_X * 64] = hit_u; }
        if (COOP) rstart = __float_as_uint(st[WS_RSTART * 64]);
      } else {
        asm volatile("" ::: "memory");
        color = mk(st[TS_COLOR_X * 64], st[TS_COLOR_Y * 64], st[TS_COLOR_Z * 64]);
        px = __float_as_int(st[TS_PX * 64]); py = __float_as_int(st[TS_PY * 64]); pcode = __float_as_int(st[TS_PCODE * 64]);
        frame = __float_as_int(st[TS_FRAME * 64]); sample = __float_as_int(st[TS_SAMPLE * 64]);
        steps = __float_as_uint(st[TS_STEPS * 64]); rstart = __float_as_uint(st[TS_RSTART * 64]);
      }
      if (shade_me) {
        if (ended) {
          color = color + radiance;
          sample++;
          tr.node = LANE_REFILL;
        } else {
          trav_begin(tr);
          rstart = steps;
          fresh_ray = true;
          if (COUNT) c.rays++;
        }
      }
      // ---- lanes between paths: next sample of the same pixel, or store and take a new pixel
      bool want_pixel = false;
      // (a launch that adds a frame-minor batch atomically: the lanes that end the same pixel in this phase add one sum -- device_shade.hpp; wave-uniform)
      // (the five stash words from WS_COLOR_Y on are registers between the unstash and the restore, in every lane: the merge's slots)
      static_assert(WS_SAMPLE - WS_COLOR_Y == 4, "five consecutive stash words");
      const bool merged = STORES_MERGED != 0 && WIDE && !PERFRAME && P.sample_magic != 0u && P.accumulate == 2;
      if (merged) {
        const bool store_me = tr.node == LANE_REFILL && px >= 0 && !((float)sample < P.spp_f && !degenerate);
        if (STORES_MERGED == 2) store_pixels_merged_lds(P, reinterpret_cast<int*>(st) + WS_COLOR_Y * 64, lane, store_me, pcode, px, py, color);
        else store_pixels_merged(P, store_me, pcode, px, py, color);
      }
      if (tr.node == LANE_REFILL) {
        if (px >= 0 && (float)sample < P.spp_f && !degenerate) {
          // same pixel, next sample (K:1059)
        } else {
          if (px >= 0) {
            if (!merged) store_pixel(P, px, py, color, PERFRAME ? (size_t)frame * (size_t)P.out_frame_stride : (size_t)0);
            if (pixel_cost) pixel_cost[pcode & PCODE_MASK] = steps;
          }
          px = -1;
          want_pixel = true;
        }
      }
      if (WIDE && COOP && splitting) {
        // A wave that took a part of a split tile holds -- fetches no further tile -- while one of those pixels lives: its lanes, as
        // their own pixels end, are helpers that take over subtrees of the long pixels' rays (the work-sharing block below); once
        // the pixels are done the lanes go back to fetching.
        held = __ballot(px >= 0 && pcode < 0) != 0ull;
        if (!held && tr.node == LANE_RETIRED && share < 0 && !(cur_tile >= ntiles && regions_left == 0)) { tr.node = LANE_REFILL; want_pixel = true; }
      }
      unsigned long long need = __ballot(want_pixel);
      unsigned cam_cert = 0u;                      // lean build: the word (entry code, grade) of the tile this lane's pixel came from in this phase
      while (need != 0ull) {
        // (the fetch below stays written out in the refill loop: moved into an always-inline lambda, the same statements compile to a different kernel --
        // most of the file's assembly changes; like the wide steps further down, not to be restructured without a GPU to measure on)
        if (cur_next >= cur_limit) {               // wave-uniform: fetch the next chunk (tile, frame)
          if (WIDE && COOP && held) {              // holding: no new tile, the lanes asking become helpers
            if (want_pixel) { tr.node = LANE_RETIRED; want_pixel = false; }
            break;
          }
          cur_tile = ntiles;
          cur_next = 0; cur_limit = 64; cur_split = false;
          while (regions_left > 0) {
            const int r0 = region_start ? region_start[region] : P.region_start[region];
            const int r1 = region_start ? region_start[region + 1] : P.region_start[region + 1];
            unsigned t = 0;
            if (lane == 0) t = atomicAdd(tile_counter + region * cursor_stride, 1u);      // (a line per cursor: launch_plan.hpp cursor_take)
            const int q = (int)__builtin_amdgcn_readfirstlane(t);
            const int nsplit = splitting ? region_start[MAX_REGIONS + 1 + region] : 0;
            if (q < (r1 - r0 + nsplit * (P.split_parts - 1)) * P.batch) {
              int tt = q / P.batch;
              cur_frame = q - tt * P.batch;
              if (WIDE && COOP && tt < nsplit * P.split_parts) {
                // one of the tiles whose pixels were the longest of the last frame (the head of the order): this wave takes
                // 64 / split_parts of its pixels and holds (no further tile) until they are done -- its other lanes help with
                // their rays from the start
                const int part = tt % P.split_parts, width = 64 / P.split_parts;
                tt /= P.split_parts;
                cur_next = part * width; cur_limit = cur_next + width; cur_split = true; held = true;
              } else {
                tt -= nsplit * (P.split_parts - 1);
              }
              cur_tile = tile_order ? tile_order[r0 + tt] : r0 + tt;
              if (BOUNCE_HOME) cur_cert = P.cert_level != nullptr ? P.cert_level[cur_tile] : 0u;
              break;
            }
            region = region + 1 == P.regions ? 0 : region + 1;   // this band is done: help with the next one
            regions_left--;
          }
        }
        if (cur_tile >= ntiles) {                  // frame exhausted: retire the lanes still asking
          if (want_pixel) { tr.node = LANE_RETIRED; want_pixel = false; }
          if (WAVE_LOG && r_empty == 0ull) r_empty = __builtin_amdgcn_s_memrealtime();
          break;
        }
        const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(need >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)need, 0u));
        const int avail = cur_limit - cur_next;
        if (want_pixel && rank < avail) {
          // slot l of unit cur_frame is sample 64 cur_frame + l of the tile: which pixel of the tile and which frame that is, is option sample_order's
          // (launch_plan.hpp tile_sample; a split tile's parts exist in launches of one frame only, where it is the identity)
          const TileSample ts = tile_sample(P.sample_magic, P.batch, cur_frame * 64 + cur_next + rank);
          const int col = cur_tile / P.gy, by = cur_tile - col * P.gy;
          px = (P.stripe_rem + col * P.stripe_mod) * 8 + (ts.p >> 3);
          py = by * 8 + (ts.p & 7);
          pcode = (cur_tile * 64 + ts.p) | (cur_split ? PCODE_SPLIT : 0);
          frame = ts.f;
          steps = 0;
          sample = 0;
          color = mk(0, 0, 0);
          want_pixel = false;
          cam_cert = cur_cert;
        }
        const int n = __popcll(need);
        cur_next += n < avail ? n : avail;
        need = __ballot(want_pixel);
      }
      // ---- start the next path of every lane that has a pixel and no path
      DR_MARK("phase_camera");
      bool new_path = false;
      float cam_nu = 0.0f, cam_nv = 0.0f;
      if (tr.node == LANE_REFILL && px >= 0) {
        if (degenerate) {
          sample = 0x7fffffff;                     // nothing to trace: the pixel is stored as 0 next round
          if (COUNT) c.samples++;
        } else {
          rng.init(sample_seed(P, px, py, sample, frame));
          if (COUNT) { c.samples++; c.rays++; }
          camera_prepare(P, px, py, rng, cam_nu, cam_nv);
          new_path = true;
        }
      }
      {
        // ---- the phase's rejection loop, once for the wave: sphere points for the lanes that scatter, disk points for the lanes that start a path
        unsigned my_turns = 0;
        const int draw_kind = scatter_me && shade_needs_sphere(sc) ? 3 : (new_path ? 2 : 0);
        const V3 pt = rand_points_merged<COUNT>(rng, draw_kind, &my_turns);
        if (COUNT) {
          // the phase's budget (dr_stats_phase_counts): how many turns the wave's rejection loop ran (= its unluckiest lane's), how many lane-turns were useful
          unsigned wave_turns = my_turns;
          for (int off = 32; off > 0; off >>= 1) { const unsigned o = (unsigned)__shfl_xor((int)wave_turns, off, 64); wave_turns = o > wave_turns ? o : wave_turns; }
          unsigned long long lane_turns = my_turns;
          for (int off = 32; off > 0; off >>= 1) lane_turns += __shfl_xor(lane_turns, off, 64);
          const unsigned n_sphere = (unsigned)__popcll(__ballot(draw_kind == 3)), n_disk = (unsigned)__popcll(__ballot(draw_kind == 2));
          const unsigned n_retired = (unsigned)__popcll(__ballot(tr.node == LANE_RETIRED));
          if (lane == 0) atomicAdd(&P.counters[STAT_TURN_HIST + (wave_turns < (unsigned)(STAT_TURN_BINS - 1) ? wave_turns : (unsigned)(STAT_TURN_BINS - 1))], 1ull);      // histogram of turns per phase (the sums below leave with the wave)
          pb_cands += lane_turns; pb_turns += wave_turns; pb_sphere += n_sphere; pb_disk += n_disk; pb_retired += n_retired;
        }
        if (scatter_me) shade_scatter(path, sc, pt, rng);
        if (new_path) {
          camera_finish(P, cam_nu, cam_nv, pt, path.rayo, path.raydir);
          path.atten = splat(1.0f);
          bounce = 0;
          if (BOUNCE_HOME) st[WS_BOUNCE * 64] = __int_as_float(0);
          trav_begin(tr);
          // the camera rays of a tile start at the tile's entry record (no word: the root, as trav_begin left it); ENTRY_NONE: nothing of the scene can
          // be seen from the tile -- the walk is over before it began and the next phase shades a miss
          if (BOUNCE_HOME) tr.node = (int)cam_cert >> ENTRY_SHIFT;
          rstart = steps;
          fresh_ray = true;
        }
      }
      // lean build: the certificate's grade of the lane's ray (the stash layout above)
      if (BOUNCE_HOME && fresh_ray) reinterpret_cast<unsigned char*>(st + WS_W1 * 64)[WS_W1_GRADE_BYTE] = (unsigned char)(new_path ? cam_cert & ((1u << ENTRY_SHIFT) - 1u) : 0u);
      if (COUNT && ray_log && fresh_ray && frame == 0) {      // measurement aid (dr_context_probe_trace): the rays the launch's first frame traces, in the
        // order a per-bounce wavefront would hold them: bounce by bounce, pixels in tile order
        atomicAdd(&P.counters[STAT_LOG_RAYS], 1ull);
        const unsigned long long k = (unsigned long long)bounce * (unsigned long long)(ntiles * 64) + (unsigned long long)(pcode & PCODE_MASK);
        if (k < ray_log_room) {
          float* const r = ray_log + k * 8;
          r[0] = path.rayo.x; r[1] = path.rayo.y; r[2] = path.rayo.z; r[3] = 0.0f; r[4] = path.raydir.x; r[5] = path.raydir.y; r[6] = path.raydir.z; r[7] = 0.0f;
        }
      }
      DR_MARK("phase_restore");
      if (WIDE) {
        asm volatile("" ::: "memory");
        const int w1 = __float_as_int(st[WS_W1 * 64]);
        ws.top = __float_as_uint(st[WS_TOP * 64]); ws.sp = (w1 >> (8 * WS_W1_SP_BYTE)) & 0xff;
        if (UV_CARRIED) st[WS_TOP * 64] = st[WS_COLOR_X * 64];
        // the phase-only state goes home (the values in registers are dead from here to the next phase)
        st[WS_COLOR_X * 64] = color.x; st[WS_COLOR_Y * 64] = color.y; st[WS_COLOR_Z * 64] = color.z;
        st[WS_XY * 64] = __int_as_float(((px + 1) << 16) | py); st[WS_PCODE * 64] = __int_as_float(pcode);
        st[WS_SAMPLE * 64] = __int_as_float(sample);
        reinterpret_cast<unsigned short*>(st + WS_W1 * 64)[WS_W1_FRAME_HALF] = (unsigned short)frame;
        asm volatile("" ::: "memory");
        color = mk(0, 0, 0); px = -1; py = 0; pcode = 0; sample = 0; frame = 0;
        if (fresh_ray) { ws.top = 0u; ws.sp = 0; ws.sb = 0; }
        inv = mk(1.0f / path.raydir.x, 1.0f / path.raydir.y, 1.0f / path.raydir.z);      // 1/direction and the folded test's margins are
        // (a camera ray of a tile of grade g in the view's grazing certificate -- the grade byte of WS_W1 -- carries E scaled by 1e-4 / a_star of ladder step g - 1,
        // grade 0 by 1: DESIGN.md 4.10)
        const float cert = BOUNCE_HOME ? P.wide_cert_k[(w1 >> (8 * WS_W1_GRADE_BYTE)) & CERT_MAX_LEVELS] : 1.0f;
        wr = wide_ray(path.rayo, path.raydir, inv, P.wide_pmax, P.wide_mu.e, P.wide_mu.l, P.wide_mu.v, cert);                // recomputed for every lane rather than stashed
        sg = sign_mask(inv);
      } else {
        asm volatile("" ::: "memory");
        pk.v0x = st[TS_V0X * 64];
        pk.C = u32x4{__float_as_uint(st[(TS_C + 0) * 64]), __float_as_uint(st[(TS_C + 1) * 64]), __float_as_uint(st[(TS_C + 2) * 64]), __float_as_uint(st[(TS_C + 3) * 64])};
        pk.D = u32x4{__float_as_uint(st[(TS_D + 0) * 64]), __float_as_uint(st[(TS_D + 1) * 64]), __float_as_uint(st[(TS_D + 2) * 64]), __float_as_uint(st[(TS_D + 3) * 64])};
        pk.info = __float_as_int(st[TS_INFO * 64]); pk.parked = st[TS_PARKED * 64] != 0.0f;
        inv = mk(st[TS_INV_X * 64], st[TS_INV_Y * 64], st[TS_INV_Z * 64]);
        if (fresh_ray) inv = mk(1.0f / path.raydir.x, 1.0f / path.raydir.y, 1.0f / path.raydir.z);
      }
      if (COUNT) t_phase += __builtin_readcyclecounter() - t0;
      DR_MARK("phase_end");
      if (__ballot(tr.node != LANE_RETIRED) == 0ull) break;
    }
    if (WIDE && COOP && !COUNT && P.coop_steps > 0 && (cur_tile >= ntiles || held)) {
      // ---- draining (the queue is empty), or holding (pixels of a split tile, see the refill above): lanes without a pixel take over subtrees of the rays that still walk.  A walking lane
      // hands the OLDEST word of its stack (the children of a node near the root that it entered but has not visited: the
      // largest piece of work it owns) to an idle lane, which walks it with the same ray.  All lanes of one ray keep the best
      // hit in one LDS word (ds_min_u64 on the (t, slot) key: the lexicographic minimum whatever the order) and prune
      // against it; the owner shades when its own part and every helper's is done.  A ray that would cost one lane hundreds
      // of dependent steps is spread over the idle lanes at the cost of one hand-over per piece -- every leaf is still
      // tested by exactly one lane, with the reference's box and arithmetic, against a bound no smaller than the final t.
      for (int round = 0; round < P.coop_rounds; round++) {      // (a lane that has just taken a word over may hand part of it on in the next round)
      const unsigned long long idle = __ballot(tr.node == LANE_RETIRED);
      const bool can_give = tr.node >= 0 && (ws.sp > ws.sb || ws.top != 0u) && (int)(steps - rstart) >= P.coop_steps;
      const unsigned long long givers = __ballot(can_give);
      const int n_idle = (int)__popcll(idle), n_give = (int)__popcll(givers);
      // (the exchange: XCH_MAX hand-overs per round in the stash's step-count words -- the stash layout above)
      const int n_most = n_idle < n_give ? n_idle : n_give;
      const int n = n_most < XCH_MAX ? n_most : XCH_MAX;
      if (n == 0) break;
      {
        int* const xch = my_lds + XCH_OFF;      // field f of hand-over e at xch[f * XCH_MAX + e]
        const int rank_g = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(givers >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)givers, 0u));
        const int rank_i = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(idle >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)idle, 0u));
        if (can_give && rank_g < n) {
          const int root = share >= 0 && share < SHARE_OWNER ? share : lane;               // the lane whose pixel this ray belongs to
          if (share < 0) { share_key[lane] = hit_key(tr.best_t, tr.best_slot); share_pend[lane] = 0u; share = SHARE_OWNER; }
          atomicAdd(&share_pend[root], 1u);
          unsigned word;
          if (ws.sp > ws.sb) { word = (unsigned)my_stack[ws.sb * 64]; ws.sb++; }
          else { word = ws.top; ws.top = 0u; }
          xch[rank_g + XCH_OX * XCH_MAX] = __float_as_int(path.rayo.x); xch[rank_g + XCH_OY * XCH_MAX] = __float_as_int(path.rayo.y); xch[rank_g + XCH_OZ * XCH_MAX] = __float_as_int(path.rayo.z);
          xch[rank_g + XCH_DX * XCH_MAX] = __float_as_int(path.raydir.x); xch[rank_g + XCH_DY * XCH_MAX] = __float_as_int(path.raydir.y); xch[rank_g + XCH_DZ * XCH_MAX] = __float_as_int(path.raydir.z);
          xch[rank_g + XCH_WORD * XCH_MAX] = (int)word; xch[rank_g + XCH_ROOT * XCH_MAX] = root;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (tr.node == LANE_RETIRED && rank_i < n) {
          path.rayo = mk(__int_as_float(xch[rank_i + XCH_OX * XCH_MAX]), __int_as_float(xch[rank_i + XCH_OY * XCH_MAX]), __int_as_float(xch[rank_i + XCH_OZ * XCH_MAX]));
          path.raydir = mk(__int_as_float(xch[rank_i + XCH_DX * XCH_MAX]), __int_as_float(xch[rank_i + XCH_DY * XCH_MAX]), __int_as_float(xch[rank_i + XCH_DZ * XCH_MAX]));
          ws.top = (unsigned)xch[rank_i + XCH_WORD * XCH_MAX]; ws.sp = 0; ws.sb = 0;
          share = xch[rank_i + XCH_ROOT * XCH_MAX];
          inv = mk(1.0f / path.raydir.x, 1.0f / path.raydir.y, 1.0f / path.raydir.z);
          wr = wide_ray(path.rayo, path.raydir, inv, P.wide_pmax, P.wide_mu.e, P.wide_mu.l, P.wide_mu.v);
          sg = sign_mask(inv);
          const unsigned long long k = share_key[share];
          tr.best_t = __uint_as_float((unsigned)(k >> 32)); tr.best_slot = (int)(unsigned)k;
          wide_pop(tr, ws, my_stack);                              // the first pending child of the word
          rstart = steps - (unsigned)P.coop_steps;                 // a helper may hand on at once
        }
        __builtin_amdgcn_wave_barrier();                           // the exchange words are read before a phase (or the next round) may overwrite them
      }
      }
      // lanes of a shared ray: publish an improvement, take over a better bound
      if (tr.node >= 0 && share >= 0) {
        const int root = share < SHARE_OWNER ? share : lane;
        const unsigned long long mine = hit_key(tr.best_t, tr.best_slot), k = share_key[root];
        if (mine < k) atomicMin(&share_key[root], mine);
        else if (k < mine) { tr.best_t = __uint_as_float((unsigned)(k >> 32)); tr.best_slot = (int)(unsigned)k; }
      }
    }
    if (!WIDE && COOP && !COUNT && P.coop_steps > 0 && cur_tile >= ntiles && (int)__popcll(walking) <= P.coop_lanes) {
      // ---- threaded walk, draining: a ray that is already old is finished by the whole wave at once (coop_closest_hit)
      unsigned long long cand = __ballot(tr.node >= 0 && !(PARK_MIN > 0 && pk.parked) && (int)(steps - rstart) >= P.coop_steps);
      while (cand != 0ull) {
        const int L = __ffsll((long long)cand) - 1;
        cand &= cand - 1ull;
        auto bcast = [L](float v) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), L)); };
        const V3 uo = mk(bcast(path.rayo.x), bcast(path.rayo.y), bcast(path.rayo.z));
        const V3 ud = mk(bcast(path.raydir.x), bcast(path.raydir.y), bcast(path.raydir.z));
        const V3 ui = mk(bcast(inv.x), bcast(inv.y), bcast(inv.z));
        Hit r;
        const bool done = coop_closest_hit(P.pairs, P.prims, uo, ud, ui, bcast(tr.best_t), __builtin_amdgcn_readlane(tr.best_slot, L), my_lds, r);
        if (lane == L) {
          if (done) { tr.best_t = r.t; tr.best_slot = r.slot; tr.node = LANE_DONE; }
          else rstart = 0x80000000u;              // stack overflow: never ask again for this ray ((int)(steps - rstart) is negative from now on)
        }
      }
    }
    if (WIDE) {
      // ---- one record per walking lane.  Lanes at a leaf (exact box + primitive: the long block) wait until enough of
      // them stand at one, or nobody can take a node step.
      // A leaf step and a node step taken together share their fetch round trip, but each then runs for about half the wave (the two are
      // different code).  The kernel is bound by instruction issue, not by latency (seven waves per SIMD are no faster than six,
      // profiles/r3_h), so outside the drain the node lanes of the lean build sit out a leaf step and the node steps in between run fuller:
      // 0.626 -> 0.598 ms/frame with park_min 20 (profiles/r3_i_exclusive_steps.txt).  The work-sharing build keeps the merged steps (one
      // round trip for both kinds of lanes): what exclusive steps gain in its bulk they lose in its tail, 1.10 against 1.075 ms for a single frame.
      // (Leaf postponing, "leaves as soon as they outnumber the nodes" and other thresholds: measured and dropped, profiles/r3_t_*, r3_p_*.)
      // (the first step is written out and the further ones loop: one loop over all of them compiles to a 3.5 % slower lean kernel -- the same
      // work, another schedule; profiles/r4_a_cleanup_ab.txt)
      if (STEP_MASKS) {
        // STEP_MASKS: one step of the wide walk (the rule and its reasons: at the steps of the loop below, which every other build keeps).  Who steps is the same
        // for the whole wave, so it is decided from the two ballots on the scalar unit (device_walk.hpp step_masks) and reaches the lanes as exec masks
        // (device_prims.hpp lane_bit: the masks are wave-uniform, and this runs at the loop's top level with all 64 lanes active).  Spelled per lane the compiler
        // writes do_leaves and do_nodes into registers, selects, masks and compares again, forms `node & 1` a second time for the fetch and compares cur_tile --
        // wave-uniform, but held in a VGPR -- on the VALU: some ten vector instructions in front of every step (profiles/step_control_ab.txt).
        auto step_by_masks = [&]() {
          const unsigned long long on = __ballot(tr.node >= 0), odd = __ballot(tr.node & 1);
          const StepMasks m = step_masks(on & odd, on & ~odd, wave_uniform(cur_tile) >= ntiles, PARK_MIN > 0 ? PARK_MIN : 1, !COOP);
          const bool at_leaf = lane_bit(m.leaf);
          if (lane_bit(m.step)) {
            const WideRec r = wide_fetch(walk, tr.node, at_leaf);
            if (at_leaf) {
              if (UV_CARRIED) wide_leaf_compute_uv<POP_LEAN>(r, path.rayo, path.raydir, inv, sg, tr, ws, my_stack, uv_words + WS_TOP * 64, uv_words + WS_STEPS * 64);
              else wide_leaf_compute<COUNT>(r, path.rayo, path.raydir, inv, sg, tr, ws, my_stack, c);
            }
            else wide_node_compute<COUNT, POP_LEAN>(r, wr, sg, tr, ws, my_stack, c);
            steps++;
          }
        };
        step_by_masks();
        for (int u = 1; u < P_UNROLL; u++) step_by_masks();      // the further steps of an iteration decide anew
        continue;
      }
      const bool at_leaf = tr.node >= 0 && (tr.node & 1);
      const unsigned long long leaves = __ballot(at_leaf);
      const unsigned long long nodes = __ballot(tr.node >= 0 && !(tr.node & 1));
      constexpr int park_thr = PARK_MIN > 0 ? PARK_MIN : 1;
      const bool draining = cur_tile >= ntiles || held;
      const bool do_leaves = leaves != 0ull && ((int)__popcll(leaves) >= park_thr || nodes == 0ull || draining);
      constexpr bool EXCLUSIVE = !COOP;
      const bool do_nodes = !EXCLUSIVE || !do_leaves || draining;
      if (COUNT) { n_leafstep += do_leaves; n_nodestep += nodes != 0ull && do_nodes; }
      if (tr.node >= 0 && (at_leaf ? do_leaves : do_nodes)) {
        if (COUNT) { if (first_active_lane()) c.trav_slots += 64; }
        const WideRec r = wide_fetch(walk, tr.node);
        if (at_leaf) {
          if (UV_CARRIED) wide_leaf_compute_uv<POP_LEAN>(r, path.rayo, path.raydir, inv, sg, tr, ws, my_stack, uv_words + WS_TOP * 64, uv_words + WS_STEPS * 64);
          else wide_leaf_compute<COUNT>(r, path.rayo, path.raydir, inv, sg, tr, ws, my_stack, c);
        }
        else wide_node_compute<COUNT, POP_LEAN>(r, wr, sg, tr, ws, my_stack, c);
        steps++;
      }
      for (int u = 1; u < P_UNROLL; u++) {         // the further steps of an iteration decide anew
        const bool at_leaf2 = tr.node >= 0 && (tr.node & 1);
        const unsigned long long leaves2 = __ballot(at_leaf2);
        const unsigned long long nodes2 = __ballot(tr.node >= 0 && !(tr.node & 1));
        const bool do_leaves2 = leaves2 != 0ull && ((int)__popcll(leaves2) >= park_thr || nodes2 == 0ull || draining);
        const bool do_nodes2 = !EXCLUSIVE || !do_leaves2 || draining;
        if (COUNT) { n_leafstep += do_leaves2; n_nodestep += nodes2 != 0ull && do_nodes2; }
        if (tr.node >= 0 && (at_leaf2 ? do_leaves2 : do_nodes2)) {
          if (COUNT) { if (first_active_lane()) c.trav_slots += 64; }
          const WideRec r = wide_fetch(walk, tr.node);
          if (at_leaf2) {
            if (UV_CARRIED) wide_leaf_compute_uv<POP_LEAN>(r, path.rayo, path.raydir, inv, sg, tr, ws, my_stack, uv_words + WS_TOP * 64, uv_words + WS_STEPS * 64);
            else wide_leaf_compute<COUNT>(r, path.rayo, path.raydir, inv, sg, tr, ws, my_stack, c);
          }
          else wide_node_compute<COUNT, POP_LEAN>(r, wr, sg, tr, ws, my_stack, c);
          steps++;
        }
      }
    } else if (PARK_MIN > 0) {
      // ---- test the parked leaves once enough lanes hold one (or nobody could step anyway)
      const unsigned long long parked = __ballot(pk.parked);
      const unsigned long long steppers = __ballot(tr.node >= 0 && !pk.parked);
      // (once the queue is empty the wave only drains: waiting for company just lengthens the tail)
      if (parked != 0ull && (__popcll(parked) >= PARK_MIN || steppers == 0ull || cur_tile >= ntiles)) {
        if (pk.parked) parked_test<COUNT>(path.rayo, path.raydir, tr, pk, c);
      }
      // ---- UNROLL node steps for every lane that is walking and not parked (the bookkeeping above
      // is then paid once per UNROLL steps; a lane that parks or finishes sits out the rest)
      for (int u = 0; u < P_UNROLL; u++) {     // P_UNROLL is a template constant: fully unrolled by the optimizer
        if (tr.node >= 0 && !pk.parked) {
          if (COUNT) { if (first_active_lane()) c.trav_slots += 64; }
          trav_step_park<COUNT>(walk, path.rayo, inv, tr, pk, c);
          steps++;
        }
      }
    } else {
      // ---- one node step for every walking lane
      if (tr.node >= 0) {
        if (COUNT) { if (first_active_lane()) c.trav_slots += 64; }
        trav_step<COUNT>(walk, path.rayo, path.raydir, inv, tr, c);
        steps++;
      }
    }
  }
  if (WIDE && !COOP && !COUNT && !PERFRAME) {
    // ---- sky tiles (option sky_tiles = 2): every lane has retired -- the queues are empty and this wave's last pixel is stored --, but the
    // launch lasts until its slowest wave's last pixel.  The wave renders the launch's sky tiles in that time, a unit (launch_plan.hpp sky_unit: a sky tile
    // and a chunk of the batch's frames) at a time from a cursor; no walk, no stash: the body of sky_tiles_kernel on all 64 lanes.
    sky_units_run((ArgBlock)__builtin_amdgcn_kernarg_segment_ptr(), lane, pixel_cost);      // P is the kernel's first argument
  }
  if (lane == 0) {
    const unsigned long long r_end = __builtin_amdgcn_s_memrealtime();
    atomicAdd(&P.counters[STAT_WAVE_CYCLES], __builtin_readcyclecounter() - t_begin);
    atomicAdd(&P.counters[STAT_WAVE_TICKS], r_end - r_begin);      // 100 MHz ticks: wave cycles / this = shader clock / 100 MHz
    if (WAVE_LOG && P.wave_log) {
      unsigned long long* const w = P.wave_log + (size_t)wave_id * 16;
      w[0] = r_begin; w[1] = r_empty; w[2] = r_end; w[3] = n_after;
    }
  }
  if (COUNT && lane == 0) {
    atomicAdd(&P.counters[STAT_PHASE_CYCLES], t_phase);
    atomicAdd(&P.counters[STAT_ITERATIONS], n_iter);
    atomicAdd(&P.counters[STAT_PHASES], n_phase);
    atomicAdd(&P.counters[STAT_NODE_STEPS], n_nodestep);
    atomicAdd(&P.counters[STAT_LEAF_STEPS], n_leafstep);
    atomicAdd(&P.counters[STAT_SHADED], n_shaded);
    atomicAdd(&P.counters[STAT_PB_CANDS], pb_cands);        // candidates drawn by all lanes
    atomicAdd(&P.counters[STAT_PB_TURNS], pb_turns);        // turns the waves ran
    atomicAdd(&P.counters[STAT_PB_SPHERE], pb_sphere);       // lanes that drew a point in the sphere (scatter)
    atomicAdd(&P.counters[STAT_PB_DISK], pb_disk);         // lanes that drew a point in the disk (new path)
    atomicAdd(&P.counters[STAT_PB_RETIRED], pb_retired);      // retired lanes summed over phases
  }
  if (COUNT) {
    unsigned v[8] = {c.rays, c.V, c.L, c.S, c.T, c.samples, c.trav_slots, c.ray_slots};
    for (int k = 0; k < 8; k++) {
      unsigned long long s = v[k];
      for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
      if (lane == 0 && s) atomicAdd(&P.counters[STAT_RAYS + k], s);
    }
  }
}

// ------------------------------------------------------------------ launchers
// launch_plan.hpp decides and lists the instantiations; the tables below are expanded from its lists, and a launch is one lookup
namespace {

struct TileEntry { bool count; int mode, occ; void (*kernel)(RenderParams); };
#define DR_ENTRY(COUNT, MODE, OCC) {COUNT, MODE, OCC, render_kernel<COUNT, MODE, OCC>},
const TileEntry TILE_BUILDS[] = {DR_TILE_BUILDS(DR_ENTRY)};
#undef DR_ENTRY

struct PersistentEntry { PersistentBuild build; void (*kernel)(RenderParams, unsigned*, const int*, const int*, unsigned*, int); };
#define DR_ENTRY(COUNT, OCC, T, P, U, WIDE, COOP, PERFRAME) \
  {{COUNT, OCC, T, P, U, WIDE, COOP, PERFRAME}, render_persistent_kernel<COUNT, OCC, T, P, U, WIDE, COOP, PERFRAME>},
const PersistentEntry PERSISTENT_BUILDS[] = {DR_PERSISTENT_BUILDS(DR_ENTRY)};
#undef DR_ENTRY

}  // namespace

void launch_tile_kernel(hipStream_t stream, const RenderParams& P, int traversal, bool count, int occupancy) {
  const int tiles = P.ncols * P.gy;
  const int mode = traversal == DR_TRAVERSAL_ORDERED || traversal == DR_TRAVERSAL_WIDE ? traversal : DR_TRAVERSAL_THREADED, occ = occupancy >= 6 ? 6 : 4;
  for (const TileEntry& e : TILE_BUILDS)
    if (e.count == count && e.mode == mode && e.occ == occ) {
      hipLaunchKernelGGL(e.kernel, dim3((unsigned)((tiles + 3) / 4)), dim3(256), 0, stream, P);
      return;
    }
}

int launch_persistent_kernel(hipStream_t stream, const RenderParams& P_in, const PersistentCfg& cfg, unsigned* tile_counter, int cursor_stride, const int* order,
                             const int* region_start, unsigned* pixel_cost) {
  RenderParams P = P_in;
  const PersistentPlan plan = plan_persistent(cfg, (long long)P.ncols * P.gy * P.batch, P.coop_steps, P.out_frame_stride != 0, P.wave_log != nullptr);
  if (plan.clear_wave_log) P.wave_log = nullptr;
  const int* rstart = order ? region_start : nullptr;        // identity order: the split travels in P.region_start
  for (const PersistentEntry& e : PERSISTENT_BUILDS)
    if (e.build == plan.build) {
      hipLaunchKernelGGL(e.kernel, dim3((unsigned)plan.blocks), dim3(256), 0, stream, P, tile_counter, order, rstart, pixel_cost, cursor_stride);
      return plan.log_waves;
    }
  return -1;      // no such build: nothing is launched in its place
}

}  // namespace dr
