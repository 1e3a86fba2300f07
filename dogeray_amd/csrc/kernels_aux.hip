// Everything on the device that is not a render kernel: tile-order feedback of the persistent kernels, the split of a launch's order, the display divide,
// the stripe copies of the multi-GPU gather, the gather-ceiling probe and the trace-only probe.
#include <hip/hip_runtime.h>

#include "device_rng.hpp"
#include "device_wide.hpp"
#include "device_list.hpp"
#include "device_cert.hpp"
#include "device_surface.hpp"
#include "device_sky.hpp"
#include "device_adaptive.hpp"
#include "device_block.hpp"
#include "kernels.hpp"
#include "../../include/dogeray_amd.h"

namespace dr {

// Cost feedback for the persistent kernel: per-tile cost = the most node steps any of its pixels
// took (the critical path of the tile), then tiles sorted by cost, most expensive first.
__global__ __launch_bounds__(256) void tile_cost_kernel(const unsigned* __restrict__ pixel_cost, unsigned* __restrict__ tile_cost, int ntiles) {
  int tile = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tile >= ntiles) return;
  unsigned v = pixel_cost[(size_t)tile * 64 + (threadIdx.x & 63)];
  for (int off = 32; off > 0; off >>= 1) { unsigned o = __shfl_xor(v, off, 64); v = o > v ? o : v; }
  if ((threadIdx.x & 63) == 0) tile_cost[tile] = v;
}
// One workgroup builds the next launch's tile order.  Per region (band of the tile numbering): first the
// EXPENSIVE tiles (cost above `heavy_factor` x the mean), most expensive first -- they set the length of a
// launch, so they start first; then all other tiles in their natural order, so that the waves of an XCD walk
// their band coherently (neighbouring tiles see neighbouring parts of the scene).
constexpr int ORDER_BUCKETS = 256;
// exclusive prefix sum over the threads of a 1 024-thread block (all of them call it); total = the sum over the block
__device__ __forceinline__ unsigned block_exclusive_scan(unsigned v, unsigned& total) {
  __shared__ unsigned wave_sum[16];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  unsigned x = v;
  for (int off = 1; off < 64; off <<= 1) { const unsigned y = __shfl_up(x, off, 64); if (lane >= off) x += y; }
  if (lane == 63) wave_sum[w] = x;
  __syncthreads();
  if (w == 0) {
    unsigned sw = lane < 16 ? wave_sum[lane] : 0u;
    for (int off = 1; off < 16; off <<= 1) { const unsigned y = __shfl_up(sw, off, 64); if (lane >= off) sw += y; }
    if (lane < 16) wave_sum[lane] = sw;                  // inclusive over the waves
  }
  __syncthreads();
  const unsigned before = w > 0 ? wave_sum[w - 1] : 0u;
  total = wave_sum[15];
  __syncthreads();                                       // wave_sum may be reused by the next call
  return before + x - v;
}
__global__ __launch_bounds__(1024) void tile_order_kernel(const unsigned* __restrict__ tile_cost, int* __restrict__ order,
                                                           int* __restrict__ region_start, int ntiles, int regions, int heavy_factor, int split_steps, int split_limit) {
  constexpr int WAVES = 16, GROUPS = 8;                    // 1 024 threads; a wave reads GROUPS x 64 costs per round trip
  __shared__ unsigned hist[MAX_REGIONS * ORDER_BUCKETS];   // expensive tiles per (region, cost class)
  __shared__ unsigned base[MAX_REGIONS * ORDER_BUCKETS];
  __shared__ unsigned light_cnt[WAVES][MAX_REGIONS];       // light tiles of a wave's range per region, then: of the waves before it
  __shared__ unsigned light_in_region[MAX_REGIONS], light_before[MAX_REGIONS], light_start[MAX_REGIONS], split_tiles[MAX_REGIONS];
  __shared__ int rb[MAX_REGIONS + 1];                      // first tile of region r (region_of(t) = t * regions / ntiles)
  __shared__ unsigned long long total_cost;
  const int nb = regions * ORDER_BUCKETS;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  for (int i = tid; i < nb; i += blockDim.x) hist[i] = 0;
  if (tid < WAVES * MAX_REGIONS) (&light_cnt[0][0])[tid] = 0;
  if (tid < MAX_REGIONS) split_tiles[tid] = 0;
  if (tid <= regions) rb[tid] = (int)(((long long)tid * ntiles + regions - 1) / regions);
  if (tid == 0) total_cost = 0;
  __syncthreads();
  // Wave w owns the contiguous range [w0, w1) of the tile numbering and walks it 64 tiles at a time, lane l on tile g + l: the light
  // tiles keep their natural order through ballots and prefix counts (a range at a time, a region at a time), the expensive ones are
  // binned by cost class.  (One thread per 32-tile chunk with everything per tile took 70-100 us on the one CU this block has.)
  const int w0 = wave_range(ntiles, WAVES, w).w0, w1 = wave_range(ntiles, WAVES, w).w1;
  // body(t, cost, valid, rcur): rcur = region of the 64-tile group's first tile (wave-uniform); a lane's own region is rcur or rcur + 1
  auto for_range = [&](auto&& body) {
    int rcur = 0;
    while (rcur + 1 < regions && w0 >= rb[rcur + 1]) rcur++;
    for (int g0 = w0; g0 < w1; g0 += 64 * GROUPS) {
      unsigned v[GROUPS];
#pragma unroll
      for (int k = 0; k < GROUPS; k++) { const int t = g0 + 64 * k + lane; v[k] = t < w1 ? tile_cost[t] : 0u; }
#pragma unroll
      for (int k = 0; k < GROUPS; k++) {
        const int g = g0 + 64 * k;
        if (g < w1) {
          while (rcur + 1 < regions && g >= rb[rcur + 1]) rcur++;
          body(g + lane, v[k], g + lane < w1, rcur);
        }
      }
    }
  };
  {
    unsigned long long sum = 0;
    for_range([&](int, unsigned cost, bool, int) { sum += cost; });
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
    if (lane == 0) atomicAdd(&total_cost, sum);
  }
  __syncthreads();
  const unsigned long long threshold = heavy_factor > 0 ? (total_cost * (unsigned long long)heavy_factor) / (unsigned long long)(ntiles > 0 ? ntiles : 1)
                                                       : (heavy_factor < 0 ? 0ull : ~0ull);       // -1: every tile by cost, 0: all natural
  auto key_of = [&](unsigned cost, int r) {
    unsigned b = cost >> 4; if (b > ORDER_BUCKETS - 1) b = ORDER_BUCKETS - 1;
    return r * ORDER_BUCKETS + (ORDER_BUCKETS - 1 - (int)b);      // ascending key = region, then most expensive first
  };
  // count: expensive tiles per class; tiles whose longest pixel took at least split_steps node steps (a whole cost class: they are a
  // prefix of their region's order; launches of one frame hand them out in parts, render_persistent_kernel nsplit); light tiles per
  // (wave, region)
  for_range([&](int t, unsigned cost, bool valid, int rcur) {
    const int r = rcur + ((rcur + 1 < regions && t >= rb[rcur + 1]) ? 1 : 0);
    const bool heavy = valid && (unsigned long long)cost > threshold;
    if (heavy) {
      atomicAdd(&hist[key_of(cost, r)], 1u);
      if (split_steps > 0 && (cost >> 4) >= (unsigned)(split_steps >> 4)) atomicAdd(&split_tiles[r], 1u);
    }
    const bool light = valid && !heavy;
    const unsigned long long b0 = __ballot(light && r == rcur), b1 = __ballot(light && r != rcur);
    if (lane == 0) { light_cnt[w][rcur] += (unsigned)__popcll(b0); if (b1) light_cnt[w][rcur + 1] += (unsigned)__popcll(b1); }
  });
  __syncthreads();
  // positions: region r's expensive tiles by class, then its light tiles
  if (tid < regions) {
    unsigned run = 0;
    for (int k = 0; k < WAVES; k++) { const unsigned n = light_cnt[k][tid]; light_cnt[k][tid] = run; run += n; }      // now: light tiles of region tid in the waves before k
    light_in_region[tid] = run;
  }
  unsigned total_heavy;
  const int i0 = tid * 2;                                                            // nb <= 2 * blockDim.x
  const unsigned h0 = i0 < nb ? hist[i0] : 0u, h1 = i0 + 1 < nb ? hist[i0 + 1] : 0u;
  const unsigned heavy_before = block_exclusive_scan(h0 + h1, total_heavy);         // expensive tiles in the classes before i0 (syncs the block)
  if (tid == 0) {
    unsigned lights = 0;
    for (int r = 0; r < regions; r++) { light_before[r] = lights; lights += light_in_region[r]; }      // light tiles in the regions before r
  }
  __syncthreads();
  if (i0 < nb) base[i0] = heavy_before + light_before[i0 / ORDER_BUCKETS];
  if (i0 + 1 < nb) base[i0 + 1] = heavy_before + h0 + light_before[(i0 + 1) / ORDER_BUCKETS];
  __syncthreads();
  if (tid < regions) {
    region_start[tid] = (int)base[tid * ORDER_BUCKETS];
    const unsigned heavy_through = tid + 1 < regions ? base[(tid + 1) * ORDER_BUCKETS] - light_before[tid + 1] : total_heavy;
    light_start[tid] = heavy_through + light_before[tid];                            // where region r's light tiles begin
    const int limit = split_limit / regions;                                         // (any prefix of a region's order will do)
    region_start[MAX_REGIONS + 1 + tid] = (int)split_tiles[tid] < limit ? (int)split_tiles[tid] : limit;
  }
  if (tid == 0) region_start[regions] = ntiles;
  __syncthreads();
  // place
  int placed_r = -1; unsigned placed0 = 0, placed1 = 0;      // light tiles of this wave already placed in regions placed_r and placed_r + 1
  for_range([&](int t, unsigned cost, bool valid, int rcur) {
    if (rcur != placed_r) { placed0 = rcur == placed_r + 1 ? placed1 : 0u; placed1 = 0u; placed_r = rcur; }
    const int r = rcur + ((rcur + 1 < regions && t >= rb[rcur + 1]) ? 1 : 0);
    const bool heavy = valid && (unsigned long long)cost > threshold;
    if (heavy) order[atomicAdd(&base[key_of(cost, r)], 1u)] = t;
    const bool light = valid && !heavy;
    const unsigned long long b0 = __ballot(light && r == rcur), b1 = __ballot(light && r != rcur);
    if (light) {
      if (r == rcur) order[light_start[r] + light_cnt[w][r] + placed0 + lanes_before(b0)] = t;
      else order[light_start[r] + light_cnt[w][r] + placed1 + lanes_before(b1)] = t;
    }
    placed0 += (unsigned)__popcll(b0); placed1 += (unsigned)__popcll(b1);
  });
}

// ---- the split of a launch's order (device_split.hpp order_split_plain says what comes out): the tiles a predicate keeps stay in the
// persistent kernel's queues.  One workgroup: wave w owns a contiguous range of the order's positions -- and, for the list of the dropped tiles, of the tile
// numbering -- and walks it GROUPS x 64 at a time, twice: counting, then placing through ballots and prefix counts, as tile_order_kernel places its light
// tiles; a round trip's loads are all issued before any is used.  Two instances: SkyKeep over the tiles' words (option sky_tiles: with the list, counts [0]
// dropped = sky tiles, [1] kept = geometry tiles) and FlagKeep over an adaptive pass's flags (no list, no counts).  own: the identity order's region starts.
struct OrderRegions { int start[MAX_REGIONS + 1]; };
template <class Keep, bool LIST, int GROUPS>
__global__ __launch_bounds__(1024) void order_split_kernel(const int* __restrict__ order, const int* __restrict__ region_start, OrderRegions own, Keep keep,
                                                            int ntiles, int regions, int* __restrict__ launch_order, int* __restrict__ launch_region_start,
                                                            int* __restrict__ dropped_list, unsigned* __restrict__ counts) {
  constexpr int WAVES = 16; typedef typename Keep::Value Value;
  __shared__ int rs[MAX_REGIONS + 1];
  __shared__ unsigned cnt[LIST ? 2 : 1][WAVES];            // per wave: [0] kept tiles of its positions, [1] dropped tiles of its tile numbers
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (tid <= MAX_REGIONS) {
    int v = ntiles;
    if (tid <= regions) {
      if (order) v = region_start[tid];
      else {
#pragma unroll
        for (int k = 0; k <= MAX_REGIONS; k++) if (tid == k) v = own.start[k];
      }
    }
    rs[tid] = v;
  }
  if (tid > regions && tid < 2 * MAX_REGIONS + 1) launch_region_start[tid] = 0;      // (the split counts among them: such a launch hands out no tile in parts)
  __syncthreads();
  const int w0 = wave_range(ntiles, WAVES, w).w0, w1 = wave_range(ntiles, WAVES, w).w1;
  // body(i, t, kept, dropped): position i of the order holds tile t, which is (not) kept; tile i is dropped (never, without a list).  Whole waves come
  // here, i >= w1 in the lanes past the range
  auto for_range = [&](auto&& body) {
    for (int g0 = w0; g0 < w1; g0 += 64 * GROUPS) {
      int t[GROUPS]; Value vt[GROUPS], vi[GROUPS] = {};
#pragma unroll
      for (int k = 0; k < GROUPS; k++) { const int i = g0 + 64 * k + lane; t[k] = i < w1 ? (order ? order[i] : i) : -1; }
#pragma unroll
      for (int k = 0; k < GROUPS; k++) {
        const int i = g0 + 64 * k + lane;
        if constexpr (LIST) vi[k] = i < w1 ? keep.load(i) : Value(0);
        vt[k] = (unsigned)t[k] < (unsigned)ntiles ? keep.load(t[k]) : Value(0);
      }
#pragma unroll
      for (int k = 0; k < GROUPS; k++) {
        const int i = g0 + 64 * k + lane;
        if (g0 + 64 * k < w1) body(i, t[k], (unsigned)t[k] < (unsigned)ntiles && Keep::keep(vt[k]), LIST && i < w1 && !Keep::keep(vi[k]));
      }
    }
  };
  unsigned nk = 0, nd = 0;
  for_range([&](int, int, bool kept, bool dropped) { nk += (unsigned)__popcll(__ballot(kept)); if constexpr (LIST) nd += (unsigned)__popcll(__ballot(dropped)); });
  if (lane == 0) { cnt[0][w] = nk; if constexpr (LIST) cnt[1][w] = nd; }
  __syncthreads();
  unsigned kbase = 0, dbase = 0, ktotal = 0, dtotal = 0;
  for (int k = 0; k < WAVES; k++) {
    if (k < w) { kbase += cnt[0][k]; if constexpr (LIST) dbase += cnt[1][k]; }
    ktotal += cnt[0][k]; if constexpr (LIST) dtotal += cnt[1][k];
  }
  for_range([&](int i, int t, bool kept, bool dropped) {
    const unsigned long long bk = __ballot(kept);
    const unsigned p = kbase + lanes_before(bk);             // kept tiles in front of position i
    if (i < w1)
      for (int r = 0; r <= regions; r++) if (i == rs[r]) launch_region_start[r] = (int)p;
    if (kept) launch_order[p] = t;
    kbase += (unsigned)__popcll(bk);
    if constexpr (LIST) {
      const unsigned long long bd = __ballot(dropped);
      if (dropped) dropped_list[dbase + lanes_before(bd)] = i;
      dbase += (unsigned)__popcll(bd);
    }
  });
  if (tid <= regions && rs[tid] >= ntiles) launch_region_start[tid] = (int)ktotal;      // (the end, and regions that start there)
  if constexpr (LIST) if (tid == 0) { counts[0] = dtotal; counts[1] = ktotal; }
}
// One wave per sky tile and the launch's whole batch (device_sky.hpp sky_tile_frames: the body it shares with the lean build's retiring waves, option
// sky_tiles = 2).
__global__ __launch_bounds__(256) void sky_tiles_kernel(RenderParams P, const int* __restrict__ sky_list, const unsigned* __restrict__ counts,
                                                         unsigned* __restrict__ pixel_cost) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= (int)counts[0]) return;
  sky_tile_frames(P, sky_list[i], lane, 0, P.batch, pixel_cost);
}

// clamp(acc / divide_by, 0, 255) into row-major RGB8 (draw loop K:2281-2287)
__global__ void present_kernel(const int32_t* acc, const int32_t* hist, uint8_t* rgb, int W, int H, int div) {
  int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= W * H) return;
  int x = idx / H, y = idx - x * H;          // consecutive threads walk a column (coalesced read)
  const int32_t* p = acc + (size_t)idx * 3;
  uint8_t* q = rgb + ((size_t)y * W + x) * 3;
  if (hist) {                                // a history plane (dr_accum_reproject): the pixel's own divisor, 0 giving 0
    div += hist[idx];
    if (div == 0) { q[0] = 0; q[1] = 0; q[2] = 0; return; }
  }
  for (int k = 0; k < 3; k++) {
    int v = p[k] / div;
    v = v < 0 ? 0 : (v > 255 ? 255 : v);
    q[k] = (uint8_t)v;
  }
}

// Multi-GPU gather (K:1006: the framebuffer is column-major, so an 8-pixel block column is ONE contiguous run of
// 8*H*3 int32): copies `ncols` such runs between a strided position in a frame and a packed buffer, 16 bytes per lane.
//   pack    frame column rem + j*mod  ->  packed column j          (dr_accum_pack_stripe)
//   unpack  packed column j of rank r ->  frame column r + j*R     (dr_accum_unpack_stripes, on rank 0)
__global__ __launch_bounds__(256) void stripe_copy_kernel(int4* __restrict__ dst, const int4* __restrict__ src, int ncols, int run4,
                                                          long long dst_first4, long long dst_stride4, long long src_first4, long long src_stride4) {
  const int col = blockIdx.y;
  if (col >= ncols) return;
  int4* d = dst + dst_first4 + (long long)col * dst_stride4;
  const int4* sp = src + src_first4 + (long long)col * src_stride4;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < run4; i += gridDim.x * blockDim.x) d[i] = sp[i];
}

// Ceiling probe for the measurement harness (bench.py `roofline.gather`): every lane fetches 64-byte records of the
// resident wide array at addresses that depend on what it fetched before -- the walk's memory behaviour without its
// arithmetic.  `nrec` restricts the walk to the first records of the array (a set that fits the L2s, or all of it).
__global__ __launch_bounds__(256, 5) void gather_probe_kernel(RenderParams P, unsigned nrec, int iters, unsigned* out) {
  const WalkRsrc r = wide_rsrc(P);
  unsigned x = (blockIdx.x * 256u + threadIdx.x) * 2654435761u + 12345u;
  unsigned acc = 0;
  for (int i = 0; i < iters; i++) {
    const unsigned off = (x % nrec) << 6;
    const u32x4 a = ld_unit_raw(r, off), b = ld_unit_raw(r, off + 16), c = ld_unit_raw(r, off + 32), d = ld_unit_raw(r, off + 48);
    acc += a.x ^ b.y ^ c.z ^ d.w;
    x = x * 1664525u + 1013904223u + (acc & 1u);
  }
  if (acc == 0x12345678u) out[0] = acc;
}

// ---- measurement aid: a TRACE-ONLY kernel over a list of rays (dr_context_probe_trace).  What would the walk cost if it were a kernel of its own -- a wave's
// lanes refilling from a global ray queue in a few instructions, no generator / attenuation / pixel state in its registers, shading done elsewhere?  Same node and
// leaf steps as the render kernel (exclusive steps, leaf steps once PARK lanes stand at a leaf), results {t bits, slot} per ray ({10000, -1}: no hit).
template <int OCC, int REFILL_MIN, int PARK>
__global__ __launch_bounds__(256, OCC) void trace_probe_kernel(RenderParams P, const float4* __restrict__ rays, unsigned n, unsigned* __restrict__ cursor, uint2* __restrict__ out) {
  __shared__ int lds[4 * WIDE_STACK * 64];
  const int lane = threadIdx.x & 63;
  int* const my_stack = lds + (threadIdx.x >> 6) * (WIDE_STACK * 64) + lane;
  const WalkRsrc walk = wide_rsrc(P);
  Trav tr; tr.node = LANE_REFILL; tr.best_t = 0; tr.best_slot = -1;      // LANE_REFILL: wants a ray; LANE_DONE: result not written yet (device_walk.hpp)
  WideStack ws; ws.top = 0u; ws.sp = 0; ws.sb = 0;
  V3 o = mk(0, 0, 0), d = mk(0, 0, 0), inv = mk(0, 0, 0);
  WideRay wr = wide_ray_none();
  SignMask sg = sign_mask(inv);
  Ctr c = {0, 0, 0, 0, 0, 0, 0, 0};
  unsigned idx = 0;
  ListFeed feed;
  for (;;) {
    const unsigned long long want = __ballot(tr.node == LANE_DONE || tr.node == LANE_REFILL);
    const unsigned long long walking = __ballot(tr.node >= 0);
    if (want != 0ull && ((int)__popcll(want) >= REFILL_MIN || walking == 0ull)) {
      if (tr.node == LANE_DONE) out[idx] = make_uint2(__float_as_uint(tr.best_t), (unsigned)tr.best_slot);
      const bool mine = tr.node == LANE_DONE || tr.node == LANE_REFILL;
      const ListItem it = feed.take<128u>(want, cursor, n);
      if (mine) {
        if (it.ok) {
          const float4 a = rays[2 * (size_t)it.index], b = rays[2 * (size_t)it.index + 1];
          idx = it.index; o = mk(a.x, a.y, a.z); d = mk(b.x, b.y, b.z);
          inv = mk(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
          wr = wide_ray(o, d, inv, P.wide_pmax, P.wide_mu.e, P.wide_mu.l, P.wide_mu.v); sg = sign_mask(inv);
          trav_begin(tr); ws.top = 0u; ws.sp = 0; ws.sb = 0;
        } else tr.node = it.state;
      }
      if (__ballot(tr.node != LANE_RETIRED) == 0ull) break;
    }
    list_walk_round<PARK>(walk, wr, sg, feed.exhausted, tr, ws, my_stack, c,
                          [&](const WideRec& r) { wide_leaf_compute<false>(r, o, d, inv, sg, tr, ws, my_stack, c); });
  }
}
// the same rays, one per lane, each wave waiting for its slowest (the reference the probe's results are checked against)
__global__ __launch_bounds__(256) void trace_plain_kernel(RenderParams P, const float4* __restrict__ rays, unsigned n, uint2* __restrict__ out) {
  __shared__ int lds[4 * WIDE_STACK * 64];
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  int* const stack = lds + (threadIdx.x >> 6) * (WIDE_STACK * 64) + (threadIdx.x & 63);
  Ctr c = {0, 0, 0, 0, 0, 0, 0, 0};
  const float4 a = rays[2 * (size_t)i], b = rays[2 * (size_t)i + 1];
  const Hit h = closest_hit_wide<false>(wide_rsrc(P), P.wide_pmax, P.wide_mu.e, P.wide_mu.l, P.wide_mu.v, mk(a.x, a.y, a.z), mk(b.x, b.y, b.z), c, stack);
  out[i] = h.slot < 0 ? make_uint2(__float_as_uint(10000.0f), 0xffffffffu) : make_uint2(__float_as_uint(h.t), (unsigned)h.slot);
}

// acc += frame, 16 bytes per lane (pipelined single frames: every frame renders into a buffer of its own and is folded into
// the accumulator in frame order, K:2213-2218)
__global__ __launch_bounds__(256) void frame_add_kernel(int4* __restrict__ acc, const int4* __restrict__ frame, size_t n4, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    int4 a = acc[i];
    const int4 f = frame[i];
    a.x += f.x; a.y += f.y; a.z += f.z; a.w += f.w;
    acc[i] = a;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3))       // W * H * 3 need not be a multiple of 4
    reinterpret_cast<int*>(acc)[n4 * 4 + threadIdx.x] += reinterpret_cast<const int*>(frame)[n4 * 4 + threadIdx.x];
}

// ------------------------------------------------------------------ launchers
// Per-view grazing certificate of the camera rays (option camera_cert): one thread per primitive (slot order); a small triangle whose
// bound A_T of |d . (e1 x e2)| over the view's camera rays meets only g < n_levels steps of the view's ladder sets, in bit plane g, the bits of the
// launch's tiles that can see its padded box (device_cert.hpp cert_leaf).  mask: words [0, nwords) = one bit per tile (flagged at a_star: a bit in a
// plane g <= cv.base), word nwords = "every tile", word nwords + 1 = flagged tiles, then the n_levels planes of nwords words each; the first
// nwords + 2 words and the level bytes are cert_finish_kernel's.
__global__ __launch_bounds__(256) void cert_mask_kernel(const DevPrim* __restrict__ prims, int n, CertView cv, uint32_t* __restrict__ mask, int nwords) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const DevPrim p = prims[i];
  if (p.type != 2) return;
  const float e1[3] = {p.e1x, p.e1y, p.e1z}, e2[3] = {p.e2x, p.e2y, p.e2z};
  int rect[4] = {0, -1, 0, -1};
  int g = 0;
  const int k = cert_leaf(cv, p.v0, e1, e2, rect, &g);
  if (k == 0) return;
  if (k == 2) { atomicOr(&mask[nwords], 1u); return; }
  uint32_t* const plane = mask + nwords + 2 + (size_t)g * (size_t)nwords;
  for (int col = rect[0]; col <= rect[1]; col++) {
    const int b0 = col * cv.gy + rect[2], b1 = col * cv.gy + rect[3];      // bits [b0, b1]: one run per column
    for (int w = b0 >> 5; w <= (b1 >> 5); w++) {
      const int lo = w * 32 > b0 ? 0 : b0 - w * 32, hi = w * 32 + 31 < b1 ? 31 : b1 - w * 32;
      const uint32_t bits = (hi == 31 ? ~0u : ((1u << (hi + 1)) - 1u)) & ~((1u << lo) - 1u);
      if ((plane[w] & bits) != bits) atomicOr(&plane[w], bits);      // (neighbouring grazing triangles flag the same tiles: most words are set already)
    }
  }
}
// one workgroup: the planes -> the tile bits (planes 0 .. base) and a tile's grade, one byte per tile in `level` (8 words per mask word: the lowest plane
// with its bit, n_levels without one; bytes past the last tile 0); "every tile" -> all bits and grade 0; the number of flagged tiles into word nwords + 1
__global__ __launch_bounds__(1024) void cert_finish_kernel(uint32_t* __restrict__ mask, uint32_t* __restrict__ level, int ntiles, int nwords, int n_levels, int base) {
  __shared__ unsigned part[16];
  const bool all = mask[nwords] != 0u;
  unsigned cnt = 0;
  for (int w = threadIdx.x; w < nwords; w += 1024) {
    const int left = ntiles - w * 32;
    const uint32_t valid = left >= 32 ? ~0u : ((1u << left) - 1u);
    uint32_t pl[CERT_MAX_LEVELS];
    uint32_t v = 0u;
    for (int g = 0; g < CERT_MAX_LEVELS; g++) {
      pl[g] = g < n_levels ? mask[nwords + 2 + (size_t)g * (size_t)nwords + w] : 0u;
      if (g <= base) v |= pl[g];
    }
    v &= valid;
    if (all) v = valid;
    mask[w] = v;
    cnt += (unsigned)__popc(v);
    for (int q = 0; q < 8; q++) {
      uint32_t word = 0u;
      for (int b = 0; b < 4; b++) {
        const int bit = q * 4 + b;
        unsigned grade = (unsigned)n_levels;
        for (int g = CERT_MAX_LEVELS - 1; g >= 0; g--) if ((pl[g] >> bit) & 1u) grade = (unsigned)g;
        if (all || !((valid >> bit) & 1u)) grade = 0u;
        word |= grade << (8 * b);
      }
      level[w * 8 + q] = word;
    }
  }
  for (int off = 32; off > 0; off >>= 1) cnt += (unsigned)__shfl_xor((int)cnt, off, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned t = 0;
    for (int k = 0; k < 16; k++) t += part[k];
    mask[nwords + 1] = t;
  }
}

// The camera rays' entry table of the same view (option camera_entry; the bodies: device_cert.hpp entry_leaf, entry_tile).  One
// thread per leaf of the wide tree, in depth-first order (leaf_rec: rank -> record): its record's box folded into the lowest and the highest rank
// of every tile it can be seen from (mm: 2 ntiles + 1 words, all ones before).
__global__ __launch_bounds__(256) void entry_leaf_kernel(const DevUnit* __restrict__ wide, const uint32_t* __restrict__ leaf_rec, int n, CertView cv,
                                                         uint32_t* __restrict__ mm, int ntiles) {
  const int rank = blockIdx.x * 256 + threadIdx.x;
  if (rank >= n) return;
  const DevUnit* const rec = wide + (size_t)leaf_rec[rank] * WIDE_UNITS;
  const DevUnit A = rec[0], B = rec[1];
  entry_leaf(cv, A.f, B.f, (uint32_t)rank, mm, ntiles);
}
// one thread per tile: its word for the render kernel, entry code << ENTRY_SHIFT | grade (level: cert_finish_kernel's bytes; mm null: every
// tile starts at the root)
__global__ __launch_bounds__(256) void entry_finish_kernel(const DevUnit* __restrict__ wide, const uint32_t* __restrict__ range, const uint32_t* __restrict__ mm,
                                                           const uint32_t* __restrict__ level, uint32_t* __restrict__ word, int ntiles) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= ntiles) return;
  const uint32_t grade = (level[t >> 2] >> ((t & 3) * 8)) & 0xffu;
  const int code = mm ? entry_tile(wide, range, mm[2 * (size_t)t], mm[2 * (size_t)t + 1], mm[2 * (size_t)ntiles] == 0u) : 0;
  word[t] = ((uint32_t)code << ENTRY_SHIFT) | grade;
}

void launch_cert_mask(hipStream_t stream, const DevPrim* prims, int n, const CertView& cv, uint32_t* mask, uint32_t* level, int ntiles) {
  const int nwords = (ntiles + 31) / 32;
  (void)hipMemsetAsync(mask, 0, cert_mask_words(ntiles, cv.n_levels) * sizeof(uint32_t), stream);
  if (n > 0) hipLaunchKernelGGL(cert_mask_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, prims, n, cv, mask, nwords);
  hipLaunchKernelGGL(cert_finish_kernel, dim3(1), dim3(1024), 0, stream, mask, level, ntiles, nwords, cv.n_levels, cv.base);
}
void launch_camera_entry(hipStream_t stream, const DevUnit* wide, const uint32_t* leaf_rec, const uint32_t* range, int n_leaves, const CertView& cv,
                         uint32_t* mm, const uint32_t* level, uint32_t* word, int ntiles) {
  if (mm) {
    (void)hipMemsetAsync(mm, 0xff, entry_mm_words(ntiles) * sizeof(uint32_t), stream);
    if (n_leaves > 0) hipLaunchKernelGGL(entry_leaf_kernel, dim3((unsigned)((n_leaves + 255) / 256)), dim3(256), 0, stream, wide, leaf_rec, n_leaves, cv, mm, ntiles);
  }
  hipLaunchKernelGGL(entry_finish_kernel, dim3((unsigned)((ntiles + 255) / 256)), dim3(256), 0, stream, wide, range, mm, level, word, ntiles);
}
void launch_tile_feedback(hipStream_t stream, const unsigned* pixel_cost, unsigned* tile_cost, int* tile_order, int* region_start, int tiles, int regions,
                          int heavy_factor, int split_steps, int split_limit) {
  hipLaunchKernelGGL(tile_cost_kernel, dim3((unsigned)((tiles + 3) / 4)), dim3(256), 0, stream, pixel_cost, tile_cost, tiles);
  hipLaunchKernelGGL(tile_order_kernel, dim3(1), dim3(1024), 0, stream, tile_cost, tile_order, region_start, tiles, regions, heavy_factor, split_steps, split_limit);
}
void launch_order_split(hipStream_t stream, int kind, const int* order, const int* region_start, const int* own_region_start, const void* key, int tiles,
                        int regions, int* launch_order, int* launch_region_start, int* dropped_list, unsigned* counts) {
  if (tiles <= 0) return;
  OrderRegions own;
  for (int r = 0; r <= MAX_REGIONS; r++) own.start[r] = own_region_start[r];
  if (!order) region_start = nullptr;
  if (kind == SPLIT_BY_WORD)
    hipLaunchKernelGGL((order_split_kernel<SkyKeep, true, 8>), dim3(1), dim3(1024), 0, stream, order, region_start, own, SkyKeep{static_cast<const uint32_t*>(key)},
                       tiles, regions, launch_order, launch_region_start, dropped_list, counts);
  else
    hipLaunchKernelGGL((order_split_kernel<FlagKeep, false, 1>), dim3(1), dim3(1024), 0, stream, order, region_start, own, FlagKeep{static_cast<const uint8_t*>(key)},
                       tiles, regions, launch_order, launch_region_start, nullptr, nullptr);
}
void launch_sky_tiles(hipStream_t stream, const RenderParams& P, const int* sky_list, const unsigned* counts, unsigned* pixel_cost) {
  const int tiles = P.ncols * P.gy;
  hipLaunchKernelGGL(sky_tiles_kernel, dim3((unsigned)((tiles + 3) / 4)), dim3(256), 0, stream, P, sky_list, counts, pixel_cost);
}
void launch_present(hipStream_t stream, const int32_t* acc, const int32_t* hist, uint8_t* rgb, int W, int H, int div) {
  const int n = W * H;
  hipLaunchKernelGGL(present_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, acc, hist, rgb, W, H, div);
}
void launch_frame_add(hipStream_t stream, int32_t* acc, const int32_t* frame, size_t n) {      // n int32
  const size_t n4 = n / 4;
  size_t blocks = (n4 + 255) / 256; if (blocks > 2048) blocks = 2048; if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(frame_add_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, reinterpret_cast<int4*>(acc), reinterpret_cast<const int4*>(frame), n4, n);
}
void launch_stripe_copy(hipStream_t stream, int32_t* dst, const int32_t* src, int ncols, int run4, long long dst_first4, long long dst_stride4,
                        long long src_first4, long long src_stride4) {
  int bx = (run4 + 255) / 256; if (bx > 64) bx = 64;
  hipLaunchKernelGGL(stripe_copy_kernel, dim3((unsigned)bx, (unsigned)ncols), dim3(256), 0, stream, reinterpret_cast<int4*>(dst), reinterpret_cast<const int4*>(src),
                     ncols, run4, dst_first4, dst_stride4, src_first4, src_stride4);
}
void launch_gather_probe(hipStream_t stream, const RenderParams& P, int blocks, unsigned nrec, int iters, unsigned* out) {
  hipLaunchKernelGGL(gather_probe_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, P, nrec, iters, out);
}
void launch_trace_probe(hipStream_t stream, const RenderParams& P, int num_cus, int variant, const float* rays, unsigned n, unsigned* cursor, unsigned* out) {
  const float4* r4 = reinterpret_cast<const float4*>(rays);
  uint2* o2 = reinterpret_cast<uint2*>(out);
  switch (variant) {
    case 0: hipLaunchKernelGGL(trace_plain_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, P, r4, n, o2); break;
    case 1: hipLaunchKernelGGL((trace_probe_kernel<6, 1, 20>), dim3((unsigned)(num_cus * 6)), dim3(256), 0, stream, P, r4, n, cursor, o2); break;
    case 2: hipLaunchKernelGGL((trace_probe_kernel<6, 8, 20>), dim3((unsigned)(num_cus * 6)), dim3(256), 0, stream, P, r4, n, cursor, o2); break;
    case 3: hipLaunchKernelGGL((trace_probe_kernel<6, 16, 20>), dim3((unsigned)(num_cus * 6)), dim3(256), 0, stream, P, r4, n, cursor, o2); break;
    case 4: hipLaunchKernelGGL((trace_probe_kernel<8, 8, 20>), dim3((unsigned)(num_cus * 8)), dim3(256), 0, stream, P, r4, n, cursor, o2); break;
    case 5: hipLaunchKernelGGL((trace_probe_kernel<8, 8, 28>), dim3((unsigned)(num_cus * 8)), dim3(256), 0, stream, P, r4, n, cursor, o2); break;
    case 6: hipLaunchKernelGGL((trace_probe_kernel<6, 8, 28>), dim3((unsigned)(num_cus * 6)), dim3(256), 0, stream, P, r4, n, cursor, o2); break;
    default: hipLaunchKernelGGL((trace_probe_kernel<8, 4, 32>), dim3((unsigned)(num_cus * 8)), dim3(256), 0, stream, P, r4, n, cursor, o2); break;
  }
}

}  // namespace dr
