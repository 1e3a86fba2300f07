// What one launch of an accumulator stage needs: the grids, the parameters and the planes of the denoiser, the upsampler, the temporal
// reprojection and the noise estimate -- and what a launch of dr_trace_radiance or dr_query_nearest needs.  No HIP in here: kernels.hpp hands these structs to the launchers with device pointers in them, and the
// host build (tools/host_kernel.cpp) fills the same structs with host pointers; the per-pixel bodies of device_denoise.hpp, device_upscale.hpp,
// device_reproject.hpp and device_moments.hpp take them and run on either.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "device_layout.h"

namespace dr {

// kernels_denoise.hip: planes of the gw x gh pixel grid, row-major (pixel (x, y) at y * gw + x), as launch_aov writes them
struct DnLaunch {
  int gw, gh;                     // pixel grid
  int W, H;                       // accumulator (column-major, (x * H + y) * 3) and output (row-major W x H x 3)
  int divide_by;
  DnParams D;
  const int32_t* acc;
  const int32_t* hist;            // the accumulator's history plane (pixel (x, y) at x * H + y: its divisor is hist + divide_by), or null
  const float* normal;            // launch_aov's normal (3 per pixel) and depth: read by the guide prepare only
  const float* depth;
  const float* albedo;            // launch_aov's albedo (3 per pixel)
  const int32_t* mat;             // launch_aov's material (-1: miss)
  const unsigned long long* m2;   // the second-moment plane (pixel (x, y) at x * H + y) when stage 1 takes the temporal variance from it (option
                                  // "denoise_variance"), or null: the spatial estimate everywhere
  float* guide;                   // float4 (n.x, n.y, n.z, z)
  float* gz;                      // depth gradient
  const float* src;               // colour planes, float4 per pixel: (e, l) or (e, var)
  float* dst;
  float* out_f32;                 // W x H x 3 (null: not written)
  uint8_t* out_rgb8;
};

// kernels_upscale.hip: the low side is the denoiser's (DnLaunch's grid, guide, albedo, mat and a colour plane), the full side the same planes
// over the full-resolution pixel grid FW x FH = (W / 8) * 8 x (H / 8) * 8 (pixel (X, Y) at Y * FW + X); block mode reads neither
struct UpLaunch {
  int gw, gh;                     // low pixel grid; the output grid is gw * div x gh * div
  int FW, FH;                     // full-resolution pixel grid
  int W, H;                       // accumulator (column-major) and output (row-major W x H x 3)
  int div;                        // (int)settings13[11]
  int divide_by;
  UpParams U;
  const int32_t* acc;
  const int32_t* hist;            // the accumulator's history plane, or null
  const float* e;                 // low colour plane, float4 per pixel: (e.r, e.g, e.b, *)
  const float* guide;             // low guides: float4 (n, z), material
  const int32_t* mat;
  const float* Fguide;            // full guides: float4 (N, Z), albedo (3 per pixel), material, depth gradient
  const float* Falbedo;
  const int32_t* Fmat;
  const float* Fgz;
  float* out_f32;                 // W x H x 3 (null: not written)
  uint8_t* out_rgb8;
};

// kernels_reproject.hip: the guides of both views are row-major gw x gh planes as launch_aov writes them; the accumulators are column-major W x H x 3
// ((x * H + y) * 3) and the history planes W x H (x * H + y).  Pixels outside the grid are not written (the caller clears the `to` pair).
struct RpLaunch {
  int gw, gh;                     // pixel grid of both views
  int W, H;
  int frames;                     // frames the `from` accumulator holds beyond its history plane
  RpParams R;
  RpCamera to, from;
  RpProj J;                       // projection into the `from` camera
  const float* t_to; const float* normal_to; const int32_t* mat_to;
  const float* t_from; const float* normal_from; const int32_t* mat_from;
  const int32_t* acc_from;
  const int32_t* hist_from;       // null: no history yet (0 everywhere)
  int32_t* acc_to;
  int32_t* hist_to;
  const unsigned long long* m2_from;   // the second-moment planes (W x H at x * H + y), or both null: no plane is carried
  unsigned long long* m2_to;
  unsigned long long* counts;     // [4]: pixels of class RP_VALID, RP_MASKED, RP_OFFSCREEN, RP_REJECTED are added
};

// kernels_moments.hip, the noise estimate over the gw x gh pixel grid: sigma row-major W x H (null: not written; pixels outside the grid are not
// written) and the counts (MO_WORDS words, device_layout.h: estimated, above, sum_var_q16, bins; added to; null: not counted)
struct MoLaunch {
  int gw, gh;
  int W, H;
  int divide_by;
  float tolerance;
  const int32_t* acc;
  const int32_t* hist;            // null: no history plane (0 everywhere)
  const unsigned long long* m2;
  float* out_sigma;
  unsigned long long* counts;
};

// kernels_adaptive.hip (dr_render_adaptive; device_adaptive.hpp): one pass over the gx x gy tiles of the view's pixel grid -- tile t = col * gy + by,
// its lane l pixel (8 col + (l >> 3), 8 by + (l & 7)), as in the render kernels.  The selection reads the three planes and writes a flag per tile
// and the two counts; the fold adds `nframes` frame buffers (frame f at frames + f * frame_stride, the accumulator's layout) into the planes of the
// tiles a compacted list names.
struct AdParams {
  float tolerance;
  int min_samples, max_samples, tile_pixels;
};
constexpr int AD_ACTIVE = 0, AD_ASKING = 1, AD_WORDS = 2;      // the counts: active tiles, asking pixels
struct AdLaunch {
  int gx, gy;                     // the tile grid
  int W, H;                       // the accumulator: sums column-major (x * H + y) * 3, history and M2 at x * H + y
  int divide_by;
  AdParams A;
  int nframes;                    // the fold: frames per pixel
  size_t frame_stride;            // ... and the int32 words from one frame buffer to the next
  int32_t* acc;
  int32_t* hist;                  // the selection: null = no history plane (0 everywhere); the fold needs one
  unsigned long long* m2;
  const int32_t* frames;
  uint8_t* flags;                 // a byte per tile: 1 active
  unsigned* counts;               // AD_WORDS words, added to
};

// kernels_radiance.hip (dr_trace_radiance): n caller rays (origin / dir 3 floats per ray), their seeds (null: base_seed + i) and the generator outputs
// to discard after seeding (null: none), spp samples each; radiance (3 floats per ray: the samples' float sum) and bounces (closest-hit queries of all
// samples), null: not written.  max_depth, the background and backtex travel in RenderParams, where trace_path reads them.
struct RadianceLaunch {
  const float* origin; const float* dir;
  const uint64_t* seed;
  const int32_t* skip;
  unsigned n;
  int spp;
  uint64_t base_seed;
  float* radiance;
  int32_t* bounces;
  unsigned* cursor;               // persistent kernel: the ray list's cursor, zeroed on the launch's stream by the caller
};

// kernels_nearest.hip (dr_query_nearest): n query points (3 floats each), their search radii (null: unbounded) and the scene's largest
// |e1| + |e2| / radius (the pruning slack's constant).  The walk kernel writes key -- {d2 bits, slot} per query, a miss {0, -1}: what
// the finishing pass reads --, d2, distance and object; the finishing pass material, qpoint (3 per query) and uv (2).  Null: not written (key: always).
struct NearestLaunch {
  const float* point; const float* rmax;
  unsigned n;
  float lmax;
  const int32_t* slot_to_orig;    // slot -> object index of the file (read when `object` is written)
  uint32_t* key;
  float* distance; float* d2; int32_t* object;
  int32_t* material; float* qpoint; float* uv;
};

}  // namespace dr
