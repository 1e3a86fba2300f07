/*
 * dogeray_amd.h -- C ABI of the MI355X-native DOGERAY render path (libdogeray_amd.so).
 *
 * The reference (PhilipPragerUrbina/DOGERAY, raygpu/kernel.cu, cited as K:<line>) has no
 * plugin/FFI layer.  The seam this library sits behind is the free function
 *
 *     cudaError_t CudaStarter(int3* outputr, bvh* nbvhtree, singleobject* allobjects,
 *                             cudaTextureObject_t* texarray, int divisor);     K:138, K:2562-2669
 *
 * plus the host functions that feed it (getnum/read K:1113-1530, getppm* and readtextures
 * K:1915-2018, build_bvh K:1864-1909) and the ~14 globals it reads implicitly
 * (K:29-30,109,119-132).  Everything implicit there is an explicit argument here.
 *
 * Conventions
 *   - plain C types only; every function returns DR_OK (0) or a negative dr_status;
 *     dr_last_error() returns the message of the calling thread's last failure.
 *   - a dr_scene lives on the host; a dr_context owns one GPU and the resident scene.
 *   - one host thread per context at a time; calls are synchronous unless they say otherwise.
 *   - there is NO CPU fallback: device entry points fail with DR_ERR_DEVICE without a GPU.
 */
#ifndef DOGERAY_AMD_H
#define DOGERAY_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DR_ABI_VERSION 2

typedef enum dr_status {
  DR_OK = 0,
  DR_ERR_INVALID = -1, /* bad argument / call order                                   */
  DR_ERR_IO = -2,      /* file cannot be opened (reference: message box, K:1162,1524) */
  DR_ERR_PARSE = -3,   /* stof/stoi would have thrown in the reference                */
  DR_ERR_SCENE = -4,   /* scene the reference cannot build (fewer than 2 objects)     */
  DR_ERR_DEVICE = -5,  /* HIP error, or no GPU                                        */
  DR_ERR_NOMEM = -6
} dr_status;

typedef struct dr_scene dr_scene;     /* host: parsed .rts + textures + BVH */
typedef struct dr_context dr_context; /* device: one GPU, one resident scene */

const char* dr_last_error(void);
int dr_abi_version(void);

/* ------------------------------------------------------------------ host-side types ---- */

/* struct singleobject (K:48-74), field for field; bools widened to int32. */
typedef struct dr_object {
  int32_t type;      /* 0 sphere, 2 triangle (K:440-447) */
  float pos[3];      /* vertex 0 / sphere centre */
  float rot[3];      /* vertex 2 */
  float norm[3];     /* face normal, z == -20 means absent (K:55,750) */
  float n1[3], n2[3], n3[3];
  float t1[3], t2[3], t3[3];
  int32_t smooth, tex, mat;
  float dim[3];      /* vertex 1, or radius in dim[0] */
  float col[3];
  int32_t texnum, rtexnum;
  float addional[3]; /* [1] = roughness / IOR, [0] = diffuse mode (K:827,852,917) */
} dr_object;

/* struct bvh (K:79-96), field for field. */
typedef struct dr_bvh_node {
  int32_t active;
  int32_t children[2];
  int32_t count;
  int32_t hit_node, miss_node;
  int32_t under;
  float min[3], max[3];
  int32_t end;
} dr_bvh_node;

/* The globals the '*' settings line fills (K:1223-1299; defaults K:29-30,109,123-132). */
typedef struct dr_settings {
  float campos[3], look[3];
  float aperture, focus_dist;
  int32_t fov, max_depth, spp;
  float background;
  int32_t backtex;
  int32_t width, height;
} dr_settings;

/* ------------------------------------------------------------------ scene ingest -------- */

/* getnum + getppmnum/getppmpaths + read + readtextures' file loading (K:2055-2082).
 * texture_dir: directory scanned for entries whose path contains "ppm"/"PPM" (the reference
 * scans the process cwd, K:1981); NULL = current directory, "" = no textures.  Entries are
 * taken in sorted name order. */
int dr_scene_load(const char* rts_path, const char* texture_dir, dr_scene** out);
void dr_scene_free(dr_scene* s);

/* The same scene from arrays the caller already holds -- what the reference's main() has after
 * read()/build_bvh() (allobjects K:2061, nbvhtree K:2075, nanum/bvhnum K:1518,2073) and what it
 * hands to CudaStarter.  objects: n_objects + 1 entries (the reference allocates one more than it
 * fills).  bvh: bvhnum = 2 * (n_objects + 1) nodes from the caller's own build_bvh, or NULL to
 * build later with dr_scene_build_bvh.  Everything is copied.  Textures are added in index order
 * (dr_object.texnum / rtexnum and settings.backtex index this list, as texarray[] K:2077-2082). */
int dr_scene_create_from_arrays(const dr_object* objects, int n_objects, const dr_settings* settings,
                                const dr_bvh_node* bvh, int bvhnum, dr_scene** out);
int dr_scene_add_texture(dr_scene* s, const uint8_t* rgba, int width, int height, const char* name);

int dr_scene_num_objects(const dr_scene* s);            /* N = object lines (objnum - 1)   */
int dr_scene_get_objects(const dr_scene* s, dr_object* out /* N + 1 entries */);
int dr_scene_get_settings(const dr_scene* s, dr_settings* out);
int dr_scene_set_settings(dr_scene* s, const dr_settings* in);
int dr_scene_num_textures(const dr_scene* s);
int dr_scene_texture_info(const dr_scene* s, int i, int* width, int* height);
int dr_scene_texture_data(const dr_scene* s, int i, uint8_t* rgba /* w*h*4 */);

/* build_bvh (K:1864-1909): same tree, same node numbering, same float bounds.
 * nthreads <= 0: use all hardware threads. */
int dr_scene_build_bvh(dr_scene* s, int nthreads);
int dr_scene_bvh_size(const dr_scene* s);                /* bvhnum = 2 * (N + 1), K:2073   */
int dr_scene_bvh_used(const dr_scene* s);                /* actualbvhnum = 2N - 1          */
int dr_scene_get_bvh(const dr_scene* s, dr_bvh_node* out /* dr_scene_bvh_size entries */);

/* .rtsb sidecar: binary image of a loaded scene -- objects as parsed ('r' fields frozen at
 * the values this load drew), settings, decoded textures and, if built, the BVH -- so that a second start-up
 * skips getnum/read/build_bvh (K:2055-2094: 330 MB of text at 1M triangles).  The file carries the record sizes
 * of this ABI and a checksum; anything that does not match is DR_ERR_PARSE, never a partly filled scene. */
int dr_scene_save_binary(const dr_scene* s, const char* rtsb_path);
int dr_scene_load_binary(const char* rtsb_path, dr_scene** out);

/* ------------------------------------------------------------------ device -------------- */

int dr_device_count(void);
int dr_context_create(int device_ordinal, dr_context** out);
void dr_context_destroy(dr_context* c);

/* Uploads nodes, primitives, shading records and textures ONCE (the reference re-uploads all
 * of them on every CudaStarter call, K:2604-2629).  The BVH must have been built. */
int dr_context_upload_scene(dr_context* c, const dr_scene* s);

/* Framebuffer partition for multi-GPU: this context renders only the 8-pixel-wide block
 * columns bx with bx % mod == rem; other pixels stay 0.  Default (1, 0) = everything. */
int dr_context_set_stripe(dr_context* c, int mod, int rem);

/* Traversal used by the megakernel.  All return the same closest hit as hit() K:468-512.
 *   DR_TRAVERSAL_THREADED  the reference's order: hit/miss links, child 0 first (its visit counters are the
 *                          reference's: dr_stats.node_visits / prim_tests equal the oracle's V / L)
 *   DR_TRAVERSAL_ORDERED   near child first with a short per-lane stack, ties resolved to the
 *                          leaf the reference order would have reached first
 *   DR_TRAVERSAL_WIDE      (default) a 4-way tree with 8-bit child boxes over the reference's own leaves, nearest
 *                          entered child first, per-lane stack in LDS; the leaves keep the reference's exact boxes
 *                          and tie order.  A scene it cannot represent (non-finite boxes, > 2^24 records) is walked
 *                          THREADED; dr_context_get_option("traversal") tells which one launches use.         */
enum { DR_TRAVERSAL_THREADED = 0, DR_TRAVERSAL_ORDERED = 1, DR_TRAVERSAL_WIDE = 2 };
int dr_context_set_traversal(dr_context* c, int mode);

/* Tuning knobs of the render kernels; none of them changes a pixel.
 *   "kernel"        DR_KERNEL_PERSISTENT (default): waves are pools of 64 path slots that refill
 *                   from a tile queue; DR_KERNEL_TILE: one wave per 8x8 tile, the reference's launch shape
 *   "batch_frames"  most frames one launch of dr_render_accumulate covers (persistent kernel), default 32
 *   "feedback"      1 (default): tiles are started most-expensive-first using the previous launch's costs; the order of a view
 *                   is recomputed after its first two launches and then after every "feedback_every"-th (8); a view that differs
 *                   from the last one only in its settings (a moving camera) starts from the last view's order
 *                   ("order_follows_camera", default 1)
 *   "occupancy"     waves per SIMD.  Persistent kernel: 6 (default: six for the wide walk's lean build of long launches, five for
 *                   every other build), 5 or 4; tile kernel: 4 or 6
 *   "schedule"      persistent kernel: 0 (default, tuned) = shade / refill once fewer than 32 lanes walk, leaf steps once 20 lanes stand at
 *                   a leaf, two steps per loop iteration; 1 = 32 / 8 / one step; 2 = 48 / leaves tested on the spot / one step
 *   "xcd_regions"   1 (default): one tile queue per XCD, each an image band, with stealing; 0: one queue
 *   "heavy_factor"  with feedback: tiles that cost more than this many times the mean start first (most expensive
 *                   first), all others keep their natural order (default 1: the above-average tiles; 0: no tile is
 *                   reordered, -1: every tile by cost)
 *   "coop_steps"    work sharing (the tile queue is empty, or the wave holds a part of a split tile).  Wide walk: a ray older than
 *                   this many steps (default 2, 0 = off) hands the oldest word of its stack -- a subtree -- to a lane that has no
 *                   pixel, up to "coop_rounds" (2) times per loop iteration; all lanes of one ray keep the best hit in one LDS
 *                   word and the owner shades when every piece is done.  The kernel build that contains this is used for
 *                   launches with fewer than "coop_tiles_per_wave" (32) tiles per wave: short launches, whose tail shows; they
 *                   use one tile queue ("short_one_queue", default 1).
 *   "split_parts"   launches of ONE frame: the tiles whose longest pixel took "split_steps" (400) node steps in the previous
 *                   frame -- as many of them as give "split_waves" (12) per cent of the waves a part to start with -- are handed
 *                   out in this many parts (4; 1 = whole, 2, 8); the wave holds until those pixels are done and its other lanes
 *                   help with their rays from the first step
 *                   Threaded walk ("coop_steps" again): once the queue is empty, a ray older than that is finished by all 64
 *                   lanes breadth-first, in waves with at most "coop_lanes" (8) lanes walking
 *   "pipe_streams"  render streams the present pipeline alternates between (2, default, to 4); "pipe_group": most frames one launch of the pipeline
 *                   covers (1 to 16, default 8; see dr_pipeline_submit); "pipe_lean" 1: pipelined launches of ONE frame run the lean build on eight queues
 *                   instead of the work-sharing build (measured slower, default 0; groups are then not formed)
 *   "reserve_cus"   persistent kernel: workgroups are launched for this many CUs fewer than the device has (0 = all; dr_group ranks may leave
 *                   room for the gather's copy / RCCL kernels beside the next batch's rendering)
 *   "wave_log"      1: short launches record begin / queue empty / end of every wave (dr_stats_wave_log)
 *   "wide_tree"     tree under the wide walk, read at dr_context_upload_scene: 2 (default) binned surface-area heuristic, small
 *                   triangles entered with their own bounds instead of the reference's leaf box (those bounds padded by 0.01, K:353-354)
 *                   and every ray carrying the margin that keeps the accepted hits the reference's; 1 the same tree
 *                   over the reference's leaf boxes; 0 the reference's own topology (K:1745-1861) collapsed 4-way
 *   "denoise_tiles" dr_accum_denoise's a-trous passes: 1 (default) one workgroup per 16x16 lattice tile staged in LDS, 0 every tap loaded from
 *                   the planes; the same bits either way
 *   "camera_cert"   1 (default): per view, the camera rays of tiles where no small triangle can be hit near-grazing carry a smaller margin
 *                   (the grazing certificate); 0 every ray carries the scene's margin.  The same bits either way.  Used by the
 *                   lean and counting builds of the persistent kernel, for the first sample of each pixel (spp > 1: later samples keep the scene's
 *                   margin); a single-frame launch of a view not seen before computes no mask
 *   "cert_factor"   the certified |d . (e1 x e2)| in units of the 1e-4 cut-off (default 40)
 *   "cert_levels"   1 (default): the certificate is graded.  Every tile is measured against the ladder cert_factor x {1/4, 1/2, 1, 2, 4} (10, 20, 40,
 *                   80, 160 at the default factor; every step at least 1) and its camera rays carry the margin of the highest step it passes, the
 *                   scene's margin when it passes none (dr_stats_cert_levels); 0 one step, cert_factor: a tile passes it or keeps the scene's
 *                   margin.  The same bits either way
 *   "camera_entry"  1 (default): per view, the camera rays of a tile start their walk at the tile's entry record -- the lowest record of the wide tree
 *                   that holds every leaf a camera ray of the tile can reach (dr_stats_camera_entry) -- instead of the root; a tile
 *                   that sees nothing of the scene walks nothing.  0 every ray starts at the root.  The same bits either way.  Used where the
 *                   certificate is (the lean and counting builds, a pixel's first sample), built and dropped with it, for any scene with a wide tree
 *   "sky_tiles"     a launch of the lean build over a view with an entry table takes the tiles no leaf can be seen from (entry code -1) out of the
 *                   persistent kernel's queues (dr_stats_sky_tiles) and renders them without a walk or a path pool, a wave per tile
 *                   with the frames summed in registers: 2 (default) in the persistent kernel's own waves once all their lanes have retired, in
 *                   the time the launch waits for its slowest wave; 1 in a kernel of their own in front of the persistent kernel; 0 every tile
 *                   goes through the persistent kernel's queues.  The same bits with every value.  Not used by the counting and work-sharing
 *                   builds nor by pipelined launches
 *   "sample_order"  which of a tile's 64 x B samples share a unit of the persistent kernel's queue in a launch of B frames (batch_frames, a pipelined
 *                   group): 0 a unit is the tile's 64 pixels of one frame; 1 (default) a unit is consecutive frames of one or two pixels
 *                   of the tile, so the lanes a wave refills together are jittered samples of the same pixel.  A pixel's arithmetic depends on
 *                   (x, y, frame) only and the batch is summed in integers: the same bits either way.  Launches of one frame are the same launch
 *   "queue_cursor_stride" words between the cursors of two tile queues in a launch's block of the persistent kernel's cursor ring: 32
 *                   (default) a 128-byte line per cursor, 1 the cursors packed into consecutive words; 1 .. 1024.  The same bits with every value
 *   "queue_cursor_skew" (a measuring aid) 0 (default) the launches' blocks follow each other in the ring; s = 1 .. 31: every launch's block starts s
 *                   words into a 128-byte line, which pins the alignment a packed block otherwise gets from the launch's number.  The same bits
 *   "cert_flagged_permille" (read only) per mille of the last certified view's tiles whose camera rays keep the scene's margin; -1 none
 *   "reproject_aov_passes" (read only) first-hit AOV passes the last dr_accum_reproject traced: 2 with a cold guide cache, 1 when its `from`
 *                   view was the previous call's `to` view (0 / 1 when both views are the same settings)
 *   "upscale_aov_passes" (read only) first-hit AOV passes the last dr_accum_upscale traced: 2 with cold guide caches, 1 when only the low or only the
 *                   full-resolution guides were cached (the same view at another divisor), 0 on a repeat and in block mode
 *   "moments"       read by dr_accum_reset: 1 gives the accumulator a second-moment plane (one uint64 per pixel, see dr_accum_error below), 0
 *                   (default) drops it; a context that never sets it allocates nothing and runs the code it ran before.  No pixel of the
 *                   accumulator changes; dr_render_accumulate then runs through the pipeline
 *   "denoise_variance" 1: while the accumulator has a second-moment plane, dr_accum_denoise's variance pre-pass takes the temporal variance of pixels
 *                   with four samples or more from it (SVGF's rule; see dr_accum_error below); 0 (default): the spatial estimate everywhere, the bits as before
 *   "trace_kernel"  (private, for the tests) which kernel dr_trace_rays runs: 0 (default) the launch plan decides by the ray count, 1 the one-ray-per-lane
 *                   kernel, 2 the persistent kernel wherever it exists (the wide walk over a scene with a wide tree).  The same bits either way
 *   "radiance_kernel" (private, for the tests) which kernel dr_trace_radiance runs: 0 (default) the launch plan decides by the ray count, 1 the
 *                   one-ray-per-lane kernel, 2 the persistent kernel wherever it exists (the wide walk over a scene with a wide tree).  The same bits either way
 *   "allhits_kernel" (private, for the tests) which kernel dr_trace_all_hits runs: 0 (default) the launch plan decides by the ray count, 1 the
 *                   one-ray-per-lane kernel, 2 the persistent kernel wherever it exists (a scene with a wide tree).  The same bits either way
 *   "guide_frames"  where dr_accum_denoise and dr_accum_upscale (both of its guide sets) take their guides from: 0 (default) the pinhole pass of
 *                   dr_render_aov, the code and the bits as before; G = 1 .. 256: the lens-averaged pass of dr_render_aov_lens in its guide form over
 *                   nframes = G, frame_seed = DR_GUIDE_SEED, seed_stride = 1, so that with aperture > 0 the edge stops and the albedo see the blur the
 *                   renderer integrates.  G * (int)settings13[10] > 256 is refused by the call that traces (DR_ERR_INVALID).  The cached guides are
 *                   keyed by it: a change in either direction traces again.  dr_accum_reproject keeps its pinhole pair: it reprojects positions
 *   "aov_lens_loop" (private, for the tests and the A/B) the loop shape of dr_render_aov_lens's kernel: 0 (default, the faster one as measured) the
 *                   nested loop, every sample's walk waiting for the wave's slowest lane; 1 one walk loop per wave whose lanes start their next
 *                   sample as soon as their walk ends.  The same bits either way
 * The environment variable DOGERAY_OPTIONS="name=value,..." applies the same at context creation. */
enum { DR_KERNEL_TILE = 0, DR_KERNEL_PERSISTENT = 1 };
int dr_context_set_option(dr_context* c, const char* name, int value);
/* Read a knob back (same names), or of the uploaded scene: "tree_depth" (reference tree), "wide_depth" / "wide_nodes"
 * (wide walk; 0 = not representable), "wide_own_bounds" (triangles that entered the wide tree with their own bounds, wide_tree = 2),
 * "traversal" (the one launches really use). */
int dr_context_get_option(const dr_context* c, const char* name, int* value);

/* One CudaStarter call.  settings13 = { cam.xyz, look.xyz, aperture, focus, fov, max_depth,
 * spp, divisor, backtex } exactly as packed at K:2581; W,H = SCREEN_WIDTH/HEIGHT;
 * background = backgroundintensity[0] (K:108,2103); frame_seed replaces clock() at K:1065.
 * out_int3 (host, may be NULL) receives int32[W*H*3], pixel (x,y) at (x*H + y)*3 (K:1006):
 * trunc(mean colour * 255), unclamped; pixels outside the rendered sub-rectangle are 0. */
int dr_render_frame(dr_context* c, const float settings13[13], int W, int H, float background,
                    uint64_t frame_seed, int32_t* out_int3);

/* Progressive accumulation kept on the device (the reference accumulates on the CPU,
 * K:2213-2218).  dr_accum_reset zeroes the W*H*3 int32 accumulator; dr_render_accumulate
 * renders `nframes` frames with seeds frame_seed + k*seed_stride and adds each into it
 * (no host synchronisation between frames; returns after the last one has finished).  While the accumulator has a second-moment
 * plane (option "moments") dr_render_accumulate runs as dr_render_accumulate_pipelined -- the same sums, every kernel and traversal option;
 * dr_stats are what that call leaves -- and dr_render_accumulate_async returns DR_ERR_INVALID. */
int dr_accum_reset(dr_context* c, int W, int H);
int dr_render_accumulate(dr_context* c, const float settings13[13], int W, int H, float background,
                         uint64_t frame_seed, uint64_t seed_stride, int nframes);
/* The same without the final wait: the launches are queued on the context's stream and the call returns; at most two
 * such batches are in flight (a third call waits for the first).  dr_context_synchronize waits for everything queued
 * and brings dr_stats up to date.  Used to overlap the multi-GPU gather of one batch with the rendering of the next. */
int dr_render_accumulate_async(dr_context* c, const float settings13[13], int W, int H, float background,
                               uint64_t frame_seed, uint64_t seed_stride, int nframes);
int dr_context_synchronize(dr_context* c);

/* ---- the present loop at the batched rate: pipelined single frames.
 * The reference renders ONE frame per CudaStarter call, adds it to `outr` and shows the running mean (K:2154-2224, K:2213-2218,
 * K:2287).  A launch of one frame ends with its slowest pixels while most of the GPU idles.  Here frames are SUBMITTED one by one and every
 * frame still renders into a buffer of its own, but
 *   - frames submitted one after the other for the same view with seeds in arithmetic progression (what a progressive render submits) share
 *     one LAUNCH: a group of up to "pipe_group" (option, default 8; 1 = a launch per frame) frames, rendered by the kernel's batch queue into
 *     that many buffers -- a launch long enough to run the lean build and to hide its tail;
 *   - group k + 1 starts on a second stream while group k drains ("pipe_streams", default 2; streams + 1 groups of buffers rotate);
 *   - a third stream adds the finished frames to the accumulator ONE BY ONE IN TICKET ORDER, so what dr_pipeline_wait(ticket) hands out --
 *     clamp(sum of frames <= ticket / present_divide_by, 0, 255), row-major RGB8 as dr_accum_present -- is exactly the image the reference
 *     shows after that frame.
 *   dr_pipeline_submit   queues one frame (same arguments as dr_render_frame; the frame must match dr_accum_reset's size);
 *                        present_divide_by != 0 also queues the display divide and its download.  Returns at once; *ticket = 0, 1, 2 ...
 *                        The frame's group is launched when it is full, when a frame that does not continue it is submitted, or when it is waited for.
 *   dr_pipeline_wait     blocks until that frame has been added (and presented); out_rgb8 may be NULL.  A caller that keeps two groups' worth of
 *                        frames in flight gets the batched rate; one that waits for every frame before it submits the next gets groups of one
 *                        (the rate of round 3's pipeline).
 *   dr_render_accumulate_pipelined   nframes frames, no presents: dr_render_accumulate's result through the pipeline.
 * Every ticket handed out stays waitable until it has been waited for, however many groups have been launched since: the image of a frame that was
 * presented is kept until dr_pipeline_wait(ticket) has returned and the next group is launched after that; a frame without a present whose buffers
 * have been reused has finished, and dr_pipeline_wait(ticket, NULL) returns DR_OK for it.  At most 32 images are kept for frames whose buffers have
 * been reused: dr_pipeline_submit returns DR_ERR_INVALID ("... call dr_pipeline_wait for the oldest tickets first") for a frame that could take
 * them beyond that -- it refuses, it never drops an image.  A ticket that was never handed out is DR_ERR_INVALID.  Setting "pipe_streams" to another
 * value drains the pipeline and starts again from ticket 0; earlier tickets are gone.
 * A frame is launched with the state it was submitted under: a scene upload, dr_context_set_stripe, dr_context_set_traversal,
 * dr_stats_enable_counters and dr_context_set_option first launch the frames still held, and apply to frames submitted AFTER them.  Any other call
 * on the context -- the dr_stats_* readers, dr_accum_device_ptr and its kin, and the probes among them -- is ordered behind the frames submitted
 * before it (their groups are launched first, and the context's stream waits for them). */
int dr_pipeline_submit(dr_context* c, const float settings13[13], int W, int H, float background, uint64_t frame_seed,
                       int present_divide_by, uint64_t* ticket);
int dr_pipeline_wait(dr_context* c, uint64_t ticket, uint8_t* out_rgb8);
/* the presented image of a ticket that has been waited for, in place: a pointer into the library's pinned download buffer (W * H * 3 bytes, row-major
 * RGB8), valid until the next call that may launch a group (dr_pipeline_submit, and any call ordered behind held frames): the launch may reuse or release
 * it -- for a caller that uploads it to a texture anyway (K:2243-2275) and would rather not copy 6 MB per frame twice */
int dr_pipeline_image(dr_context* c, uint64_t ticket, const uint8_t** rgb8);
int dr_render_accumulate_pipelined(dr_context* c, const float settings13[13], int W, int H, float background,
                                   uint64_t frame_seed, uint64_t seed_stride, int nframes);
/* The HIP stream (hipStream_t) every launch of this context is queued on, for callers that order their own device work
 * (a collective on packed stripes) against it with events. */
int dr_context_stream(dr_context* c, void** hip_stream);
int dr_accum_read(dr_context* c, int32_t* out_int3 /* W*H*3 */);
/* The display divide of K:2287: rgb8[(y*W + x)*3 + ch] = clamp(acc / divide_by, 0, 255).  While the accumulator has a history plane
 * (dr_accum_reproject) pixel p divides by hist[p] + divide_by, and a divisor of 0 gives 0. */
int dr_accum_present(dr_context* c, int divide_by, uint8_t* out_rgb8 /* W*H*3, row-major */);
/* Device address of the accumulator (int32[W*H*3]) for device-side gathers (RCCL); dr_accum_reproject swaps between two buffers, this is
 * the current one. */
int dr_accum_device_ptr(dr_context* c, void** dev_ptr, uint64_t* bytes);
/* The history plane (dr_accum_reproject): int32 per pixel, pixel (x, y) at x * H + y like the accumulator -- the samples acc[p] carries in
 * addition to the frames the caller counts itself.  Without a plane (no reprojection since the last dr_accum_reset) dr_accum_history_read
 * writes zeros and dr_accum_history_device_ptr gives NULL / 0 bytes. */
int dr_accum_history_read(dr_context* c, int32_t* out /* W*H */);
int dr_accum_history_device_ptr(dr_context* c, void** dev_ptr, uint64_t* bytes);
/* Multi-GPU gather, device side.  The framebuffer is column-major (K:1006), so one 8-pixel block column is one
 * contiguous run of 8*H*3 int32 and a context's stripe (dr_context_set_stripe: columns rem, rem+mod, ...) packs into
 * [ncols][8*H*3].  dr_accum_pack_stripe queues that copy on the context's stream into one of two library-owned
 * buffers (slot 0/1: pack batch k+1 while batch k is still being sent) and returns its device address and size.
 * dr_accum_unpack_stripes, on the gathering rank, copies the packed stripes of ranks first_rank .. world-1 (rank r's at
 * packed_dev + r * rank_stride_bytes, rank_stride_bytes a multiple of 16) into its own accumulator's columns
 * r, r+world, ..., on hip_stream (NULL: the context's stream).  Ranks render disjoint columns, so the unpack may run
 * beside the gathering rank's own rendering. */
int dr_accum_pack_stripe(dr_context* c, int slot, void** dev_ptr, uint64_t* bytes);
/* allocates pack buffer `slot` for the current accumulator and stripe without packing (so that no allocation falls into a
 * timed or latency-critical gather; dr_group_accum_reset does this for every rank) */
int dr_accum_reserve_pack(dr_context* c, int slot);
int dr_accum_unpack_stripes(dr_context* c, const void* packed_dev, uint64_t rank_stride_bytes, int world, int first_rank,
                            void* hip_stream);

/* ------------------------------------------------------------------ first-hit AOVs ------ */
/* What a pixel SEES, as buffers ("arbitrary output variables"): depth, normal, albedo, object id ... of the first hit of one camera ray per pixel
 * -- for picking the object under a cursor, focusing on it (the reference sets the focus distance by hand, Z/X keys K:2471-2483), denoiser
 * guides, datasets.
 *   pixel grid  the one dr_render_frame renders: (W / div / 8) * 8 x (H / div / 8) * 8 pixels, div = (int)settings13[11] (K:2633-2636)
 *   ray         the pinhole ray through the pixel CENTRE: nu = (float)(((double)x + 0.5) / den_w), nv likewise with y (den_w / den_h as
 *               K:1067-1068); origin = lookfrom, direction = llc + nu * horizontal + nv * vertical - lookfrom (K:1030-1073 without the jitter
 *               and without the lens offset: the aperture is ignored)
 *   first hit   hit() K:468-512 on the uploaded scene with the context's traversal (dr_context_set_traversal: all give the same hit)
 * Channels (NULL: not computed), each a buffer of its own, row-major: pixel (x, y) of the window at (y - y0) * w + (x - x0) -- row index = the
 * renderer's y, the order of dr_accum_present's image --, vector channels with their components consecutive per pixel:
 *   t         f32    hit()'s ray parameter (bit-identical to dr_kat_hit on the same ray); on a miss -1
 *   distance  f32    t * sqrtf(dx * dx + dy * dy + dz * dz), in that order; +inf on a miss
 *   depth     f32    t * settings13[7]: the distance along the view axis (every pinhole direction's component along -w is the focus distance,
 *                    K:1047-1049); +inf on a miss
 *   object    i32    index of the object in dr_scene_get_objects order, as dr_kat_hit reports it; -1 on a miss (hit() says 0, K:507)
 *   material  i32    the object's mat (K:852-944); -1 on a miss
 *   normal    3 f32  the shading normal as raycolor forms it: getnormal, flipped to face the ray (K:807-825); 0 on a miss
 *   uv        2 f32  the interpolated texture coordinate texco.x, texco.y (K:728-745); 0 on a miss
 *   albedo    3 f32  ocolor as raycolor forms it (K:826-844): the texture at (u, 1 - v), the checker, or col -- for emissive materials the
 *                    emitted colour; 0 on a miss
 *   dir       3 f32  the ray direction as traced (unnormalised) */
typedef struct dr_aov_buffers {
  float* t;
  float* distance;
  float* depth;
  int32_t* object;
  int32_t* material;
  float* normal;   /* w * h * 3 */
  float* uv;       /* w * h * 2 */
  float* albedo;   /* w * h * 3 */
  float* dir;      /* w * h * 3 */
} dr_aov_buffers;
/* The channels of the window (x0, y0, w, h) of the pixel grid (1 x 1: a pick).  device_pointers = 0: host buffers, the call returns when they are
 * filled; 1: device buffers on this context's GPU, the work is queued on dr_context_stream and the call returns at once.  Ordered behind the
 * frames submitted before it (dr_pipeline_submit); changes neither the accumulator, nor dr_stats, the stripe or any option.  The settings are
 * accepted or refused as by dr_render_frame; no scene, an empty window or one not inside the grid: DR_ERR_INVALID.  The first call after a scene
 * upload copies the slot -> object map to the device. */
int dr_render_aov(dr_context* c, const float settings13[13], int W, int H, int x0, int y0, int w, int h, const dr_aov_buffers* buffers,
                  int device_pointers);

/* ------------------------------------------------------------------ lens-averaged AOVs -- */
/* The same window of the same pixel grid, seen through the rays the RENDERER traces: the jittered rays that leave from a point on the lens
 * (K:1065-1073, lens radius settings13[6] / 2, K:1052), averaged over N samples per pixel.  With aperture > 0 a defocused edge is a ramp of coverage
 * and a blend of albedos here, where dr_render_aov shows the sharp pinhole edge; with aperture 0 what remains is the pixel jitter.
 *   samples     of pixel (x, y): frame k = 0 .. nframes - 1 outer, sample s = 0 .. spp - 1 inner, spp = (int)settings13[10]; N = nframes * spp,
 *               1 <= N <= 256 (one call costs about N pinhole passes)
 *   ray         sample (k, s) seeds a fresh generator with frame_seed + k * seed_stride + s * 0x9E3779B97F4A7C15 + (x + y * 8 * gx) (64-bit
 *               wrapping; gx = W / div / 8: the unstriped view's launch width, K:1065) and draws the jitter and the lens point as K:1066-1073 do:
 *               exactly the camera rays dr_render_accumulate(settings13, W, H, ., frame_seed, seed_stride, nframes) traces on an unstriped context,
 *               and dr_kat_camera's (frame seed frame_seed + k * seed_stride, stride 8 * gx)
 *   per sample  the closest hit (hit() K:468-512, as dr_render_aov) and, there, what dr_trace_rays' surface channels report: t, distance, the
 *               facing normal, ocolor, mat.  h = the number of samples that hit
 * Every sum below is a plain float + in sample order starting from 0 (a product is rounded before it is added: no FMA contraction), every quotient
 * one division at the end; there is no random draw beyond the camera ray's and no counter.  Channels (NULL: not computed), laid out as dr_render_aov's:
 *   coverage  f32    (float)h / (float)N                                                        h = 0: 0
 *   depth     f32    (sum over the hits of t * settings13[7]) / (float)h: the lens offset lies in the u, v plane, so every lens ray keeps the focus
 *                    distance as its component along -w (K:1047-1049) and t * focus is still the distance along the view axis      h = 0: +inf
 *   distance  f32    (sum over the hits of dr_trace_rays' distance) / (float)h                  h = 0: +inf
 *   normal    3 f32  (sum over the hits of the facing normal, K:807-825) / (float)h, not renormalised: shorter where the normals disagree    h = 0: 0
 *   albedo    3 f32  (sum over the hits of ocolor, K:826-844) / (float)N: premultiplied by coverage    h = 0: 0
 *   material  i32    the Boyer-Moore majority candidate of the per-sample values in sample order, a sample's value being its mat (K:852-944) on a
 *                    hit and -1 on a miss: cnt = 0; for each value v: if cnt == 0 { cand = v; cnt = 1 } else if v == cand cnt++ else cnt--; the
 *                    result is cand -- the majority whenever there is one.  material != -1 implies h >= 1              h = 0: -1
 * The GPU is bit-identical to the host build of the same source (dogeray_amd/csrc/device_aov_lens.hpp) and to the fold of dr_kat_camera's rays
 * through dr_trace_rays written out in tests/aov_lens_checks.py, with every traversal and every loop shape (option "aov_lens_loop").
 * Not here: t, uv, dir and object channels, stripes and dr_group, more than 256 samples per call. */
#define DR_GUIDE_SEED 0x67756964656C656Eull /* the frame_seed of the guides option "guide_frames" traces ("guidelen") */
typedef struct dr_aov_lens_buffers {
  float* coverage;
  float* depth;
  float* distance;
  int32_t* material;
  float* normal;   /* w * h * 3 */
  float* albedo;   /* w * h * 3 */
} dr_aov_lens_buffers;
/* The channels of the window (x0, y0, w, h) of the pixel grid.  Windows, host / device buffers, stream ordering and error codes as dr_render_aov;
 * changes neither the accumulator, nor dr_stats, the stripe or any option (the context's stripe is ignored: the view is the unstriped one).
 * DR_ERR_INVALID also for N = nframes * spp outside 1 .. 256. */
int dr_render_aov_lens(dr_context* c, const float settings13[13], int W, int H, int x0, int y0, int w, int h, uint64_t frame_seed, uint64_t seed_stride,
                       int nframes, const dr_aov_lens_buffers* buffers, int device_pointers);

/* ------------------------------------------------------------------ ray queries --------- */
/* Closest hit and occlusion on the CALLER's rays -- line of sight, ambient occlusion, baking, picking along arbitrary rays, a tensor of rays in a
 * learning loop, shadow rays: what rtcIntersect / rtcOccluded are elsewhere.  Rays are three arrays; ray i is origin[3i..], dir[3i..], tmax[i].
 *
 * DR_TRACE_CLOSEST.  The answer for ray i is hit()'s own answer (K:468-512) on the resident scene if its t <= min(tmax_i, 10000), else a miss -- for
 * every ray, without exception.  A hit at exactly t == tmax_i is kept; a NaN tmax, or one <= 0, is a miss.  The channels (NULL: not computed) have the
 * meaning, the miss values and the bit patterns of dr_render_aov's channels of the same name -- t -1, object -1, material -1, distance +inf, normal /
 * uv / albedo 0 -- with the ray's own origin in place of the camera.
 *   tmax decides at the end of the walk; it does not prune the walk.  hit() with its running best started at (tmax, no slot) would skip every box
 *   entered behind tmax, and that is the same answer only while no leaf's computed box entry exceeds the computed t of the primitive inside it.  It
 *   does at coordinates around 2^20 and for a few accepted hits of grazing rays and sliver triangles (a few rays in a thousand of the adversarial
 *   classes of tests/ray_cases.py): there the pruned walk reports a miss in front of a hit at t <= tmax_i.  This call does not.
 * DR_TRACE_ANY.  occluded[i] = 1 exactly when the closest-hit query above would return a hit, else 0; the walk stops as soon as that is known (it
 * holds a primitive at t <= tmax_i), and which primitive that was is not exposed: every channel other than `occluded` must be NULL (DR_ERR_INVALID
 * otherwise).  In closest mode a non-NULL `occluded` is DR_ERR_INVALID.
 *
 * device_pointers = 0: host buffers, the call returns when they are filled; 1: every pointer is device memory on this context's GPU, the work is
 * queued on dr_context_stream and the call returns at once (dr_render_aov's convention).  Ordered behind the frames submitted before it; changes
 * neither the accumulator, nor dr_stats, the stripe or any option.  Works with every traversal (dr_context_set_traversal; a scene without a wide
 * tree walks the threaded links).  DR_ERR_INVALID: no scene, n < 0 or n >= 2^31, a null origin or dir, no output channel, a mode other than the
 * two.  n == 0 is DR_OK and launches nothing.  The per-ray scratch the call needs belongs to the context, grows on demand and goes with
 * dr_context_destroy; a context that never traces allocates nothing. */
enum { DR_TRACE_CLOSEST = 0, DR_TRACE_ANY = 1 };
typedef struct dr_ray_buffers {
  const float* origin;   /* n * 3 */
  const float* dir;      /* n * 3, as traced: not normalised, t is in units of |dir| like hit()'s */
  const float* tmax;     /* n, or NULL: every ray hit()'s own cap (10000) */
} dr_ray_buffers;
typedef struct dr_hit_buffers {   /* NULL: not computed */
  float* t;
  int32_t* object;
  int32_t* material;
  float* distance;
  float* normal;         /* n * 3 */
  float* uv;             /* n * 2 */
  float* albedo;         /* n * 3 */
  int32_t* occluded;     /* DR_TRACE_ANY only: 1 / 0 */
} dr_hit_buffers;
int dr_trace_rays(dr_context* c, int mode, int64_t n, const dr_ray_buffers* rays, const dr_hit_buffers* hits, int device_pointers);

/* ------------------------------------------------------------------ radiance queries ---- */
/* The LIGHT along the caller's rays: raycolor (K:787-982) on ray i = (origin[3i..], dir[3i..]) instead of a camera ray -- a lightmap or an irradiance
 * probe, a reflection probe or a 360-degree panorama (tools/panorama.py), a fisheye or orthographic view, the radiance target of a batch of training
 * rays.  The materials' scatter, the texel fetch, the background and the generator are the renderer's own, bit for bit.
 *
 * Sample s (0 <= s < spp) of ray i runs
 *   Xorwow::init(S_i + s * 0x9E3779B97F4A7C15), S_i = rays->seed ? seed[i] : params->seed + (uint64_t)i, both sums wrapping (curand_init(seed, 0, 0),
 *     K:1065, with the caller's word where Kernel has the pixel's);
 *   then skip[i] calls of next(), their outputs discarded (curand(), K:644) -- so that a caller who drew a camera ray of its own from the same
 *     generator continues where that left off;
 *   then raycolor from (origin_i, dir_i) with attenuation 1, depth params->max_depth (settings13[9]'s meaning), bgint params->background and
 *     backtex params->backtex (settings13[12]'s meaning: -1 the sky gradient K:971-974, else the environment texture K:953-966).
 * radiance[i] = the float sum of the samples' results in sample order, starting from 0: Kernel's color = color + raycolor(...) (K:1076).  The sum is
 * NOT divided by spp and NOT quantised (K:1081-1085 does both for a pixel): the caller divides, and the bits stay defined.
 * bounces[i] = the closest-hit queries (hit(), K:801) of all samples of ray i.
 *
 * device_pointers = 0: host buffers, the call returns when they are filled; 1: every pointer is device memory on this context's GPU, the work is
 * queued on dr_context_stream and the call returns at once (dr_trace_rays' convention).  Ordered behind the frames submitted before it; changes
 * neither the accumulator, nor dr_stats, the stripe or any option.  Works with every traversal (a scene without a wide tree walks the threaded
 * links); every walk starts at the root with the margin of a scattered ray -- the rays are the caller's, so there is no camera certificate and no
 * entry table.  DR_ERR_INVALID: no scene, n < 0 or n >= 2^31, a null origin or dir, no output, spp < 1, max_depth < 1, a backtex that
 * dr_render_frame would refuse for the resident scene (a texture that is not loaded), and -- host pointers -- a negative skip.  With device pointers
 * the skips are not read by the host: a negative skip discards nothing, as 0.  n == 0 is DR_OK and launches nothing.  The scratch the call needs
 * belongs to the context, grows on demand and goes with dr_context_destroy; a context that never calls this allocates nothing. */
typedef struct dr_radiance_params {
  int      spp;         /* samples per ray, >= 1 */
  int      max_depth;   /* raycolor's depth (settings13[9]'s meaning), >= 1 */
  float    background;  /* bgint, as dr_render_frame's `background` */
  int      backtex;     /* settings13[12]'s meaning: -1 the sky gradient, else a texture */
  uint64_t seed;        /* base seed */
} dr_radiance_params;
int dr_radiance_defaults(dr_radiance_params* p);   /* 1, 10, 1.0f, -1, 0 */
typedef struct dr_radiance_rays {
  const float*    origin;  /* n * 3 */
  const float*    dir;     /* n * 3, as traced, not normalised */
  const uint64_t* seed;    /* n, or NULL: params->seed + i */
  const int32_t*  skip;    /* n, or NULL: generator outputs discarded after seeding, >= 0 */
} dr_radiance_rays;
typedef struct dr_radiance_out {   /* NULL: not computed; at least one non-NULL */
  float*   radiance;   /* n * 3 */
  int32_t* bounces;    /* n: closest-hit queries made, summed over the samples */
} dr_radiance_out;
int dr_trace_radiance(dr_context* c, int64_t n, const dr_radiance_rays* rays, const dr_radiance_params* params, const dr_radiance_out* out,
                      int device_pointers);

/* ------------------------------------------------------------------ point queries ------- */
/* How far is a point from the resident scene, and where is the nearest surface point -- unsigned distance fields, snapping probes off walls, collision
 * radii, sphere-tracing grids: what rtcPointQuery, Open3D's compute_closest_points and trimesh's nearest are elsewhere.  Query i is point[3i..] and
 * rmax[i].
 *
 * Per primitive, nearest_prim (dogeray_amd/csrc/device_nearest.hpp) gives the squared distance d2, the nearest point and its barycentrics (u, v):
 * a triangle v0 + u e1 + v e2 with the point translated to the origin first, a sphere | |p - c| - r |; degenerate triangles answer as the segment or
 * point they are, objects of other types and spheres of negative radius never answer.  The answer of a query is the minimum of (bits of d2, leaf
 * order) over all primitives -- a tie goes to the primitive the renderer's own traversal reaches first -- and it is a hit when d2 <= rmax * rmax
 * rounded to float.  rmax NULL or +inf: unbounded.  A NaN or negative rmax, or a point with a non-finite component: a miss, nothing is walked.
 * No traversal, tree (option wide_tree) or fallback changes a bit of it: the walks prune with a proven slack.
 *   distance  sqrtf(d2), -1 on a miss          d2      the key's float, 0 on a miss
 *   object    index in the scene file, -1      material the object's mat, -1
 *   point     the nearest surface point, 0     uv      its barycentrics (a sphere: 0, 0), 0
 * sqrtf(d2) is within 32 * 2^-24 * (d + 2 Lmax) of the true distance d, Lmax the scene's largest |e1| + |e2| or radius, for points and scenes
 * below 2^30.  Unsigned: which side of a surface the point is on is not answered.
 *
 * device_pointers = 0: host buffers, the call returns when they are filled; 1: every pointer is device memory on this context's GPU, the work is
 * queued on dr_context_stream and the call returns at once (dr_trace_rays' convention).  Ordered behind the frames submitted before it; changes
 * neither the accumulator, nor dr_stats, the stripe or any option.  A scene with a wide tree is walked through it whatever the traversal option
 * says; one without walks the threaded links.  DR_ERR_INVALID: no scene, n < 0 or n >= 2^31, a null `point`, no output channel.  n == 0 is DR_OK
 * and launches nothing.  The scratch the call needs belongs to the context, grows on demand and goes with dr_context_destroy. */
typedef struct dr_point_buffers {
  const float* point;    /* n * 3 */
  const float* rmax;     /* n, or NULL: unbounded */
} dr_point_buffers;
typedef struct dr_nearest_buffers {   /* NULL: not computed; at least one non-NULL */
  float* distance;
  float* d2;
  int32_t* object;
  int32_t* material;
  float* point;          /* n * 3 */
  float* uv;             /* n * 2 */
} dr_nearest_buffers;
int dr_query_nearest(dr_context* c, int64_t n, const dr_point_buffers* pts, const dr_nearest_buffers* out, int device_pointers);

/* ------------------------------------------------------------------ all hits ------------ */
/* EVERY surface a caller ray goes through, not only the first -- thickness and entry / exit pairs, x-ray and transparency compositing, crossing counts
 * that decide inside or outside, the multi-hit lists of acoustic or RF propagation: what an RTC_FILTER that never accepts collects elsewhere.  Rays are
 * dr_trace_rays' three arrays; cap_i = min(tmax_i, 10000), tmax NULL: 10000; a NaN or non-positive tmax_i gives count 0 and nothing is walked.
 *
 * The primitive at leaf-order slot s is CROSSED by ray (o, d, cap) when all of these hold: its kind is in kind_mask; slab(o, 1 / d, box) passes on the
 * box stored in its leaf record -- the reference's padded box, in both trees --; t = prim_hit_kind(...) satisfies 0 < t <= cap.  That is hit()'s own
 * acceptance rule (K:484-488) without its running best.  The answer of a ray is the SET of crossed slots ordered by (bits of t, slot) ascending: each
 * slot at most once, every tie on t present, lower slot first.  The definition uses no tree, and no traversal, tree (option wide_tree), kernel or
 * fallback changes a bit of it: the walks prune nothing by t (DESIGN.md 4.19 has the reachability argument; no class of rays is excepted).
 *   count     int32 n          the size of the whole set, also when it exceeds max_hits
 *   t         float n * K      the K = max_hits smallest, in order; -1 in unused entries
 *   object    int32 n * K      index in the scene file, -1           material  int32 n * K   the object's mat, -1
 *   distance  float n * K      t * |dir|, 0                          normal / uv / albedo    n * K * 3 / 2 / 3 as dr_trace_rays', 0
 * The first entry is NOT by definition dr_trace_rays' closest hit: hit()'s answer depends on the order in which boxes are entered for the rare accepted
 * hits whose float t lies in front of their own padded box, so the first entry's t is <= the closest hit's t whenever both report a hit, and equal
 * on well-conditioned rays.
 *
 * max_hits 0 .. DR_ALLHITS_MAX; 0 returns the count only, and every pointer other than `count` must be NULL then.  A caller who needs more than
 * DR_ALLHITS_MAX entries pages with a larger origin offset of their own.  kind_mask: DR_ALLHITS_TRIANGLES | DR_ALLHITS_SPHERES (default both; at least one).
 * A sphere answers with hit_sphere's one root (its entry), as everywhere in this library.
 *
 * device_pointers, the stream, the ordering behind submitted frames and the side effects (none) are dr_trace_rays'.  A scene with a wide tree is
 * walked through it whatever the traversal option says; one without walks the threaded links.  DR_ERR_INVALID: no scene, n < 0 or n >= 2^31, a null
 * origin or dir, no output channel, max_hits or kind_mask out of range, a K-shaped channel with max_hits 0.  n == 0 is DR_OK and launches nothing.
 * params NULL: the defaults. */
#define DR_ALLHITS_MAX 8
enum { DR_ALLHITS_TRIANGLES = 1, DR_ALLHITS_SPHERES = 2 };
typedef struct dr_allhits_params {
  int max_hits;          /* K: listed hits per ray, default 4 */
  int kind_mask;         /* default DR_ALLHITS_TRIANGLES | DR_ALLHITS_SPHERES */
} dr_allhits_params;
typedef struct dr_allhits_buffers {   /* NULL: not computed; at least one non-NULL */
  int32_t* count;        /* n */
  float* t;              /* n * K */
  int32_t* object;       /* n * K */
  int32_t* material;     /* n * K */
  float* distance;       /* n * K */
  float* normal;         /* n * K * 3 */
  float* uv;             /* n * K * 2 */
  float* albedo;         /* n * K * 3 */
} dr_allhits_buffers;
int dr_allhits_defaults(dr_allhits_params* params);
int dr_trace_all_hits(dr_context* c, int64_t n, const dr_ray_buffers* rays, const dr_allhits_params* params, const dr_allhits_buffers* out,
                      int device_pointers);

/* ------------------------------------------------------------------ denoiser ------------ */
/* An edge-avoiding a-trous wavelet filter over the accumulator (Dammertz et al. 2010; the spatial part of SVGF, Schied et al. 2017), guided by
 * the first-hit AOVs of the same settings13 (dr_render_aov).  No temporal reprojection here: the accumulator is the temporal mean already
 * (dr_accum_reproject carries it across a camera move; the filter then reads each pixel's own divisor).  Every
 * weight is + - * /, sqrtf, fminf / fmaxf and comparisons in the order written here (dogeray_amd/csrc/device_denoise.hpp, no FMA contraction),
 * so the GPU is bit-identical to the host build of the same source and to the numpy restatement in the tests.
 *   grid       the pixel grid of dr_render_aov: gw x gh = (W / div / 8) * 8 x (H / div / 8) * 8; pixel p = (x, y)
 *   guides     normal n (3 f32), albedo a (3 f32), depth z, material m (-1: a miss) of p's pinhole ray (dr_render_aov's channels)
 *   colour     c = (float)acc / (float)divide_by per channel, acc the column-major accumulator at (x * H + y) * 3; while the accumulator
 *              has a history plane (dr_accum_reproject) c = (float)acc / (float)(hist_p + divide_by), and 0 where that divisor is 0
 *   demodulate e = c / a', a' = (m == -1 || a <= 1e-3f || !demodulate) ? 1 : a, per channel; l = (0.2126f e.r + 0.7152f e.g) + 0.0722f e.b
 *   q(x)       (1 + x) + (0.5 x) x; phi(x) = 1 / q(x) (phi(inf) = 0) is the rational stand-in for exp(-x)
 *   gz_p       fmaxf(gx, gy), gx = fminf(|z(x+1) - z_p|, |z_p - z(x-1)|), a neighbour outside the grid or a miss counting as +inf, an axis with
 *              no usable neighbour giving 0; gy likewise along y
 *   pair       g(p, q) = num / den for q = p + step (dx, dy), k = |dx| + |dy|:
 *                q outside the grid, exactly one of p, q a miss, or material_stop and m_p != m_q: no tap
 *                q = p, or both miss: 1 / 1
 *                otherwise num = wn = fmaxf((n_p.x n_q.x + n_p.y n_q.y) + n_p.z n_q.z, 0), squared normal_power_log2 times;
 *                den = q(xz), xz = dz > 0 ? dz * rz_k : 0, dz = |z_p - z_q|, rz_k = 1 / ((sigma_depth * gz_p) * (float)(step * k) + 1e-3f * z_p)
 *   variance   var_p = fmaxf(mu2 - mu1 * mu1, 0), mu1 = s1 / sw, mu2 = s2 / sw: over the 5x5 taps at step 1 inside the grid (dy = -2 .. 2
 *              outer, dx = -2 .. 2 inner) w = num / den, sw += w, s1 += w * l_q, s2 += w * (l_q * l_q)
 *   iteration  i = 0 .. iterations - 1, step = 2^i, l recomputed from the current e:
 *                gv_p = (sum kk var_q) / (sum kk) over the 3x3 taps at the same step that are not "no tap" above (dy outer, dx inner),
 *                       kk = k[dx] * k[dy], k = (1/4, 1/2, 1/4): the variance crosses no edge stop either, so pixels of one material (and
 *                       hit pixels against misses) are filtered independently of the others' colour, bit for bit
 *                rl = 1 / (sigma_luminance * sqrtf(gv_p) + 1e-4f)
 *                w = ((h[dx] * h[dy]) * num) / (den * q(|l_p - l_q| * rl)), h = (1/16, 1/4, 3/8, 1/4, 1/16), over the 5x5 taps as above
 *                e' = (sum w e_q) / sw per channel, var' = (sum (w * w) var_q) / (sw * sw); the centre's w is h[0]^2 > 0
 *   output     f = e * a' per channel: out_f32 row-major W x H x 3 in the accumulator's 0..255 units, unclamped; out_rgb8 =
 *              (uint8)(int)fminf(fmaxf(f, 0), 255) -- dr_accum_present's layout; pixels outside the grid are 0
 *   iterations 0: no filter and no demodulation, f = c: out_rgb8 is dr_accum_present(divide_by) byte for byte for divide_by < 65536 and
 *              |acc| < 2^24
 * By default the guides are pinhole rays through the pixel centres: with aperture > 0 the defocused parts of the image are then filtered against
 * sharp guides.  Option "guide_frames" = G > 0 takes them from dr_render_aov_lens over G frames instead, in its guide form: a pixel whose material
 * is -1 is a miss in every channel (n = 0, z = +inf, a = 0), and a = albedo + (1 - coverage) per channel -- a missed sample counts as albedo 1, so
 * demodulation leaves the sky's share alone; a' above then applies unchanged. */
typedef struct dr_denoise_params {
  int iterations;          /* 0 .. 10, default 5 */
  float sigma_luminance;   /* >= 0, default 4 */
  int normal_power_log2;   /* 0 .. 16, default 7 (wn^128, as SVGF) */
  float sigma_depth;       /* >= 0, default 1 */
  int demodulate;          /* default 1: filter c / albedo, then multiply the albedo back */
  int material_stop;       /* default 1: no weight between pixels of different materials */
} dr_denoise_params;
int dr_denoise_defaults(dr_denoise_params* p);
/* The denoised image of the accumulator (divided by divide_by) into out_f32 (W * H * 3 floats) and / or out_rgb8 (W * H * 3 bytes), either NULL
 * (not both).  params NULL: the defaults.  device_pointers = 0: host buffers, the call returns when they are filled; 1: device buffers on this
 * context's GPU, the work is queued on dr_context_stream.  The guides are computed by the AOV kernel into context-owned planes and kept for the
 * next call with the same settings13, W, H and scene (dr_context_upload_scene drops them); a context that never denoises allocates nothing for
 * it.  Ordered behind the frames submitted before it (dr_pipeline_submit); changes neither the accumulator, nor dr_stats, the stripe or any
 * option.  The settings are accepted or refused as by dr_render_aov; DR_ERR_INVALID for no scene, no accumulator, W / H not the accumulator's,
 * divide_by < 1, iterations outside 0 .. 10, a negative sigma, normal_power_log2 outside 0 .. 16, or no output. */
int dr_accum_denoise(dr_context* c, const float settings13[13], int W, int H, int divide_by, const dr_denoise_params* params, float* out_f32,
                     uint8_t* out_rgb8, int device_pointers);

/* ------------------------------------------------------------------ upsampler ----------- */
/* Shows an accumulator rendered at a fraction of the resolution (settings13[11] = div > 1, the reference's preview ladder K:2169-2199) at full
 * size.  DR_UPSCALE_BLOCK is the reference's display: every low pixel fills a div x div block (K:2281-2300).  DR_UPSCALE_GUIDED is a joint-
 * bilateral upsample (Kopf et al. 2007) of the demodulated low-resolution colour against the first-hit AOVs of the same view traced at full
 * resolution, with the denoiser's normal, depth and material stops; the full-resolution albedo is multiplied back, so geometric edges and
 * texture detail are sharp although the light is not.  Only + - * /, fminf / fmaxf and comparisons in the order written here
 * (dogeray_amd/csrc/device_upscale.hpp, no FMA contraction): the GPU is bit-identical to the host build of the same source and to the numpy
 * restatement in the tests.  q(x), a', gz and the pair terms wn, xz are the denoiser's, above.
 *   grids      div = (int)settings13[11] >= 1.  Low grid gw x gh: dr_render_aov's grid of settings13, low pixel q.  Output grid Gw x Gh =
 *              gw * div x gh * div, output pixel P = (X, Y); it lies inside the full-resolution AOV grid (W / 8) * 8 x (H / 8) * 8.  Output
 *              pixels outside Gw x Gh are 0; layout and units of out_f32 / out_rgb8 are dr_accum_denoise's
 *   low colour c_q = (float)acc / (float)divide_by per channel, with a history plane (float)acc / (float)(hist_q + divide_by), 0 where that
 *              divisor is 0 (the denoiser's colour)
 *   block      the output at P is low pixel (X / div, Y / div): out_f32 = c_q; out_rgb8 = clamp(acc / divisor, 0, 255) in integers, byte for
 *              byte what dr_accum_present writes for that pixel (div = 1: dr_accum_present's image).  No guides are traced and nothing is
 *              allocated beyond the staging of host outputs
 *   guides     full: N_P, Z_P, M_P, A_P = normal, depth, material, albedo of dr_render_aov for settings13 with element 11 set to 1.0f; gz_P
 *              the denoiser's depth gradient over P's four neighbours in the full grid; A'_P = a'(A_P, M_P).  Low: n_q, z_q, m_q, a_q the same
 *              channels for settings13 itself, a'_q; e_q = c_q / a'_q per channel.  Option "guide_frames" = G > 0: both sets are
 *              dr_render_aov_lens's guide form over G frames instead, as for dr_accum_denoise
 *   position   in integers: tx = 2 X + 1 - div, x0 = floor(tx / (2 div)) (-1 on the left edge), rx = tx - 2 div x0, fx = (float)rx /
 *              (float)(2 div); y0, fy likewise.  bx = (1.0f - fx, fx), by = (1.0f - fy, fy)
 *   taps       j = 0, 1 outer, i = 0, 1 inner, q = (x0 + i, y0 + j), b = bx_i * by_j.  No tap when q is outside the low grid, b == 0, exactly
 *              one of M_P, m_q is a miss, or material_stop and M_P != m_q.  Both miss: w = b.  Otherwise
 *              wn = fmaxf((N_P.x n_q.x + N_P.y n_q.y) + N_P.z n_q.z, 0) squared normal_power_log2 times, dz = |Z_P - z_q|,
 *              rz = 1 / ((sigma_depth * gz_P) * (float)div + 1e-3f * Z_P), xz = dz > 0 ? dz * rz : 0, w = (b * wn) / q(xz).
 *              sw += w, s += w * e_q per channel
 *   output     sw > 0: f = (s / sw) * A'_P per channel.  Otherwise (no usable tap: a thin object only the full-resolution guides see) f = c of
 *              low pixel (X / div, Y / div), the block value.  out_rgb8 = (uint8)(int)fminf(fmaxf(f, 0), 255)
 *   prefilter  non-NULL: dr_accum_denoise's a-trous filter runs on the low grid first, with these parameters, the options "denoise_variance" and
 *              "denoise_tiles" and the history plane as there; e_q is then the filter's e plane after its last iteration (what the denoiser's
 *              output stage would multiply by a'_q).  The block value of a pixel without a tap stays the unfiltered c */
enum { DR_UPSCALE_BLOCK = 0, DR_UPSCALE_GUIDED = 1 };
typedef struct dr_upscale_params {
  int mode;                /* default DR_UPSCALE_GUIDED */
  int normal_power_log2;   /* 0 .. 16, default 5 (wn^32: the taps are at most one low pixel away) */
  float sigma_depth;       /* >= 0, default 1 */
  int demodulate;          /* default 1: upsample c / albedo, then multiply the full-resolution albedo back */
  int material_stop;       /* default 1: no weight between pixels of different materials */
} dr_upscale_params;
int dr_upscale_defaults(dr_upscale_params* p);
/* The accumulator rendered with settings13 (divided by divide_by) at full size into out_f32 (W * H * 3 floats) and / or out_rgb8 (W * H * 3
 * bytes), either NULL (not both).  params NULL: the defaults; prefilter NULL: no filter.  device_pointers as dr_accum_denoise.  The low guides
 * are the denoiser's cached planes (a dr_accum_denoise and a dr_accum_upscale of the same settings13 share them); the full-resolution guides
 * live in context-owned planes of their own, allocated by the first guided call and keyed by (settings13 with element 11 = 1, W, H, scene), so
 * the stages of a preview ladder trace them once; dr_context_upload_scene drops both, a context that never upscales allocates nothing, and
 * option "upscale_aov_passes" reads how many AOV passes the last call traced.  Ordered behind the frames submitted before it
 * (dr_pipeline_submit); changes neither the accumulator, nor dr_stats, the stripe or any option.  The settings are accepted or refused as by
 * dr_render_aov; DR_ERR_INVALID for no scene, no accumulator, W / H not the accumulator's, divide_by < 1, a mode other than 0 / 1,
 * normal_power_log2 outside 0 .. 16, a negative sigma_depth, no output, and for a prefilter in block mode (call dr_accum_denoise), with
 * iterations < 1, with demodulate other than params' or with parameters dr_accum_denoise refuses. */
int dr_accum_upscale(dr_context* c, const float settings13[13], int W, int H, int divide_by, const dr_upscale_params* params,
                     const dr_denoise_params* prefilter, float* out_f32, uint8_t* out_rgb8, int device_pointers);

/* ------------------------------------------------------------------ temporal reprojection */
/* Carries the accumulator across a camera move: the temporal half of SVGF (Schied et al. 2017) as a nearest-neighbour BACKWARD reprojection.
 * The accumulated sums of the `from` view are moved to where the same surface points appear in the `to` view, and a per-pixel HISTORY PLANE
 * keeps how many samples each pixel carries.  All arithmetic is double on the float camera blocks (from, llc, hor, ver, den_w, den_h as
 * dr_render_frame forms them from settings13, K:1016-1068) and the float first-hit AOVs, only + - * /, sqrt, floor and comparisons in the
 * order written here (dogeray_amd/csrc/device_reproject.hpp, no FMA contraction), every dot product a . b = (a.x b.x + a.y b.y) + a.z b.z, so
 * the GPU is bit-identical to the host build of the same source and to the numpy restatement in the tests.
 *   grid       the pixel grid of dr_render_aov, gw x gh, the same for both views; p = (x, y) a pixel of the `to` view
 *   guides     t, shading normal n, material m (-1: a miss) of both views' pinhole rays (dr_render_aov's channels)
 *   d(view, x, y)   the float pinhole direction of dr_render_aov: nu = (float)(((double)x + 0.5) / den_w), nv likewise with y and den_h,
 *              d = ((llc + nu * hor) + nv * ver) - from per component in float; then widened to double
 *   masked     m_p is not allowed: a miss when sky == 0; a hit when bit b of material_mask is clear, b = m_p for 0 <= m_p <= 30, else 31
 *   world point  d_p = d(to, x, y).  A hit: X = from_to + (double)t_p * d_p per component, v = X - from_from.  A miss: v = d_p (the sky is at
 *              infinity)
 *   projection (once per call) L = llc_from - from_from; cN = hor_from x ver_from = (hor.y ver.z - hor.z ver.y, hor.z ver.x - hor.x ver.z,
 *              hor.x ver.y - hor.y ver.x), negated when cN . L < 0; L . cN zero or not finite: DR_ERR_INVALID (a degenerate view).
 *              (per pixel) a = v . cN; !(a > 0): offscreen.  s = (L . cN) / a; r = s * v - L per component; nu = (r . hor) / (hor . hor),
 *              nv = (r . ver) / (ver . ver); fx = floor(nu * den_w), fy = floor(nv * den_h); unless 0 <= fx < gw and 0 <= fy < gh: offscreen;
 *              q = (fx, fy).  Pixel centres sit at (x + 0.5) / den_w, so an unchanged view maps every pixel to itself.
 *   validation m_q != m_p: rejected.  Both miss: valid.  Hits: n_p . n_q < normal_cos (or unordered): rejected; d_q = d(from, q),
 *              e = X - (from_from + (double)t_q * d_q) per component, |e . n_p| <= plane_tolerance * sqrt(v . v) or rejected (the plane
 *              distance of SVGF).  There is no object-id test: an object is one triangle, and triangles may be pixel-sized.
 *   carry      valid: cnt = hist_from[q] + frames (hist_from = 0 without a plane).  cnt <= max_history: acc_to[p] = acc_from[q] and
 *              hist_to[p] = cnt; otherwise acc_to[p] = (int32)(((int64)acc_from[q] * max_history) / cnt) per channel (division towards
 *              zero) and hist_to[p] = max_history.  Every other pixel, and every pixel outside the grid: acc_to = 0, hist_to = 0.
 * The classes are tested in the order masked, offscreen, rejected, valid; dr_reproject_result counts the grid's pixels in each. */
typedef struct dr_reproject_params {
  int max_history;         /* 1 .. 65535, default 32: most samples a pixel carries over */
  float normal_cos;        /* -1 .. 1, default 0.9 */
  float plane_tolerance;   /* >= 0, default 0.01: in units of the distance from the `from` camera */
  uint32_t material_mask;  /* default 0xFFFFFFC3: diffuse 0, emissive 1 and every id from 6 on are carried; mirror 2, metal 3, glass 4 and
                              glossy 5 are view-dependent and start again */
  int sky;                 /* default 1: misses are carried */
} dr_reproject_params;
typedef struct dr_reproject_result {
  int64_t pixels;          /* gw * gh = valid + masked + offscreen + rejected */
  int64_t valid, masked, offscreen, rejected;
} dr_reproject_result;
int dr_reproject_defaults(dr_reproject_params* p);
/* frames >= 1: the frames added to the accumulator since the last dr_accum_reset or dr_accum_reproject (the caller's divide_by).  params
 * NULL: the defaults; result may be NULL.  The context owns two accumulator / history pairs; the call reads the current pair, writes the other
 * and makes it the current one: afterwards accumulator and history plane belong to the `to` view and the caller's frame count starts again at
 * 0.  While a plane exists, dr_accum_present, dr_accum_denoise and dr_pipeline_submit's presents divide pixel p by hist[p] + divide_by;
 * dr_accum_reset drops the plane, and a context that never reprojects allocates nothing for it.  The guides of the `to` view are kept and keyed
 * like the denoiser's (settings13, W, H, scene; dr_context_upload_scene drops them): a later call whose `from` is that view traces one AOV
 * pass instead of two (option "reproject_aov_passes").  Ordered behind the frames submitted before it (dr_pipeline_submit); returns when the
 * counts are known; changes neither dr_stats nor any option.  Both settings are accepted or refused as by dr_render_aov; DR_ERR_INVALID for no
 * scene, no accumulator, W / H not the accumulator's, frames < 1, views with different divisors, a stripe other than (1, 0), a degenerate
 * `from` view, or parameters outside their ranges.  The guides are pinhole rays whatever option "guide_frames" says: what is
 * reprojected is a position, and the lens-averaged channels (dr_render_aov_lens) are no position. */
int dr_accum_reproject(dr_context* c, const float from_settings13[13], const float to_settings13[13], int W, int H, int frames,
                       const dr_reproject_params* params, dr_reproject_result* result);

/* ------------------------------------------------------------------ second moments ------ */
/* How noisy is this pixel, and when can the render stop: a per-pixel SECOND-MOMENT PLANE beside the accumulator -- the "variance estimate carried
 * along with the sums" of SVGF (Schied et al. 2017) -- and the noise estimate formed from it.  Option "moments" = 1 before dr_accum_reset gives the
 * accumulator the plane; all integer arithmetic below is exact, the estimate is double with only + - * /, sqrt, floor and comparisons in the order
 * written here (dogeray_amd/csrc/device_moments.hpp, no FMA contraction), so the GPU is bit-identical to the host build of the same source and to
 * the numpy restatement in the tests.
 *   plane      M2: one uint64 per pixel, pixel (x, y) at x * H + y like the history plane
 *   add        for every frame folded into the accumulator, with that frame's int32 values (r, g, b) at the pixel:
 *                y  = (54 r + 183 g) + 19 b in int64: Rec.709 luma x 256 (the weights sum to 256), |y| < 2^39
 *                yc = min(max(y, -2^26), 2^26): the firefly cap, 1028 x a white pixel's 65280; yc^2 <= 2^52
 *                M2 = M2 + (uint64)(yc * yc), saturating at 2^64 - 1
 *              dr_pipeline_submit and dr_render_accumulate_pipelined fold each frame with ONE kernel, acc += frame and M2 += yc^2;
 *              dr_render_accumulate runs as dr_render_accumulate_pipelined; dr_render_accumulate_async returns DR_ERR_INVALID ("moments")
 *   first moment  not stored: S1 = (54 accR + 183 accG) + 19 accB in int64 equals the sum of y exactly, because y is linear -- as long as no
 *              frame was capped (a capped frame enters M2 with yc and S1 with y)
 *   reproject  dr_accum_reproject carries the plane (a second buffer appears with the first reprojection, as for the history): a valid pixel with
 *              cnt <= max_history takes M2_to[p] = M2_from[q]; with cnt > max_history M2_to[p] = (M2 / cnt) * max_history + ((M2 % cnt) *
 *              max_history) / cnt, which is floor(M2 * max_history / cnt) exactly; every other pixel 0.  Sums and squares scaled by the same
 *              factor leave M2 / n - (S1 / n)^2 unchanged
 *   estimate   n = hist_p + divide_by (hist_p = 0 without a history plane; divide_by >= 0: a reprojected image with no new frame has 0).  n < 2:
 *              not estimated, sigma_p = 0.  Otherwise, all in double:
 *                S1d = (double)S1; M2d = (double)M2
 *                ss = M2d - (S1d * S1d) / (double)n; ss = ss > 0 ? ss : 0
 *                var_p = (ss / ((double)(n - 1) * (double)n)) / 65536.0: the variance of the displayed mean luma, in (0..255 units)^2
 *                sigma_p = (float)sqrt(var_p)
 *              pixels outside the pixel grid: sigma = 0
 *   denoiser   option "denoise_variance" = 1 and a plane: dr_accum_denoise's variance of a pixel with n_p >= 4 is var = (float)(var_p / ((double)la *
 *              (double)la)), la = (0.2126f a'.r + 0.7152f a'.g) + 0.0722f a'.b with a' the albedo the demodulation uses; la == 0 or n_p < 4: the
 *              spatial estimate.  An approximation: the moments are of the luma before demodulation.  It feeds the luminance edge stop only. */
typedef struct dr_error_result {
  int64_t pixels;        /* gw * gh, the pixel grid of settings13 (dr_render_aov's) */
  int64_t estimated;     /* pixels with n_p >= 2 */
  int64_t above;         /* estimated pixels with sigma_p > tolerance */
  uint64_t sum_var_q16;  /* sum over estimated pixels of min(floor(var_p * 65536), 2^40) */
  int64_t bins[16];      /* estimated pixels by sigma_p: bin 0 < 2^-6; bin k: 2^(k-7) <= sigma < 2^(k-6), k = 1..14; bin 15 >= 2^8 */
} dr_error_result;
/* The noise estimate of the accumulator: sigma_p of every pixel into out_sigma (W * H floats, row-major, dr_accum_present's layout; may be NULL) and /
 * or the counts into result (may be NULL, not both).  Every field of the result is an integer count or a fixed-point sum: the same bits whatever
 * order the GPU adds them in.  device_pointers = 1 applies to out_sigma only (a device buffer on this context's GPU, written on
 * dr_context_stream); the result is host memory and the call returns when it is known.  Ordered behind the frames submitted before it
 * (dr_pipeline_submit); changes neither the accumulator, nor dr_stats or any option.  The settings are accepted or refused as by dr_render_aov;
 * DR_ERR_INVALID for no scene, no accumulator, W / H not the accumulator's, no moments plane, divide_by < 0, a negative or NaN tolerance, or no output. */
int dr_accum_error(dr_context* c, const float settings13[13], int W, int H, int divide_by, float tolerance, float* out_sigma, dr_error_result* result,
                   int device_pointers);
/* The second-moment plane, uint64 per pixel at x * H + y.  Without a plane dr_accum_moments_read writes zeros and dr_accum_moments_device_ptr gives
 * NULL / 0 bytes; dr_accum_reproject swaps between two buffers, the pointer is the current one. */
int dr_accum_moments_read(dr_context* c, uint64_t* out /* W*H */);
int dr_accum_moments_device_ptr(dr_context* c, void** dev_ptr, uint64_t* bytes);

/* ------------------------------------------------------------------ adaptive sampling ---- */
/* Acting on the noise estimate: one call is one PASS, which adds nframes frames to the 8x8 tiles whose pixels still ask for samples and to no other
 * pixel.  The render kernels are the ones every other call launches, over a shorter tile order.  All arithmetic is the second
 * moments' above, so the GPU is bit-identical to the host build of the same source (dogeray_amd/csrc/device_adaptive.hpp) and to the numpy
 * restatement in the tests.
 *   selection  made from the planes as they are when the call is reached in stream order, behind the frames submitted before it.  For grid pixel p,
 *              n = hist_p + divide_by (hist_p = 0 without a history plane; a "sample" is a frame, as everywhere else).  The pixel ASKS when
 *                n < min_samples, or
 *                (max_samples == 0 or n < max_samples) and n >= 2 and sigma_p > tolerance -- var_p, sigma_p and the float comparison exactly as
 *                dr_accum_error forms dr_error_result.above
 *              The view's pixel grid is cut into the render kernels' tiles: tile t = col * gy + by (gy = H / div / 8 tile rows, col the block
 *              column), its lane l the pixel (8 col + (l >> 3), 8 by + (l & 7)).  A tile is ACTIVE when at least tile_pixels of its 64 pixels ask
 *   render     frames k = 0 .. nframes - 1 with seeds frame_seed + k * seed_stride are rendered in the active tiles only; F_k below is, bit for bit,
 *              what dr_render_frame returns for that seed
 *   fold       for every pixel of an active tile, and every k: acc += F_k (wrapping) and M2 = M2 + yc(F_k)^2 (saturating: the add above); then
 *              hist += nframes.  Every other pixel of the three planes keeps its bits.  Without a history plane one of zeros is made first (it stays
 *              until dr_accum_reset, and dr_accum_present and the other stages divide by it from then on: pass the count of the uniform frames)
 *   limits     choosing where to sample from the samples' own variance is not exactly unbiased: a pixel whose first samples happen to agree stops
 *              early.  min_samples and the tile granularity (a tile is rendered whole) are the guard; nothing stronger is claimed
 * dr_stats.samples grows by the samples really traced and dr_stats.launches by the launches; dr_stats.frames does not change. */
typedef struct dr_adaptive_params {
  float tolerance;       /* >= 0, not NaN: the sigma_p a pixel may keep (0..255 units) */
  int min_samples;       /* >= 2 (default 4): pixels with fewer samples ask whatever their estimate says */
  int max_samples;       /* 0: no limit (default); otherwise > min_samples: pixels with that many samples do not ask */
  int tile_pixels;       /* 1 .. 64 (default 1): asking pixels that make a tile active */
} dr_adaptive_params;
typedef struct dr_adaptive_result {
  int64_t tiles;         /* gx * gy, the tiles of the pixel grid of settings13 */
  int64_t active_tiles;
  int64_t pixels;        /* 64 * tiles */
  int64_t asking_pixels;
  int64_t samples_added; /* active_tiles * 64 * nframes */
} dr_adaptive_result;
int dr_adaptive_defaults(dr_adaptive_params* p);      /* tolerance 1.0 */
/* One pass (params NULL: the defaults; result may be NULL).  Returns when the pass has been folded.  DR_ERR_INVALID, and no plane touched, for: no
 * scene, no accumulator or W / H not the accumulator's, no moments plane, a stripe other than (1, 0), the tile-per-launch kernel or the ordered
 * traversal (the pass needs the persistent kernel's queues), nframes < 1, divide_by < 0, parameters outside their ranges; settings13 as dr_render_frame. */
int dr_render_adaptive(dr_context* c, const float settings13[13], int W, int H, float background, uint64_t frame_seed, uint64_t seed_stride, int nframes,
                       int divide_by, const dr_adaptive_params* params, dr_adaptive_result* result);

/* ------------------------------------------------------------------ multi-GPU group ----- */
/* One process, one context and one host thread per GPU (the reference is single-device, K:2614-2615).  Rank r of n
 * renders the block columns bx % n == r of every frame (scene replicated); every `gather_every` frames each rank packs
 * its stripe and sends it to rank 0 over RCCL (ncclSend / grouped ncclRecv on a second stream per rank), double-
 * buffered so that the gather of one batch runs beside the rendering of the next.  After the call rank 0's accumulator
 * (dr_group_context(g, 0): dr_accum_read / dr_accum_present) holds the assembled sum of all frames.
 * device_ordinals NULL = 0 .. n-1.  Ranks that share a device, or DOGERAY_GROUP_TRANSPORT=copy, use peer copies. */
typedef struct dr_group dr_group;
int dr_group_create(int n, const int* device_ordinals, dr_group** out);
void dr_group_destroy(dr_group* g);
int dr_group_size(const dr_group* g);
int dr_group_uses_rccl(const dr_group* g);
int dr_group_rccl_ranks(const dr_group* g);   /* ranks of the RCCL communicator (ncclCommCount), 0 when the copy transport is used */
dr_context* dr_group_context(dr_group* g, int rank);
int dr_group_upload_scene(dr_group* g, const dr_scene* s);
int dr_group_accum_reset(dr_group* g, int W, int H);
int dr_group_render_accumulate(dr_group* g, const float settings13[13], int W, int H, float background,
                               uint64_t frame_seed, uint64_t seed_stride, int nframes, int gather_every);

/* Counters and timings since the last dr_stats_reset.  Ray = one hit() call (K:800). */
typedef struct dr_stats {
  uint64_t frames;        /* frames rendered                                            */
  uint64_t launches;      /* render kernel launches (one launch may cover a batch of frames) */
  uint64_t samples;       /* primary samples                                            */
  uint64_t rays;          /* closest-hit queries (counted only when counters are on)    */
  uint64_t node_visits;   /* V: AABB tests performed by the kernel's traversal          */
  uint64_t prim_tests;    /* L                                                          */
  uint64_t shades;        /* S: hits shaded                                             */
  uint64_t texels;        /* T                                                          */
  double kernel_ms;       /* sum of HIP-event durations of the render kernel launches   */
  uint64_t trav_slots;    /* 64 x wave-level traversal iterations: node_visits / trav_slots = SIMD efficiency of the node loop */
  uint64_t ray_slots;     /* 64 x wave-level closest-hit calls:    rays / ray_slots = SIMD efficiency of the bounce loop       */
  uint64_t diag[8];       /* counting build of the persistent kernel: wave cycles, cycles in the shade phase, loop iterations, shade phases,
                             wave-level node steps, wave-level leaf steps (wide walk), lanes shaded, wave lifetime in 100 MHz ticks */
} dr_stats;
int dr_stats_enable_counters(dr_context* c, int on); /* counting build of the kernel; off by default */
int dr_stats_reset(dr_context* c);
int dr_stats_get(dr_context* c, dr_stats* out);

/* Counting build of the persistent kernel (dr_stats_enable_counters): the shade / refill phase's budget since dr_stats_reset, n <= 32 words:
 * [0..15] histogram of the turns a wave's rejection loop ran in a phase (bin 15: 15 or more; bin 0: nobody drew), [16] candidates drawn by all lanes,
 * [17] turns summed over phases, [18] lanes that drew a point in the unit sphere (scatter, K:640-648), [19] lanes that drew a point in the unit disk
 * (new path, K:988-994), [20] retired lanes summed over phases.  With dr_stats.diag (phases, lanes shaded, cycles in phases) this prices the phase. */
int dr_stats_phase_counts(dr_context* c, unsigned long long* out, int n);

/* The tile mask of the camera rays' grazing certificate of the last certified view (option camera_cert): one bit per tile of
 * that launch (bit t of word t / 32; tile = local block column * tile rows + row), set = the tile's camera rays keep the scene's margin.
 * *n_tiles = 0 when no certificate is in use; otherwise the tiles, and the first min(max_words, (n_tiles + 31) / 32) words are copied to out. */
int dr_stats_cert_mask(dr_context* c, uint32_t* out, int max_words, int* n_tiles);
/* The grades of the same view's tiles (option cert_levels): one byte per tile, tile = local block column * tile rows + row.  0: the tile's camera rays
 * keep the scene's margin; g >= 1: the tile passes the ladder's steps 0 .. g - 1 and its camera rays carry the margin of step g - 1 (with cert_levels
 * = 1 the steps are cert_factor x {1/4, 1/2, 1, 2, 4}, grades 0 .. 5, and the tile's bit in dr_stats_cert_mask is set exactly when its grade is below
 * 3; with cert_levels = 0 the one step is cert_factor, grades 0 and 1).  *n_tiles = 0 when no certificate is in use; otherwise the tiles, and the
 * first min(max, n_tiles) bytes are copied to out_bytes. */
int dr_stats_cert_levels(dr_context* c, uint8_t* out_bytes, int max, int* n_tiles);
/* The entry codes of the same view's tiles (option camera_entry): one int32 per tile, tile = local block column * tile rows + row.  A code is wide
 * record << 1 | is-leaf: the record at which the tile's camera rays start their walk; 0 the root (every tile with camera_entry = 0), -1 no leaf of the
 * scene can be seen from the tile.  *n_tiles = 0 when no table is in use; otherwise the tiles, and the first min(max, n_tiles) codes are
 * copied to out. */
int dr_stats_camera_entry(dr_context* c, int32_t* out, int max, int* n_tiles);
/* The last launch's split (option sky_tiles): *n_sky = the tiles rendered by the sky kernel (entry code -1), *n_geometry = the tiles left to the
 * persistent kernel; both 0 when the launch was not split. */
int dr_stats_sky_tiles(dr_context* c, int* n_sky, int* n_geometry);
/* The last adaptive pass's tiles (dr_render_adaptive): one byte per tile, tile = block column * tile rows + row, 1 = active (rendered), 0 = left alone.
 * *n_tiles = 0 when no pass has run since the context was made; otherwise the tiles, and the first min(max, n_tiles) bytes are copied to out. */
int dr_stats_adaptive_tiles(dr_context* c, uint8_t* out, int max, int* n_tiles);

/* Timeline of the last SHORT persistent-kernel launch (fewer than coop_tiles_per_wave tiles per wave: one frame, a thin stripe;
 * option "wave_log" = 1 before the launch): sixteen words per wave --
 * begin, first time the wave found the work queue empty (0: never), end, all in 100 MHz ticks of the GPU's
 * real-time counter, and the loop iterations the wave ran after the queue was empty (words 4..15: zero).  Shows where a launch's
 * tail goes (a single frame per launch, K:2154-2224, is mostly tail).  out: 16 * max_waves words. */
int dr_stats_wave_log(dr_context* c, unsigned long long* out, int max_waves, int* n_waves);
/* Node steps each pixel of the last frame cost (the persistent kernel's feedback for its tile order, option
 * "feedback"): pixel (tile, lane) at tile * 64 + lane, tile = block column * gy + block row over the frame's whole tiles
 * (gx = W / div / 8 block columns of gy = H / div / 8 tiles, div = the preview divisor settings13[11]), lane = (x & 7) * 8 + (y & 7).
 * *n = words written: min(capacity, 64 * the tiles the buffer has room for, which is at least gx * gy); 0: no feedback recorded yet. */
int dr_stats_pixel_cost(dr_context* c, unsigned* out, size_t capacity, size_t* n);
/* The tile order the next persistent launch of the same view would use (test and measurement aid; waits for the context's stream):
 * args[5] = the arguments of the last feedback pass the context enqueued -- tiles, regions (1 or 8), heavy_factor, split_steps, split_limit;
 * *n = tiles (0: no order is valid, nothing else is written); the first min(capacity, tiles) entries of the order go to order (may be NULL
 * with capacity 0); region_start[17]: [r], r <= regions, the first position of region r in the order; [9 + r], r < regions, how many tiles
 * at the head of region r's part a one-frame launch hands out in split_parts parts.  The other words are not read by the kernel.
 * DESIGN.md 4.3 "the order's contract" says what the order is. */
int dr_stats_tile_order(dr_context* c, int* order, size_t capacity, size_t* n, int* region_start, int* args);
/* Measurement aid (bench.py `roofline.gather`): rate at which this GPU serves divergent, dependent fetches of 64-byte
 * records from the RESIDENT wide-walk array -- the walk's memory behaviour without its arithmetic.  hot_records
 * restricts the random walk to the first records of the array (0 = all of it). */
int dr_context_probe_gather(dr_context* c, uint32_t hot_records, int iters, double* records_per_s);

/* Measurement aid (tools/moments_rate.py): the two kernels that fold a frame into the accumulator, timed alone with HIP events -- `iters` launches of
 * the plain add (acc += frame) into plain_ms[iters], then `iters` of the fused add of the second-moment plane (acc += frame, M2 += yc^2) into
 * fused_ms[iters] (zeros without a plane).  The frame added is black, so neither the sums nor the plane change. */
int dr_context_probe_frame_add(dr_context* c, int iters, double* plain_ms, double* fused_ms);

/* Measurement aid (tools/exp_trace_rate.py): what the walk would cost as a kernel of its own.  Renders ONE frame with the counting build, which writes every ray
 * it traces into the order a per-bounce wavefront would hold them (bounce by bounce, pixels in tile order); then a TRACE-ONLY kernel walks `frames` copies of that
 * list -- variant 0: one ray per lane, a wave waits for its slowest; 1..7: persistent waves whose lanes refill from the ray list in a few instructions, 128 rays per
 * wave and atomic (occupancy / free lanes before a refill / lanes at a leaf before a leaf step: 6/1/20, 6/8/20, 6/16/20, 8/8/20, 8/8/28, 6/8/28, 8/4/32) -- and is
 * timed (best of three).  *n_rays = rays of the frame; *mismatches = results that differ from the one-ray-per-lane walk (t bits or slot). */
int dr_context_probe_trace(dr_context* c, const float settings13[13], int W, int H, float background, uint64_t frame_seed, int frames, int variant,
                           double* rays_per_s, uint64_t* n_rays, uint64_t* mismatches);
/* Measurement aid: the rays that probe walks -- one frame's rays in wavefront order (bounce by bounce, pixels in tile order), as the counting build logs
 * them -- for a caller who wants to send them through dr_trace_rays (tools/trace_rate.py).  origin / dir: room for `capacity` rays of 3 floats each;
 * *n_rays: the rays of the frame (call with capacity 0 to size the buffers).  Resets the accumulator to W x H, as the probe does. */
int dr_context_probe_rays(dr_context* c, const float settings13[13], int W, int H, float background, uint64_t frame_seed, float* origin, float* dir,
                          uint64_t capacity, uint64_t* n_rays);

/* ------------------------------------------------------------------ known-answer hooks -- */
/* Run single device functions on caller data (host pointers), for parity tests.  The contract of every hook: n items in, n items out, one item per
 * GPU lane; arrays hold n (or the stated multiple of n) elements.  A null context or n < 0 is DR_ERR_INVALID; n == 0 is DR_OK and touches no
 * pointer; otherwise a null pointer is DR_ERR_INVALID ("null argument") -- only dr_kat_hit's visits may be null -- and a hook that reads the resident
 * scene without one is DR_ERR_INVALID ("no scene uploaded").  Values are judged next (each hook says which), and nothing reaches the device before
 * every check has passed.  The call is ordered behind the frames submitted before it (dr_pipeline_submit), runs on the context's stream and returns
 * after the results are in the caller's arrays; a launch error is DR_ERR_DEVICE.  (dr_kat_tile_feedback and dr_kat_order_split count tiles: their
 * refusals of a count come first, and they have no empty call; dr_kat_order_split's order may be null.) */
int dr_kat_rng(dr_context* c, uint64_t seed, int n, double* out);
int dr_kat_aabb(dr_context* c, int n, const float* o, const float* d, const float* mn, const float* mx,
                int32_t* hit, float* dist);
int dr_kat_tri(dr_context* c, int n, const float* o, const float* d, const float* v0, const float* v1,
               const float* v2, float* t);
int dr_kat_sphere(dr_context* c, int n, const float* o, const float* d, const float* centre,
                  const float* radius, float* t);
int dr_kat_optics(dr_context* c, int n, const float* v, const float* nrm, const float* eta, float* refl,
                  float* refr, float* schlick);
/* getnormal K:703-773 for object `object_index[i]` (index in the .rts file) of the resident scene, ray (o, d), hit at t:
 * the normalised, not yet flipped normal and the interpolated texture coordinate (z = 0), 3 floats each */
int dr_kat_normal(dr_context* c, int n, const int32_t* object_index, const float* o, const float* d, const float* t,
                  float* normal, float* texco);
/* The shading step, function by function (device_rng.hpp, device_surface.hpp, device_shade.hpp), one element per GPU lane.  Where the render kernels
 * have two forms of a step, a hook runs BOTH on copies of the same generator state and returns both: the results of form 0 (the plain functions) for
 * the n elements, then those of form 1 (what the persistent kernel runs).  A generator is Xorwow::init(seed[i]) followed by warm[i] (0 .. 4096) calls
 * of next(); `next` holds the two outputs that follow what the step drew, which proves how many draws it consumed.
 *
 * dr_kat_sample: kind[i] 3 = a point in the unit sphere, 2 = in the unit disk, 0 = nothing (point 0).  point_plain / next_plain: rand_in_unit_sphere /
 * rand_in_unit_disk; point_merged / next_merged: rand_points_merged with the lane's kind -- the 64 lanes of a wave run ONE loop, so the order of the
 * elements decides which kinds share a loop.  Points 3 floats, next 2 words per element. */
int dr_kat_sample(dr_context* c, int n, const uint64_t* seed, const int32_t* warm, const int32_t* kind, float* point_plain,
                  uint32_t* next_plain, float* point_merged, uint32_t* next_merged);
/* outside_unit on a squared length: out[i] = 1 where the rejection loops reject */
int dr_kat_outside(dr_context* c, int n, const float* d2, int32_t* out);
/* tex_fetch of texture tex[i] of the resident scene at (u[i], v[i]): the texel word r | g << 8 | b << 16 */
int dr_kat_tex(dr_context* c, int n, const int32_t* tex, const float* u, const float* v, uint32_t* rgba);
/* One bounce of the ray (o, d) with attenuation atten on object object_index[i] (index in the .rts file) of the resident scene at a GIVEN distance t[i]
 * -- no traversal, as dr_kat_normal.  Form 0: shade_hit; form 1: shade_prepare, the point of rand_points_merged (kind 3 for the materials that draw
 * one, else 0), shade_scatter.  Per form and element: alive (1: the path continues; 0: it ended at an emissive surface or an unknown material -- the
 * ray is returned as it came and atten_out holds the radiance), the ray and attenuation afterwards, next.  alive[2 n], o_out / d_out / atten_out
 * [2 n * 3], next[2 n * 2]. */
int dr_kat_bounce(dr_context* c, int n, const int32_t* object_index, const float* o, const float* d, const float* t, const float* atten,
                  const uint64_t* seed, const int32_t* warm, int32_t* alive, float* o_out, float* d_out, float* atten_out, uint32_t* next);
/* shade_miss: the background of a ray of direction d and attenuation atten that hit nothing (backtex: a texture of the resident scene, -1 = the sky
 * gradient; background: its intensity): rgb[n * 3] */
int dr_kat_miss(dr_context* c, int n, const float* d, const float* atten, int backtex, float background, float* rgb);
/* The camera ray of sample sample[i] of pixel (x[i], y[i]) of the view (settings13, W, H) as a render launch fills it, the generator seeded with
 * sample_seed for frame_seed -- frame_seed + sample * 0x9E3779B97F4A7C15 + (uint32)(x + y * seed_stride); a launch's seed_stride is 8 * its block
 * columns.  Form 0: camera_ray; form 1: camera_prepare, the point of rand_points_merged (kind 2), camera_finish.  origin / dir [2 n * 3],
 * next[2 n * 2].  Needs an uploaded scene, as every render launch. */
int dr_kat_camera(dr_context* c, const float settings13[13], int W, int H, uint64_t frame_seed, uint32_t seed_stride, int n, const int32_t* x,
                  const int32_t* y, const int32_t* sample, float* origin, float* dir, uint32_t* next);
/* store_pixel (not accumulating) of a pixel's summed colour for spp samples: out[n * 3] */
int dr_kat_store(dr_context* c, int n, const float* color, int spp, int32_t* out);
/* The stores of a batched launch (device_shade.hpp), on lanes the caller chooses: lane i of the call is lane i % 64 of wave i / 64, four waves to a
 * workgroup as in the render kernel, all 64 lanes of a wave active at the store.  The lanes with store_me[i] != 0 add colour i (summed over spp
 * samples, store_pixel's conversion) to pixel (x[i], y[i]) of acc, a W x H accumulator in store_pixel's layout, (x * H + y) * 3, read and written
 * back; key[i] names the lane's pixel to the merge (the render kernel passes the pixel's code).  form 0: store_pixel, every storing lane adding
 * atomically on its own; 1: store_pixels_merged (a DPP sum per distinct key); 2: store_pixels_merged_lds (the default build's).  Integer addition is
 * exact in any grouping, so the three forms must return the same acc: the sum of the storing lanes' integers per pixel, wrapped to 32 bits.
 * Every wave owns 7 rows of 64 LDS words, copied from lds_in before the store and to lds_out after it ((n_lanes / 64) * 7 * 64 words each, wave-major):
 * rows 1 .. 5 are the five slot rows of form 2 -- word w of slot s of the wave at row 1 + w, column s --, rows 0 and 6 are guards; forms 0 and 1
 * leave all seven as they came, form 2 writes only the slots key & 63 of storing lanes.
 * The kernel does not test where it adds: DR_ERR_INVALID, before anything is staged, for form outside 0 .. 2, n_lanes no multiple of 64, spp < 1,
 * W or H < 1, and for a lane with store_me that has x outside [0, W), y outside [0, H), a negative key, or the key of a storing lane of another
 * pixel (the merge's precondition: one key, one pixel; two keys for one pixel are allowed).  There is no host mirror: LDS atomics and DPP have none. */
int dr_kat_store_merged(dr_context* c, int form, int n_lanes, const int32_t* store_me, const int32_t* key, const int32_t* x, const int32_t* y,
                        const float* color, int spp, int W, int H, int32_t* acc, const int32_t* lds_in, int32_t* lds_out);
/* The plane arithmetic of the wide walk's node test (device_wide.hpp wide_node_test): for word w[i] (four plane bytes) t_mix[4 i + k] =
 * fma(byte_k read as the f16 denormal byte * 2^-24 inside v_fma_mix_f32, a[i] * 2^24, b[i]) and t_cvt[4 i + k] = fma((float)byte_k, a[i], b[i]):
 * the two must agree bit for bit (a[i] * 2^24 must not overflow) -- the check that the instruction keeps f16 denormals */
int dr_kat_node_planes(dr_context* c, int n, const uint32_t* w, const float* a, const float* b, float* t_mix, float* t_cvt);
/* closest hit against the resident scene: t (-1 = miss), ORIGINAL object index and (visits may be NULL)
 * the number of boxes the chosen traversal tested for that ray */
int dr_kat_hit(dr_context* c, int n, const float* o, const float* d, float* t, int32_t* idx, int32_t* visits);
/* dr_kat_hit's rays through the LEAN build of the wide walk, the one render launches time and ship (dr_kat_hit runs the counting build): the trace-only
 * kernels of dr_context_probe_trace on caller rays -- variant 0: one ray per lane (the primitive-first leaf step behind a wave ballot); 1..7: persistent
 * waves refilling from the ray list, planes selected by sign masks, exclusive node / leaf steps (the parameter sets listed at dr_context_probe_trace).
 * Results in dr_kat_hit's convention: t (-1 = miss) and the ORIGINAL object index (0 on a miss).  Needs a resident wide tree (DR_ERR_INVALID for a scene
 * that has none, whatever the traversal option says); it does not need the persistent-kernel option.  The results are preset to a pattern no walk
 * returns, and a ray the kernel left unanswered -- anything but a hit or {10000, -1} -- is DR_ERR_DEVICE naming the ray, never a miss. */
int dr_kat_trace(dr_context* c, int variant, int n, const float* o, const float* d, float* t, int32_t* idx);
/* The two feedback kernels behind the persistent kernel's tile order, on caller data and scratch buffers (the context's own order is not
 * touched): pixel_cost[ntiles * 64] -> tile_cost[ntiles] (the maximum of each tile's 64 words), order[ntiles] and region_start[17] as
 * dr_stats_tile_order describes them.  order and region_start are filled with -1 before the launch: an entry the kernels did not write
 * stays -1.  The sum of the tile costs times heavy_factor must stay below 2^64.  DR_ERR_INVALID for what no render launch asks for:
 * ntiles < 1, regions other than 1 or 8, 8 regions of fewer than 512 tiles, split_limit < 0. */
int dr_kat_tile_feedback(dr_context* c, int ntiles, int regions, int heavy_factor, int split_steps, int split_limit,
                         const unsigned* pixel_cost, unsigned* tile_cost, int* order, int* region_start);
/* The one-workgroup kernel that splits a launch's tile order, on caller data and scratch buffers (no cache of the context is touched): the stable
 * partition of order[ntiles] (NULL: the identity) with region_start[regions + 1] -- region r owns positions [region_start[r], region_start[r + 1]) --
 * by a key per tile.  kind 0: key = uint32_t[ntiles], the tiles' words; a tile whose entry code is "sees no leaf" is dropped (the sky tiles of option
 * sky_tiles), and the dropped tiles are listed.  kind 1: key = uint8_t[ntiles], a tile is kept when its byte is not 0 (dr_render_adaptive's flags);
 * nothing is listed.  Out: launch_order[ntiles], the kept tiles in the order they had, in its first `kept` entries; launch_region_start[17], [r] the
 * compacted start of region r, [regions] = kept, every later entry 0; kind 0 only: dropped_list[ntiles], the dropped tiles in ascending tile number
 * in its first `dropped` entries, and counts[2] = {dropped, kept}.  All four outputs are filled with 0xff bytes before the launch: an entry the kernel
 * did not write -- the tails of the two lists, and for kind 1 all of dropped_list and counts -- reads as -1.  The kernel trusts its inputs, so
 * DR_ERR_INVALID, before anything is staged, for kind other than 0 or 1, ntiles < 1, regions outside 1 .. 8, a region_start that is not
 * non-decreasing from 0 to ntiles over [0 .. regions], and an order that is not a permutation of 0 .. ntiles - 1. */
int dr_kat_order_split(dr_context* c, int kind, int ntiles, int regions, const int* order_or_null, const int* region_start, const void* key,
                       int* launch_order, int* launch_region_start, int* dropped_list, unsigned* counts);

#ifdef __cplusplus
}
#endif
#endif /* DOGERAY_AMD_H */
