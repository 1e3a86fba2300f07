// launch_plan.hpp on the host -- the persistent kernel's plan and builds, the regions, the query kernels' plans and constants -- and device_sky.hpp: the
// sky split and the sky tiles' pixels and units.  Part of host_kernel.cpp.
extern "C" {
// launch_plan.hpp on the host (tests/test_launch_plan_host.py).  cfg6: traversal, occupancy, schedule, num_cus, coop_tiles_per_wave, count;
// out11: the build's eight template arguments (count, occ, trav_min, park_min, unroll, wide, coop, perframe), blocks, log_waves, clear_wave_log
void hk_persistent_plan(const int* cfg6, long long work, int coop_steps, int per_frame, int wave_log_on, int* out11) {
  const PersistentCfg cfg = {cfg6[0], cfg6[1], cfg6[2], cfg6[3], cfg6[4], cfg6[5] != 0};
  const PersistentPlan p = plan_persistent(cfg, work, coop_steps, per_frame != 0, wave_log_on != 0);
  const PersistentBuild& b = p.build;
  const int v[11] = {b.count, b.occ, b.trav_min, b.park_min, b.unroll, b.wide, b.coop, b.perframe, p.blocks, p.log_waves, p.clear_wave_log};
  memcpy(out11, v, sizeof(v));
}
int hk_persistent_can_store_per_frame(const int* cfg6) { return persistent_can_store_per_frame(PersistentCfg{cfg6[0], cfg6[1], cfg6[2], cfg6[3], cfg6[4], cfg6[5] != 0}); }
// the instantiations of render_persistent_kernel (DR_PERSISTENT_BUILDS), eight ints each, at most `room` of them; returns how many there are
int hk_persistent_builds(int* out, int room) {
#define HK_BUILD(COUNT, OCC, T, P, U, WIDE, COOP, PERFRAME) {COUNT, OCC, T, P, U, WIDE, COOP, PERFRAME},
  static const int builds[][8] = {DR_PERSISTENT_BUILDS(HK_BUILD)};
#undef HK_BUILD
  const int n = (int)(sizeof(builds) / sizeof(builds[0]));
  if (out && room > 0) memcpy(out, builds, sizeof(builds[0]) * (size_t)(room < n ? room : n));
  return n;
}
int hk_plan_regions(int tiles, int batch_hint, int xcd_regions, int short_one_queue, int tiles_per_wave, int num_cus) {
  return plan_regions(tiles, batch_hint, xcd_regions != 0, short_one_queue != 0, tiles_per_wave, num_cus);
}
// launch_plan.hpp plan_sky_split of the plan hk_persistent_plan returns for the same arguments
int hk_plan_sky_split(const int* cfg6, long long work, int coop_steps, int per_frame, int wave_log_on) {
  const PersistentCfg cfg = {cfg6[0], cfg6[1], cfg6[2], cfg6[3], cfg6[4], cfg6[5] != 0};
  return plan_sky_split(plan_persistent(cfg, work, coop_steps, per_frame != 0, wave_log_on != 0)) ? 1 : 0;
}
// device_split.hpp order_split_plain by SkyKeep: order may be NULL (identity); launch_region_start 2 * MAX_REGIONS + 1 ints; returns the number of sky tiles
int hk_sky_split(const int* order, const int* region_start, const uint32_t* word, int tiles, int regions, int* launch_order, int* launch_region_start, int* sky_list) {
  return order_split_plain(order, region_start, SkyKeep{word}, tiles, regions, launch_order, launch_region_start, sky_list).dropped;
}
// launch_plan.hpp's sample orders (option sample_order; tests/test_sample_order_host.py): the word RenderParams carries, and sample j of a tile as
// out2 = (pixel-in-tile, frame) through that word -- the kernel's own call
unsigned hk_sample_order_magic(int order, int batch) { return sample_order_magic(order, batch); }
void hk_tile_sample(unsigned magic, int batch, int j, int* out2) {
  const TileSample s = tile_sample(magic, batch, j);
  out2[0] = s.p; out2[1] = s.f;
}
// ... every sample of a tile at once: out[2 * j], out[2 * j + 1] for j = 0 .. 64 * batch - 1
void hk_tile_samples(int order, int batch, int* out) {
  const unsigned magic = sample_order_magic(order, batch);
  for (int j = 0; j < 64 * batch; j++) hk_tile_sample(magic, batch, j, out + 2 * j);
}
// launch_plan.hpp's ring of queue cursors (tests/test_queue_cursors_host.py): cursor_take as out3 = (block, next, wrap), and the layout's constants as
// out6 = (default stride, largest stride, line words, ring launches, words allocated, slots of a block)
void hk_cursor_take(int cursor, int stride, int skew, int* out3) {
  const CursorTake t = cursor_take(cursor, stride, skew);
  out3[0] = t.block; out3[1] = t.next; out3[2] = t.wrap ? 1 : 0;
}
void hk_cursor_layout(int* out6) {
  const int v[6] = {QUEUE_CURSOR_STRIDE, QUEUE_CURSOR_STRIDE_MAX, CURSOR_LINE_WORDS, CURSOR_RING_LAUNCHES, CURSOR_RING_ALLOC, MAX_REGIONS + 1};
  memcpy(out6, v, sizeof(v));
}
int hk_cursor_ring_blocks(int stride, int skew) { return cursor_ring_blocks(stride, skew); }
int hk_plan_split_limit(int num_cus, int occupancy, int split_parts, int split_waves) { return plan_split_limit(num_cus, occupancy, split_parts, split_waves); }
// launch_plan.hpp plan_trace: out3 = kernel (QUERY_KERNEL_*), the traversal really walked, workgroups
void hk_trace_plan(long long n, int traversal, int has_wide, int num_cus, int force, int* out3) {
  const TracePlan p = plan_trace(n, traversal, has_wide != 0, num_cus, force);
  out3[0] = p.kernel; out3[1] = p.traversal; out3[2] = p.blocks;
}
long long hk_trace_persistent_min_rays() { return TRACE_PERSISTENT_MIN_RAYS; }
int hk_allhits_max() { return ALLHITS_MAX; }
int hk_allhits_chunk() { return ALLHITS_CHUNK; }
// launch_plan.hpp plan_allhits: out3 = kernel (QUERY_KERNEL_*), wide (1 / 0), workgroups
void hk_allhits_plan(long long n, int has_wide, int num_cus, int force, int* out3) {
  const AllHitsPlan p = plan_allhits(n, has_wide != 0, num_cus, force);
  out3[0] = p.kernel; out3[1] = p.wide ? 1 : 0; out3[2] = p.blocks;
}
long long hk_allhits_persistent_min_rays() { return ALLHITS_PERSISTENT_MIN_RAYS; }
// launch_plan.hpp plan_radiance: out3 = kernel (QUERY_KERNEL_*), the traversal really walked, workgroups
void hk_radiance_plan(long long n, int traversal, int has_wide, int num_cus, int force, int* out3) {
  const RadiancePlan p = plan_radiance(n, traversal, has_wide != 0, num_cus, force);
  out3[0] = p.kernel; out3[1] = p.traversal; out3[2] = p.blocks;
}
long long hk_radiance_persistent_min_rays() { return RADIANCE_PERSISTENT_MIN_RAYS; }
int hk_radiance_chunk() { return RADIANCE_CHUNK; }
int hk_radiance_occ() { return RADIANCE_OCC; }
int hk_radiance_refill_min() { return RADIANCE_REFILL_MIN; }
int hk_radiance_park() { return RADIANCE_PARK; }
// device_sky.hpp sky_pixel summed over `frames` frames of a launch (seed, stride: dr_render_accumulate's) for n pixels (xs, ys): out[3 * n].
// Returns 0, or -1 with hk_last_error.
int hk_sky_pixel(void* hv, const float* settings13, int W, int H, float background, uint64_t seed, uint64_t stride, int frames, int n, const int* xs, const int* ys,
                 int32_t* out) {
  HkScene* h = (HkScene*)hv;
  if (!h || !settings13 || n < 0 || (n > 0 && (!xs || !ys || !out))) { hk_err = "bad argument"; return -1; }
  RenderParams P;
  if (const char* why = host_view(h->img, settings13, W, H, background, seed, 1, 0, P)) { hk_err = why; return -1; }
  fill_image(h->img, P);
  P.batch = frames; P.batch_seed_stride = stride;
  for (int i = 0; i < n; i++) {
    int r = 0, g = 0, b = 0;
    for (int f = 0; f < frames; f++) {
      int fr, fg, fb;
      sky_pixel(P, xs[i], ys[i], f, fr, fg, fb);
      r += fr; g += fg; b += fb;
    }
    out[3 * i] = r; out[3 * i + 1] = g; out[3 * i + 2] = b;
  }
  return 0;
}
// launch_plan.hpp's sky units (option sky_tiles = 2): how many a launch of `batch` frames with n_sky sky tiles has, and unit u as (position in sky_list,
// first frame, frames)
unsigned hk_sky_units(unsigned n_sky, int batch, int chunk) { return sky_units(n_sky, batch, chunk); }
void hk_sky_unit(unsigned u, int batch, int chunk, int* out3) {
  const SkyUnit s = sky_unit(u, batch, chunk);
  out3[0] = s.index; out3[1] = s.first; out3[2] = s.count;
}
// device_sky.hpp sky_tile_frames, the body the sky kernel and the persistent kernel's retiring waves share, over every unit of a launch of `batch` frames
// (seed, stride: dr_render_accumulate's) whose sky list is sky_list[n_sky], all 64 lanes of each, units in the order `perm` gives (null: ascending): added
// into acc (int32[W * H * 3], P.accumulate = 2) and, cost non-null, the cost words (unsigned[tiles * 64]) written.  Returns the units run, or -1.
long long hk_sky_units_render(void* hv, const float* settings13, int W, int H, float background, uint64_t seed, uint64_t stride, int batch, int chunk, int n_sky,
                              const int* sky_list, const unsigned* perm, int32_t* acc, unsigned* cost) {
  HkScene* h = (HkScene*)hv;
  if (!h || !settings13 || batch < 1 || n_sky < 0 || !acc || (n_sky > 0 && !sky_list)) { hk_err = "bad argument"; return -1; }
  RenderParams P;
  if (const char* why = host_view(h->img, settings13, W, H, background, seed, 1, 0, P)) { hk_err = why; return -1; }
  fill_image(h->img, P);
  P.batch = batch; P.batch_seed_stride = stride;
  P.out = acc; P.accumulate = 2;
  P.sky_chunk = sky_chunk_frames(batch, chunk);
  const unsigned n_units = sky_units((unsigned)n_sky, batch, P.sky_chunk);
  for (unsigned k = 0; k < n_units; k++) {
    const SkyUnit s = sky_unit(perm ? perm[k] : k, batch, P.sky_chunk);
    if (s.index < 0 || s.index >= n_sky || sky_list[s.index] < 0 || sky_list[s.index] >= P.ncols * P.gy) { hk_err = "unit outside the list"; return -1; }
    for (int lane = 0; lane < 64; lane++) sky_tile_frames(P, sky_list[s.index], lane, s.first, s.count, cost);
  }
  return (long long)n_units;
}
// launch_state.hpp on the host (tests/test_launch_state_host.py): one set of the three caches' states behind a handle, and the rules on it.  A view
// key is settings13 and k12 = W, H, stripe mod, stripe rem, ncols, gy, regions, scene generation, cert_factor, cert_levels, camera_entry, camera_cert
struct HkLaunchState { OrderState order; CameraWordsState words; SkySplitState sky; };
static ViewKey hk_view_key(const float* st13, const long long* k12) {
  ViewKey k;
  memcpy(k.st, st13, sizeof(k.st));
  k.W = (int)k12[0]; k.H = (int)k12[1]; k.stripe_mod = (int)k12[2]; k.stripe_rem = (int)k12[3]; k.ncols = (int)k12[4]; k.gy = (int)k12[5]; k.regions = (int)k12[6];
  k.scene_gen = (uint64_t)k12[7];
  k.cert_factor = (int)k12[8]; k.cert_levels = (int)k12[9]; k.camera_entry = (int)k12[10]; k.camera_cert = (int)k12[11];
  return k;
}
static long long* hk_put_key(const ViewKey& k, long long* out) {      // 13 words of settings13, then k12
  for (int i = 0; i < 13; i++) { uint32_t w; memcpy(&w, &k.st[i], 4); *out++ = w; }
  const long long v[12] = {k.W, k.H, k.stripe_mod, k.stripe_rem, k.ncols, k.gy, k.regions, (long long)k.scene_gen, k.cert_factor, k.cert_levels, k.camera_entry, k.camera_cert};
  memcpy(out, v, sizeof(v));
  return out + 12;
}
void* hk_launch_state_new() { return new HkLaunchState(); }
void hk_launch_state_free(void* h) { delete (HkLaunchState*)h; }
// the whole state as 96 words: order valid, capacity, age, gen, args[5], key (25); words valid, cert_ok, entry_ok, tiles, gen, key (25), seen (25);
// sky valid, last, words_gen, ordered, order_gen, tiles, regions
void hk_launch_state_read(void* h, long long* out96) {
  const HkLaunchState& s = *(HkLaunchState*)h;
  long long* o = out96;
  *o++ = s.order.valid; *o++ = s.order.capacity; *o++ = s.order.age; *o++ = (long long)s.order.gen;
  for (int a : s.order.args) *o++ = a;
  o = hk_put_key(s.order.key, o);
  *o++ = s.words.valid; *o++ = s.words.cert_ok; *o++ = s.words.entry_ok; *o++ = s.words.tiles; *o++ = (long long)s.words.gen;
  o = hk_put_key(s.words.key, o);
  o = hk_put_key(s.words.seen, o);
  *o++ = s.sky.valid; *o++ = s.sky.last; *o++ = (long long)s.sky.key.words_gen; *o++ = s.sky.key.ordered; *o++ = (long long)s.sky.key.order_gen; *o++ = s.sky.key.tiles; *o++ = s.sky.key.regions;
}
// what an option does from outside (the owners' invalidate()): which = 1 the order, 2 the words, 4 the sky split, or their sum
void hk_launch_state_invalidate(void* h, int which) {
  HkLaunchState& s = *(HkLaunchState*)h;
  if (which & 1) s.order.valid = false;
  if (which & 2) s.words.valid = false;
  if (which & 4) s.sky.valid = false;
}
// order_begin: returns use_order | record_costs << 1 | grow << 2 (the buffers are taken to grow: the capacity stays as the rule set it)
int hk_order_begin(void* h, const float* st13, const long long* k12, int tiles, int feedback, int follows_camera, int hold_order) {
  const OrderUse u = order_begin(((HkLaunchState*)h)->order, hk_view_key(st13, k12), tiles, feedback != 0, follows_camera != 0, hold_order != 0);
  return (u.use_order ? 1 : 0) | (u.record_costs ? 2 : 0) | (u.grow ? 4 : 0);
}
// order_end of the launch whose order_begin returned `use`: 1 when the feedback pass runs
int hk_order_end(void* h, int use, int feedback_every) {
  return order_end(((HkLaunchState*)h)->order, OrderUse{(use & 1) != 0, (use & 2) != 0, (use & 4) != 0}, feedback_every) ? 1 : 0;
}
int hk_order_pipeline_refresh(void* h, const float* st13, const long long* k12, int tiles, int feedback_every) {
  return order_pipeline_refresh(((HkLaunchState*)h)->order, hk_view_key(st13, k12), tiles, feedback_every) ? 1 : 0;
}
// camera_words_plan: returns the CameraWordsPlan (0 not wanted, 1 reuse, 2 skip: held, 3 skip: first sight, 4 compute)
int hk_camera_words_plan(void* h, const float* st13, const long long* k12, int want_cert, int want_entry, int wide, int tiles, int hold_order, int batch) {
  return (int)camera_words_plan(((HkLaunchState*)h)->words, hk_view_key(st13, k12), want_cert != 0, want_entry != 0, wide != 0, tiles, hold_order != 0, batch);
}
// what follows a plan of WORDS_COMPUTE: camera_words_begin and camera_words_commit with the two flags
void hk_camera_words_compute(void* h, const float* st13, const long long* k12, int tiles, int cert_ok, int entry_ok) {
  CameraWordsState& s = ((HkLaunchState*)h)->words;
  camera_words_begin(s);
  camera_words_commit(s, hk_view_key(st13, k12), tiles, cert_ok != 0, entry_ok != 0);
}
// certificate_readable | entry_table_readable << 1 | camera_words_in_use << 2
int hk_camera_words_readable(void* h) {
  const CameraWordsState& s = ((HkLaunchState*)h)->words;
  return (certificate_readable(s) ? 1 : 0) | (entry_table_readable(s) ? 2 : 0) | (camera_words_in_use(s) ? 4 : 0);
}
// a launch that is split (use_order: it uses the stored order; room: the arrays are large enough): 1 when the stored split serves it, else 0 and the
// split is made anew (sky_split_commit); `split` 0: the launch is not split at all.  Either way the state's `last` is `split`
int hk_sky_split_launch(void* h, int split, int use_order, int tiles, int regions, int room) {
  HkLaunchState& s = *(HkLaunchState*)h;
  s.sky.last = split != 0;
  if (!split) return 0;
  const SkyKey key = sky_key(s.words, s.order, use_order != 0, tiles, regions);
  if (sky_split_reusable(s.sky, key, room != 0)) return 1;
  sky_split_commit(s.sky, key);
  return 0;
}
// launch_state.hpp site_use: hold | sky_split << 1 | subset_pair << 2
int hk_site_use(int hold_order, int has_subset) {
  const SiteUse u = site_use(hold_order != 0, has_subset != 0);
  return (u.hold ? 1 : 0) | (u.sky_split ? 2 : 0) | (u.subset_pair ? 4 : 0);
}
}  // extern "C"
