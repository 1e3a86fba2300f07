// What a render launch keeps from one launch of a view to the next -- the tile order, the camera rays' tile words (grazing certificate and entry
// table), the sky split -- as plain data: each cache's state, its key and the rules that decide what a launch may reuse and what it must compute
// (DESIGN.md 4.3, 4.10).  No HIP: dr_context's three owners (context.hpp) hold the buffers and do what the rules say, and the host build exports the
// rules (tests/test_launch_state_host.py).  ODDITY marks behaviour nobody would write on purpose that is kept, as in launch_plan.hpp.
#pragma once
#include <cstdint>
#include <cstring>

#include "device_layout.h"

namespace dr {

// The view and the launch geometry a cache was made for.  Each cache compares the fields its rule names, through the functions below only.
struct ViewKey {
  float st[13] = {0};                       // settings13, compared word for word
  int W = 0, H = 0, stripe_mod = 0, stripe_rem = 0, ncols = 0, gy = 0;      // frame, stripe, tile grid (the preview divisor changes it with W and H unchanged)
  int regions = 0;                          // tile queues of the launch
  uint64_t scene_gen = 0;                   // scene uploads so far
  int cert_factor = 0, cert_levels = 0, camera_entry = 0, camera_cert = 0;      // the options the tiles' words are made from
};
inline bool same_settings(const ViewKey& a, const ViewKey& b) { return memcmp(a.st, b.st, sizeof(a.st)) == 0; }
inline bool same_grid(const ViewKey& a, const ViewKey& b) {
  return a.W == b.W && a.H == b.H && a.stripe_mod == b.stripe_mod && a.stripe_rem == b.stripe_rem && a.ncols == b.ncols && a.gy == b.gy;
}
// the tile order's geometry: frame, stripe, tile grid and queues
inline bool same_order_geometry(const ViewKey& a, const ViewKey& b) { return same_grid(a, b) && a.regions == b.regions; }
// the tile order's view.  The scene is not part of it: an order survives an upload -- any order is a valid order, and the first launch's costs refresh it
inline bool same_order_view(const ViewKey& a, const ViewKey& b) { return same_settings(a, b) && same_order_geometry(a, b); }
// the tile words' view: the queues do not matter to them, the scene and their options do
inline bool same_words_view(const ViewKey& a, const ViewKey& b) {
  return same_settings(a, b) && same_grid(a, b) && a.scene_gen == b.scene_gen && a.cert_factor == b.cert_factor && a.cert_levels == b.cert_levels &&
         a.camera_entry == b.camera_entry && a.camera_cert == b.camera_cert;
}

// ---- the tile order (cost feedback of the persistent kernel): the order of the last view, made from the costs its launches recorded
struct OrderState {
  bool valid = false;        // the order was computed for `key`
  int capacity = 0;          // tiles the buffers are sized for
  int age = 0;               // launches since the view changed
  uint64_t gen = 0;          // computations of the order so far
  ViewKey key;
  int args[5] = {0, 0, 0, 0, 0};      // the last feedback pass enqueued: tiles, regions, heavy_factor, split_steps, split_limit (dr_stats_tile_order)
};
struct OrderUse {
  bool use_order;            // the launch's queues hold the stored order
  bool record_costs;         // the launch writes its pixels' costs
  bool grow;                 // the buffers are too small: the owner makes them `capacity` tiles large first (it zeroes the capacity if it cannot)
};
// the stored order serves a launch that may not touch it (a pipelined launch beside others): computed, large enough, of the same geometry
inline bool order_serves_held(const OrderState& s, const ViewKey& key, int tiles) { return s.valid && s.capacity >= tiles && same_order_geometry(s.key, key); }
// the refresh rhythm: the first two launches of a view, then every `every`-th
inline bool order_refresh_due(int age, int every) { return age < 2 || age % every == 0; }

// What a launch of `tiles` tiles of the view `key` may do; stores the view as it goes.  feedback, follows_camera: the options; hold_order: LaunchSite's
inline OrderUse order_begin(OrderState& s, const ViewKey& key, int tiles, bool feedback, bool follows_camera, bool hold_order) {
  if (hold_order) return {order_serves_held(s, key, tiles), false, false};      // ODDITY: whatever option feedback says (switching it off has dropped the order)
  if (!feedback) return {false, false, false};
  OrderUse u = {false, true, s.capacity < tiles};
  if (u.grow) { s.capacity = tiles; s.valid = false; }      // growing loses the order
  // the stored order belongs to one view: same settings, size and stripe (progressive frames)
  if (s.valid && same_order_view(s.key, key)) u.use_order = true;
  else if (s.valid && follows_camera && same_order_geometry(s.key, key)) {
    // same frame geometry, other camera / depth / samples (an interactive viewer moving the camera, K:2341-2500: every frame is a new view): the
    // last view's costs are a better guess than none -- any order is a valid order -- and they are refreshed at once
    u.use_order = true;
    s.key = key;
    s.age = 0;
  } else { s.key = key; s.valid = false; }
  return u;
}

// After the launch (every launch of the persistent kernel, held ones included): true when the feedback pass runs behind it -- the next launch's order
// from this launch's costs.  The view does not change between the frames of a progressive render, so the order is refreshed in order_refresh_due's
// rhythm only (the two kernels take 75 us: nothing for a launch of 32 frames, 6 % of a launch of one)
inline bool order_end(OrderState& s, const OrderUse& u, int feedback_every) {
  if (u.record_costs && !u.use_order) s.age = 0;
  const bool refresh = u.record_costs && order_refresh_due(s.age, feedback_every);
  if (refresh) { s.gen++; s.valid = true; }
  s.age++;
  return refresh;
}

// The pipeline's question before the launch: will it refresh the order -- and therefore run alone, for the order and the costs are shared by all
// launches?  When a held launch could not use the order, or in a rhythm four times slower than order_end's (a refresh costs the overlap of two
// launches, 0.89 against 0.82 ms/frame when every 8th single-frame launch refreshes).  ODDITY: order_end decides with its own, faster rhythm whether
// the feedback pass really runs behind a launch that this rule sent alone
inline bool order_pipeline_refresh(const OrderState& s, const ViewKey& key, int tiles, int feedback_every) {
  return !order_serves_held(s, key, tiles) || order_refresh_due(s.age, 4 * feedback_every);
}

// ---- the camera rays' tile words: per view a word per tile, entry code << ENTRY_SHIFT | the grazing certificate's grade
struct CameraWordsState {
  bool valid = false;        // `key`'s words are computed (or known to be unusable: neither cert_ok nor entry_ok)
  bool cert_ok = false;      // ... and the view has a certificate
  bool entry_ok = false;     // ... and an entry table
  int tiles = 0;             // tiles of the keyed launch
  uint64_t gen = 0;          // computations of the words so far
  ViewKey key;
  ViewKey seen;              // the view of the last single-frame launch that found no words
  float k[CERT_MAX_LEVELS + 1] = {1};      // the margin's factor of a tile of grade g ([0] = 1; [g] = 1e-4 / the ladder's step g - 1, rounded up)
};
enum CameraWordsPlan {
  WORDS_NOT_WANTED,          // no option asks for them, or the launch does not walk a wide tree: every ray the scene's margin, from the root
  WORDS_REUSE,               // the stored words are this view's
  WORDS_SKIP_HELD,           // a pipelined launch beside others that may read them computes none: the scene's margin and the root
  WORDS_SKIP_FIRST_SIGHT,    // a single-frame launch of a view not seen before (a moving camera: every frame a new view) does not pay for the mask and the
                             // table (more than they save in one frame); the view is remembered: its second launch, or any launch of several frames, computes
  WORDS_COMPUTE
};
// want_cert, want_entry: the option is on and the scene can give one; wide: the launch walks the wide tree; batch: its frames
inline CameraWordsPlan camera_words_plan(CameraWordsState& s, const ViewKey& key, bool want_cert, bool want_entry, bool wide, int tiles, bool hold_order, int batch) {
  if ((!want_cert && !want_entry) || !wide || tiles <= 0) return WORDS_NOT_WANTED;
  if (s.valid && same_words_view(s.key, key)) return WORDS_REUSE;
  if (hold_order) return WORDS_SKIP_HELD;
  if (batch < 2 && !same_words_view(s.seen, key)) { s.seen = key; return WORDS_SKIP_FIRST_SIGHT; }
  return WORDS_COMPUTE;
}
// WORDS_COMPUTE: before anything is enqueued, the old words are gone ...
inline void camera_words_begin(CameraWordsState& s) { s.valid = false; s.cert_ok = s.entry_ok = false; s.gen++; }
// ... and once everything is, the view has words (neither flag: the view gives none, which is as good to know)
inline void camera_words_commit(CameraWordsState& s, const ViewKey& key, int tiles, bool cert_ok, bool entry_ok) {
  s.cert_ok = cert_ok; s.entry_ok = entry_ok;
  s.key = key; s.tiles = tiles; s.valid = true;
}
// after WORDS_REUSE or a committed WORDS_COMPUTE: the launch reads the words
inline bool camera_words_in_use(const CameraWordsState& s) { return s.cert_ok || s.entry_ok; }
// a certificate / an entry table can be read back (dr_stats_cert_mask, dr_stats_cert_levels, "cert_flagged_permille" / dr_stats_camera_entry); each
// read-back adds its option and its buffer
inline bool certificate_readable(const CameraWordsState& s) { return s.valid && s.cert_ok && s.tiles > 0; }
inline bool entry_table_readable(const CameraWordsState& s) { return s.valid && s.entry_ok && s.tiles > 0; }

// ---- the sky split (option sky_tiles): the launch's own order without the tiles of entry code ENTRY_NONE, and their list, kept while the words and the
// order they were split from are the same
struct SkyKey {
  uint64_t words_gen = 0;    // CameraWordsState::gen
  bool ordered = false;      // the launch uses the stored tile order ...
  uint64_t order_gen = 0;    // ... of this OrderState::gen (0 without)
  int tiles = 0, regions = 0;
};
struct SkySplitState {
  bool valid = false;        // the arrays were split from `key`
  bool last = false;         // the last launch was split (dr_stats_sky_tiles)
  SkyKey key;
};
inline SkyKey sky_key(const CameraWordsState& words, const OrderState& order, bool use_order, int tiles, int regions) {
  SkyKey k;
  k.words_gen = words.gen; k.ordered = use_order; k.order_gen = use_order ? order.gen : 0; k.tiles = tiles; k.regions = regions;
  return k;
}
inline void sky_split_commit(SkySplitState& s, const SkyKey& key) { s.key = key; s.valid = true; }      // the arrays are split from `key`
// the stored split serves the launch; room: the owner's arrays hold `key.tiles` tiles
inline bool sky_split_reusable(const SkySplitState& s, const SkyKey& key, bool room) {
  return room && s.valid && s.key.words_gen == key.words_gen && s.key.ordered == key.ordered && s.key.order_gen == key.order_gen && s.key.tiles == key.tiles &&
         s.key.regions == key.regions;
}

// ---- a launch over a subset of the view's tiles (dr_render_adaptive): the launch's own order / region_start pair holds the tiles its site names and
// none of the three caches is rewritten (the order's age counts the launch, as it counts every held one).  What the site's two fields make of a launch: it is held -- the stored order as it is (or the identity), no costs,
// no feedback pass, the view's cached tile words or none (order_begin and camera_words_plan with hold_order) -- whenever it has a subset; a subset is
// never split again for the sky (its sky tiles go through the queues: the same bits); and the queues take the subset's pair
struct SiteUse {
  bool hold;                 // what order_begin, camera_words_plan and sky_split are told for hold_order
  bool sky_split;            // the sky split may be asked at all
  bool subset_pair;          // the persistent kernel's queues hold the subset's pair
};
inline SiteUse site_use(bool hold_order, bool has_subset) { return {hold_order || has_subset, !has_subset, has_subset}; }

}  // namespace dr
